"""Log-probabilities on the OpenAI-compatible routes (neural_chat/server/restful/textchat_api.py) over a stand-in
chatbot that fills `last_logprobs` the way BaseModel does when `config.logprobs` is set: response shapes of both routes,
`bytes` of a multi-byte token, `top_logprobs` cut to the requested count, stop-string truncation by `text_offset`, the
400s, and requests without the fields answering exactly as before."""
import pytest

fastapi = pytest.importorskip("fastapi")
pytest.importorskip("httpx")
from fastapi.testclient import TestClient  # noqa: E402

from intel_extension_for_transformers_amd.neural_chat.config import GenerationConfig  # noqa: E402
from intel_extension_for_transformers_amd.neural_chat.prompts import get_conv_template  # noqa: E402
from intel_extension_for_transformers_amd.neural_chat.server import create_app  # noqa: E402

PIECES = ["the", " café", " ☃", " STOP", " tail"]  # "the café ☃ STOP tail"


class _Tok:
    def __call__(self, text):
        class R:
            input_ids = text.split()
        return R


class _Bot:
    """Answers with PIECES; with config.logprobs set it leaves one entry per piece in `last_logprobs`, each with five
    alternatives (the piece itself first), as the engine streams of BaseModel do."""

    def __init__(self):
        self.model_name = "/models/tiny-llama-2-7b-chat"
        self.conv_template = get_conv_template("llama-2")
        self.tokenizer = _Tok()
        self.last_logprobs = [{"stale": True}]
        self.calls = []

    def predict(self, query, origin_query="", config=None):
        self.calls.append((query, config))
        self.last_logprobs = []
        if getattr(config, "logprobs", None) is not None:
            at = 0
            for j, p in enumerate(PIECES):
                top = [(100 + j, p, -0.25 * (j + 1))] + [(200 + 10 * j + a, "alt%d" % a, -2.0 - a) for a in range(1, 5)]
                self.last_logprobs.append({"token_id": 100 + j, "token": p, "logprob": -0.25 * (j + 1),
                                           "top": top[:config.logprobs], "text_offset": at})
                at += len(p)
        return "".join(PIECES)

    def predict_stream(self, query, origin_query="", config=None):
        self.calls.append((query, config))
        return (p for p in PIECES), []


@pytest.fixture()
def client():
    bot = _Bot()
    c = TestClient(create_app(bot))
    c.bot = bot
    return c


CHAT = {"model": "llama-2-7b-chat", "messages": [{"role": "user", "content": "Hi"}], "max_tokens": 32}
COMP = {"model": "llama-2-7b-chat", "prompt": "Once", "max_tokens": 32}


def test_generation_config_has_the_field_last():
    assert list(GenerationConfig.__dataclass_fields__)[-1] == "logprobs" and GenerationConfig().logprobs is None


def test_chat_response_carries_content_logprobs(client):
    r = client.post("/v1/chat/completions", json=dict(CHAT, logprobs=True, top_logprobs=3))
    assert r.status_code == 200, r.text
    assert client.bot.calls[-1][1].logprobs == 3
    choice = r.json()["choices"][0]
    assert choice["message"]["content"] == "".join(PIECES)
    content = choice["logprobs"]["content"]
    assert [c["token"] for c in content] == PIECES
    assert [c["logprob"] for c in content] == [-0.25, -0.5, -0.75, -1.0, -1.25]
    for c in content:
        assert set(c) == {"token", "logprob", "bytes", "top_logprobs"}
        assert len(c["top_logprobs"]) == 3 and c["top_logprobs"][0]["token"] == c["token"]
        assert all(set(t) == {"token", "logprob", "bytes"} for t in c["top_logprobs"])
        assert bytes(c["bytes"]).decode("utf-8") == c["token"]
    # multi-byte tokens: UTF-8 bytes, not code points
    assert content[1]["bytes"] == list(" café".encode("utf-8")) and len(content[1]["bytes"]) == 6
    assert content[2]["bytes"] == [0x20, 0xE2, 0x98, 0x83]
    assert content[2]["top_logprobs"][0]["bytes"] == [0x20, 0xE2, 0x98, 0x83]


def test_chat_logprobs_without_alternatives_and_n_choices(client):
    r = client.post("/v1/chat/completions", json=dict(CHAT, logprobs=True, n=2))
    assert r.status_code == 200
    assert client.bot.calls[-1][1].logprobs == 0
    for choice in r.json()["choices"]:
        assert [c["top_logprobs"] for c in choice["logprobs"]["content"]] == [[]] * len(PIECES)


def test_completion_response_carries_the_legacy_object(client):
    r = client.post("/v1/completions", json=dict(COMP, logprobs=2))
    assert r.status_code == 200, r.text
    lp = r.json()["choices"][0]["logprobs"]
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"}
    assert lp["tokens"] == PIECES and lp["token_logprobs"] == [-0.25, -0.5, -0.75, -1.0, -1.25]
    assert lp["text_offset"] == [0, 3, 8, 10, 15]
    assert lp["top_logprobs"][1] == {" café": -0.5, "alt1": -3.0}
    assert all(len(t) == 2 for t in lp["top_logprobs"])
    # echo puts the prompt in front of the text: offsets move with it
    r = client.post("/v1/completions", json=dict(COMP, logprobs=0, echo=True))
    lp = r.json()["choices"][0]["logprobs"]
    assert lp["text_offset"] == [4, 7, 12, 14, 19] and lp["top_logprobs"] == [{}] * 5


def test_stop_string_keeps_the_tokens_that_start_before_the_cut(client):
    r = client.post("/v1/chat/completions", json=dict(CHAT, logprobs=True, top_logprobs=1, stop="STOP"))
    choice = r.json()["choices"][0]
    assert choice["message"]["content"] == "the café ☃ " and choice["finish_reason"] == "stop"
    # " STOP" starts at offset 10, the cut is at 11 (its leading space is kept in the text): the token stays, " tail" goes
    assert [c["token"] for c in choice["logprobs"]["content"]] == PIECES[:4]
    r = client.post("/v1/completions", json=dict(COMP, logprobs=1, stop=[" ☃"]))
    choice = r.json()["choices"][0]
    assert choice["text"] == "the café" and choice["logprobs"]["tokens"] == PIECES[:2]
    assert choice["logprobs"]["text_offset"] == [0, 3]


@pytest.mark.parametrize("route,body,word", [
    ("/v1/chat/completions", dict(CHAT, logprobs=True, top_logprobs=21), "top_logprobs"),
    ("/v1/chat/completions", dict(CHAT, logprobs=True, top_logprobs=-1), "top_logprobs"),
    ("/v1/chat/completions", dict(CHAT, top_logprobs=2), "logprobs"),
    ("/v1/completions", dict(COMP, logprobs=6), "logprobs"),
    ("/v1/completions", dict(COMP, logprobs=-1), "logprobs"),
    ("/v1/chat/completions", dict(CHAT, logprobs=True, stream=True), "QBits: logprobs are not available on streamed"),
    ("/v1/completions", dict(COMP, logprobs=1, stream=True), "QBits: logprobs are not available on streamed"),
])
def test_bad_logprob_requests_are_answered_400(client, route, body, word):
    r = client.post(route, json=body)
    assert r.status_code == 400 and r.json()["object"] == "error" and word in r.json()["message"]
    assert not client.bot.calls


def test_requests_without_the_fields_answer_as_before(client):
    r = client.post("/v1/chat/completions", json=CHAT)
    assert r.status_code == 200 and "logprobs" not in r.json()["choices"][0]
    assert client.bot.calls[-1][1].logprobs is None
    r = client.post("/v1/chat/completions", json=dict(CHAT, logprobs=False))
    assert "logprobs" not in r.json()["choices"][0]
    r = client.post("/v1/completions", json=COMP)
    assert r.status_code == 200 and r.json()["choices"][0]["logprobs"] is None
    assert list(r.json()["choices"][0]) == ["index", "text", "logprobs", "finish_reason"]
    r = client.post("/v1/completions", json=dict(COMP, stream=True))
    assert r.status_code == 200 and '"logprobs": null' in r.text
