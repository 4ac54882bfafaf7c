"""`prompt_logprobs` on /v1/completions (neural_chat/server/restful/textchat_api.py) over a stand-in chatbot with
`score_prompt`: the legacy object over the prompt's tokens with null first entries, one `score_prompt` call per prompt
shared by its n choices, `top_logprobs` cut to the requested count, the 400s, and a request without the field answered
with exactly the keys it has today."""
import pytest

fastapi = pytest.importorskip("fastapi")
pytest.importorskip("httpx")
from fastapi.testclient import TestClient  # noqa: E402

from intel_extension_for_transformers_amd.neural_chat.prompts import get_conv_template  # noqa: E402
from intel_extension_for_transformers_amd.neural_chat.server import create_app  # noqa: E402

PROMPT = "Once upon a ☃"
WORDS = ["Once", " upon", " a", " ☃"]


class _Tok:
    def __call__(self, text):
        class R:
            input_ids = text.split()
        return R


class _PlainBot:
    """No `score_prompt`: what a chatbot without the native engine's scoring looks like to the route."""

    def __init__(self):
        self.model_name = "/models/tiny-llama-2-7b-chat"
        self.conv_template = get_conv_template("llama-2")
        self.tokenizer = _Tok()
        self.last_logprobs = []
        self.calls, self.scored = [], []

    def predict(self, query, origin_query="", config=None):
        self.calls.append((query, config))
        return " a time"

    def predict_stream(self, query, origin_query="", config=None):
        return (p for p in [" a", " time"]), []


class _Bot(_PlainBot):
    def score_prompt(self, prompt, n_top=0):
        """entries in the shape BaseModel.score_prompt returns: five alternatives known, `n_top` of them kept"""
        self.scored.append((prompt, n_top))
        out, at = [], 0
        for j, w in enumerate(WORDS):
            top = [(300 + j, w, -0.5 * j)] + [(400 + 10 * j + a, "alt%d" % a, -3.0 - a) for a in range(1, 5)]
            out.append({"token_id": 300 + j, "token": w, "logprob": None if j == 0 else -0.5 * j,
                        "top": [] if j == 0 else top[:n_top], "text_offset": at})
            at += len(w)
        return out


def _client(bot):
    c = TestClient(create_app(bot))
    c.bot = bot
    return c


@pytest.fixture()
def client():
    return _client(_Bot())


COMP = {"model": "llama-2-7b-chat", "prompt": PROMPT, "max_tokens": 8}


def test_response_carries_the_prompt_object_with_null_first_entries(client):
    r = client.post("/v1/completions", json=dict(COMP, prompt_logprobs=2))
    assert r.status_code == 200, r.text
    choice = r.json()["choices"][0]
    assert set(choice) == {"index", "text", "logprobs", "finish_reason", "prompt_logprobs"}
    assert choice["text"] == " a time" and choice["logprobs"] is None
    pl = choice["prompt_logprobs"]
    assert set(pl) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"}
    assert pl["tokens"] == WORDS
    assert pl["token_logprobs"] == [None, -0.5, -1.0, -1.5]
    assert pl["top_logprobs"][0] is None
    assert pl["top_logprobs"][3] == {" ☃": -1.5, "alt1": -4.0}
    assert pl["text_offset"] == [0, 4, 9, 11]
    assert client.bot.scored == [(PROMPT, 2)]


def test_n_choices_share_one_score_and_every_prompt_gets_its_own(client):
    r = client.post("/v1/completions", json=dict(COMP, n=2, prompt_logprobs=0))
    assert r.status_code == 200, r.text
    choices = r.json()["choices"]
    assert len(choices) == 2 and choices[0]["prompt_logprobs"] == choices[1]["prompt_logprobs"]
    assert client.bot.scored == [(PROMPT, 0)] and len(client.bot.calls) == 2
    assert choices[0]["prompt_logprobs"]["top_logprobs"] == [None, {}, {}, {}]
    r = client.post("/v1/completions", json=dict(COMP, prompt=[PROMPT, "Twice"], n=2, prompt_logprobs=1))
    assert r.status_code == 200 and len(r.json()["choices"]) == 4
    assert client.bot.scored[1:] == [(PROMPT, 1), ("Twice", 1)]


@pytest.mark.parametrize("n_top", [0, 1, 3, 5])
def test_top_logprobs_are_cut_to_the_requested_count(client, n_top):
    r = client.post("/v1/completions", json=dict(COMP, prompt_logprobs=n_top))
    assert r.status_code == 200, r.text
    top = r.json()["choices"][0]["prompt_logprobs"]["top_logprobs"]
    assert top[0] is None and all(len(t) == n_top for t in top[1:])


def test_it_goes_with_echo_and_generated_logprobs_unchanged(client):
    plain = client.post("/v1/completions", json=dict(COMP, echo=True, logprobs=0)).json()["choices"][0]
    both = client.post("/v1/completions", json=dict(COMP, echo=True, logprobs=0, prompt_logprobs=1)).json()["choices"][0]
    assert both.pop("prompt_logprobs")["tokens"] == WORDS
    assert both == plain and plain["text"] == PROMPT + " a time"


@pytest.mark.parametrize("extra", [dict(prompt_logprobs=21), dict(prompt_logprobs=-1),
                                   dict(prompt_logprobs=1, stream=True)])
def test_bad_requests_are_400(client, extra):
    r = client.post("/v1/completions", json=dict(COMP, **extra))
    assert r.status_code == 400, r.text
    assert r.json()["object"] == "error" and "prompt_logprobs" in r.json()["message"]
    assert client.bot.scored == [] and client.bot.calls == []


def test_a_bot_without_score_prompt_is_400():
    c = _client(_PlainBot())
    r = c.post("/v1/completions", json=dict(COMP, prompt_logprobs=1))
    assert r.status_code == 400 and "prompt_logprobs" in r.json()["message"]
    assert c.bot.calls == []
    assert c.post("/v1/completions", json=COMP).status_code == 200


def test_requests_without_the_field_answer_with_the_keys_they_have_today(client):
    r = client.post("/v1/completions", json=COMP)
    assert r.status_code == 200, r.text
    body = r.json()
    assert set(body) == {"id", "object", "created", "model", "choices", "usage"}
    assert set(body["choices"][0]) == {"index", "text", "logprobs", "finish_reason"}
    assert client.bot.scored == []
    # the chat route does not take the field: it is ignored there like any unknown key, nothing is scored
    chat = {"model": "llama-2-7b-chat", "messages": [{"role": "user", "content": "Hi"}], "max_tokens": 8}
    r = client.post("/v1/chat/completions", json=dict(chat, prompt_logprobs=3))
    assert r.status_code == 200 and "prompt_logprobs" not in r.json()["choices"][0]
    assert client.bot.scored == []
