"""The sampling controls of the OpenAI-compatible routes (neural_chat/server/restful/textchat_api.py) over a stand-in
chatbot: presence_penalty / frequency_penalty / logit_bias / min_p / seed reach the GenerationConfig the chatbot is
called with, each range error answers 400 with its message, and a request without them builds the GenerationConfig it
always built. The generation behind them is GPU work (tests/test_gpu_sampler_controls_engine.py)."""
import pytest

fastapi = pytest.importorskip("fastapi")
pytest.importorskip("httpx")
from fastapi.testclient import TestClient  # noqa: E402

from intel_extension_for_transformers_amd.neural_chat import GenerationConfig  # noqa: E402
from intel_extension_for_transformers_amd.neural_chat.prompts import get_conv_template  # noqa: E402
from intel_extension_for_transformers_amd.neural_chat.server import create_app  # noqa: E402

VOCAB = 32000


class _Tok:
    def __call__(self, text):
        class R:
            input_ids = text.split()
        return R

    def __len__(self):
        return VOCAB


class _Bot:
    def __init__(self):
        self.model_name = "/models/tiny-llama-2-7b-chat"
        self.conv_template = get_conv_template("llama-2")
        self.tokenizer = _Tok()
        self.calls = []

    def predict(self, query, origin_query="", config=None):
        self.calls.append((query, config))
        return "an answer"

    def predict_stream(self, query, origin_query="", config=None):
        self.calls.append((query, config))
        return iter(["an ", "answer"]), []


@pytest.fixture()
def client():
    bot = _Bot()
    c = TestClient(create_app(bot))
    c.bot = bot
    return c


CHAT = {"model": "tiny-llama", "messages": [{"role": "user", "content": "hi"}]}
PLAIN = {"model": "tiny-llama", "prompt": "once upon"}
CONTROLS = {"presence_penalty": 0.5, "frequency_penalty": -1.5, "min_p": 0.05, "seed": 1234,
            "logit_bias": {"17": -100, "31999": 2.5}}


@pytest.mark.parametrize("route,body", [("/v1/chat/completions", CHAT), ("/v1/completions", PLAIN)])
def test_the_controls_reach_the_generation_config(client, route, body):
    r = client.post(route, json=dict(body, temperature=0.8, top_k=40, **CONTROLS))
    assert r.status_code == 200, r.text
    cfg = client.bot.calls[-1][1]
    assert (cfg.presence_penalty, cfg.frequency_penalty, cfg.min_p, cfg.seed) == (0.5, -1.5, 0.05, 1234)
    assert cfg.logit_bias == {17: -100.0, 31999: 2.5} and cfg.do_sample
    # streamed requests carry them too
    r = client.post(route, json=dict(body, temperature=0.8, top_k=40, stream=True, **CONTROLS))
    assert r.status_code == 200
    cfg = client.bot.calls[-1][1]
    assert (cfg.presence_penalty, cfg.frequency_penalty, cfg.seed) == (0.5, -1.5, 1234) and cfg.logit_bias[17] == -100.0


def test_a_penalty_with_temperature_zero_is_a_greedy_request_that_keeps_the_penalty(client):
    r = client.post("/v1/chat/completions", json=dict(CHAT, temperature=0, frequency_penalty=1.0, presence_penalty=0.25))
    assert r.status_code == 200
    cfg = client.bot.calls[-1][1]
    assert not cfg.do_sample and (cfg.frequency_penalty, cfg.presence_penalty) == (1.0, 0.25)


@pytest.mark.parametrize("route,body,default_max", [("/v1/chat/completions", CHAT, 512), ("/v1/completions", PLAIN, 16)])
def test_defaults_build_the_generation_config_they_always_built(client, route, body, default_max):
    assert client.post(route, json=body).status_code == 200
    cfg = client.bot.calls[-1][1]
    # what TextChatAPIRouter.generation_config built before the controls existed: temperature 0.7, top_k 1 -> greedy
    before = GenerationConfig(temperature=0.7, top_p=1.0, top_k=1, repetition_penalty=1.0, max_new_tokens=default_max,
                              do_sample=False, task="chat")
    assert cfg == before
    assert (cfg.presence_penalty, cfg.frequency_penalty, cfg.min_p, cfg.logit_bias, cfg.seed) == (0.0, 0.0, 0.0, None, None)
    # explicit neutral values are the same request
    assert client.post(route, json=dict(body, presence_penalty=0, frequency_penalty=0.0, logit_bias={}, min_p=0)
                       ).status_code == 200
    assert client.bot.calls[-1][1] == before


BAD = [
    (dict(presence_penalty=2.5), "2.5 is greater than the maximum of 2 - 'presence_penalty'"),
    (dict(presence_penalty=-2.01), "-2.01 is less than the minimum of -2 - 'presence_penalty'"),
    (dict(frequency_penalty=3), "3.0 is greater than the maximum of 2 - 'frequency_penalty'"),
    (dict(frequency_penalty=-7), "-7.0 is less than the minimum of -2 - 'frequency_penalty'"),
    (dict(min_p=1.5), "1.5 is outside [0, 1] - 'min_p'"),
    (dict(min_p=-0.1), "-0.1 is outside [0, 1] - 'min_p'"),
    (dict(logit_bias={"5": 101}), "101.0 is outside [-100, 100] - 'logit_bias'"),
    (dict(logit_bias={"5": -100.5}), "-100.5 is outside [-100, 100] - 'logit_bias'"),
    (dict(logit_bias={str(i): 1.0 for i in range(301)}), "301 is greater than the maximum of 300 - 'logit_bias' entries"),
    (dict(logit_bias={"hello": 1.0}), "'hello' is not a token id - 'logit_bias'"),
    (dict(logit_bias={"1.5": 1.0}), "'1.5' is not a token id - 'logit_bias'"),
    (dict(logit_bias={"-1": 1.0}), "'-1' is not a token id of this model - 'logit_bias'"),
    (dict(logit_bias={str(VOCAB): 1.0}), "'%d' is not a token id of this model - 'logit_bias'" % VOCAB),
]


@pytest.mark.parametrize("extra,message", BAD)
def test_range_errors_answer_400_with_their_message(client, extra, message):
    for route, body in (("/v1/chat/completions", CHAT), ("/v1/completions", PLAIN)):
        r = client.post(route, json=dict(body, **extra))
        assert r.status_code == 400, (route, r.text)
        assert r.json() == {"object": "error", "message": message, "code": 400}
    assert not client.bot.calls
    # 300 entries at the bounds are fine
    ok = {str(i): (100 if i & 1 else -100) for i in range(300)}
    assert client.post("/v1/completions", json=dict(PLAIN, logit_bias=ok, presence_penalty=2, frequency_penalty=-2,
                                                    min_p=1)).status_code == 200
