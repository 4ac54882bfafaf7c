"""Structured output on the OpenAI-compatible routes (neural_chat/server/restful/textchat_api.py) over a stand-in
chatbot: vLLM's `guided_choice` / `guided_regex` reach the GenerationConfig the chatbot is called with, an unsupported
pattern or both fields at once answer 400 with the builder's message, and a request without them builds the
GenerationConfig it always built. The generation behind them is GPU work (tests/test_gpu_guide_engine.py)."""
import pytest

fastapi = pytest.importorskip("fastapi")
pytest.importorskip("httpx")
from fastapi.testclient import TestClient  # noqa: E402

from intel_extension_for_transformers_amd.neural_chat import GenerationConfig  # noqa: E402
from intel_extension_for_transformers_amd.neural_chat.prompts import get_conv_template  # noqa: E402
from intel_extension_for_transformers_amd.neural_chat.server import create_app  # noqa: E402


class _Tok:
    def __call__(self, text):
        class R:
            input_ids = text.split()
        return R

    def __len__(self):
        return 32000


class _Bot:
    def __init__(self):
        self.model_name = "/models/tiny-llama-2-7b-chat"
        self.conv_template = get_conv_template("llama-2")
        self.tokenizer = _Tok()
        self.calls, self.built = [], []

    def request_guide(self, config):
        """stands in for BaseModel.request_guide: the server builds the guide once while validating"""
        self.built.append((config.guided_choice, config.guided_regex))
        if config.guided_regex == "cannot be spelled":
            raise ValueError("no sequence of tokens of this vocabulary spells a text the guide accepts")

    def predict(self, query, origin_query="", config=None):
        self.calls.append((query, config))
        return "yes"

    def predict_stream(self, query, origin_query="", config=None):
        self.calls.append((query, config))
        return iter(["ye", "s"]), []


@pytest.fixture()
def client():
    bot = _Bot()
    c = TestClient(create_app(bot))
    c.bot = bot
    return c


CHAT = {"model": "tiny-llama", "messages": [{"role": "user", "content": "hi"}]}
PLAIN = {"model": "tiny-llama", "prompt": "once upon"}
ROUTES = [("/v1/chat/completions", CHAT), ("/v1/completions", PLAIN)]


@pytest.mark.parametrize("route,body", ROUTES)
def test_the_two_fields_reach_the_generation_config(client, route, body):
    r = client.post(route, json=dict(body, guided_choice=["yes", "no"]))
    assert r.status_code == 200, r.text
    cfg = client.bot.calls[-1][1]
    assert (cfg.guided_choice, cfg.guided_regex) == (["yes", "no"], None)
    choice = r.json()["choices"][0]
    assert choice["finish_reason"] == "stop" and (choice.get("text") or choice["message"]["content"]) == "yes"
    r = client.post(route, json=dict(body, guided_regex=r"(yes|no)\d{1,3}", temperature=0.8, top_k=40, seed=5))
    assert r.status_code == 200, r.text
    cfg = client.bot.calls[-1][1]
    assert (cfg.guided_choice, cfg.guided_regex, cfg.do_sample, cfg.seed) == (None, r"(yes|no)\d{1,3}", True, 5)
    assert client.bot.built == [(["yes", "no"], None), (None, r"(yes|no)\d{1,3}")]
    # streamed requests carry them too, and end with finish_reason "stop"
    r = client.post(route, json=dict(body, guided_choice=["yes"], stream=True))
    assert r.status_code == 200 and '"finish_reason": "stop"' in r.text
    assert client.bot.calls[-1][1].guided_choice == ["yes"]


@pytest.mark.parametrize("route,body,default_max", [("/v1/chat/completions", CHAT, 512), ("/v1/completions", PLAIN, 16)])
def test_a_request_without_them_builds_the_generation_config_it_always_built(client, route, body, default_max):
    assert client.post(route, json=body).status_code == 200
    cfg = client.bot.calls[-1][1]
    before = GenerationConfig(temperature=0.7, top_p=1.0, top_k=1, repetition_penalty=1.0, max_new_tokens=default_max,
                              do_sample=False, task="chat")
    assert cfg == before and (cfg.guided_choice, cfg.guided_regex) == (None, None) and not client.bot.built


BAD = [
    (dict(guided_choice=["a"], guided_regex="a"), "guided_choice and guided_regex cannot be used together"),
    (dict(guided_choice=[]), "guided_choice is a non-empty list of non-empty strings"),
    (dict(guided_choice=["a", ""]), "guided_choice is a non-empty list of non-empty strings"),
    (dict(guided_regex="^abc"), "anchor `^`"),
    (dict(guided_regex="a(?=b)"), "look-around"),
    (dict(guided_regex=r"(a)\1"), "back-reference"),
    (dict(guided_regex="a+?"), "lazy quantifier"),
    (dict(guided_regex="(ab"), "unbalanced `(`"),
    (dict(guided_regex="cannot be spelled"), "no sequence of tokens of this vocabulary spells"),
]


@pytest.mark.parametrize("extra,message", BAD)
def test_unsupported_patterns_and_both_fields_answer_400_with_the_builders_message(client, extra, message):
    for route, body in ROUTES:
        r = client.post(route, json=dict(body, **extra))
        assert r.status_code == 400, (route, r.text)
        assert r.json()["object"] == "error" and r.json()["code"] == 400 and message in r.json()["message"]
    assert not client.bot.calls


def test_the_chatbots_guide_builder_caches_and_refuses_what_the_builder_refuses():
    """BaseModel.request_guide without a model: a stub tokenizer and an engine that only names its vocabulary."""
    from intel_extension_for_transformers_amd.neural_chat.models.base_model import BaseModel

    class Tok:
        eos_token_id = 2
        all_special_ids = [0, 1, 2]
        pieces = ["<unk>", "<s>", "</s>", "▁yes", "▁no", "y", "es", "▁", "n", "o", "1", "2"]

        def __len__(self):
            return len(self.pieces)

        def convert_ids_to_tokens(self, ids):
            return [self.pieces[i] for i in ids]

    class Engine:
        class cfg:
            vocab = 16  # a head padded past the tokenizer

    bot = BaseModel.__new__(BaseModel)
    bot.tokenizer, bot.engine = Tok(), Engine()
    assert bot.request_guide(GenerationConfig()) is None
    g = bot.request_guide(GenerationConfig(guided_choice=[" yes", " no"]))
    assert g.vocab == 16 and g.eos_ids == (2,)
    assert g.allowed(g.start).tolist() == [3, 4, 7] and 2 in g.allowed(g.walk([7, 5, 6]))
    assert bot.request_guide(GenerationConfig(guided_choice=[" yes", " no"])) is g  # per tokenizer and pattern
    r = bot.request_guide(GenerationConfig(guided_regex=r" (yes|no)[12]?"))
    assert r is not g and 2 in r.allowed(r.walk([4, 10])) and bot.request_guide(GenerationConfig(guided_regex=r" (yes|no)[12]?")) is r
    b = bot.request_guide(GenerationConfig(bad_words_ids=[[5, 6], [9]]))
    assert 9 not in b.allowed(b.start) and 6 not in b.allowed(b.prompt_state([5]))
    with pytest.raises(ValueError, match="together"):
        bot.request_guide(GenerationConfig(guided_choice=["a"], guided_regex="a"))
    with pytest.raises(ValueError, match="anchor"):
        bot.request_guide(GenerationConfig(guided_regex="a$"))
    with pytest.raises(ValueError, match="spells"):
        bot.request_guide(GenerationConfig(guided_choice=["zzz"]))
