"""The fused decode engine on the model families beyond Llama-2 / Mistral: scaled RoPE (llama3, linear, yarn), Qwen2
(q / k / v biases) and Qwen3 (per-head q / k norm, tied head), against the HF module path of the SAME quantised model in
fp32 — `qmodel(ids).logits` and `_woq_hf_generate`, as tests/test_gpu_api.py::test_optimize_transformers_engine_matches_hf_path.

Random-weight HF models, seeded; biases drawn with std 0.5 and norm weights in [0.5, 1.5] (HF initialises them to 0 and
1, which would hide a missing bias or an unapplied weight). Bounds: decode logits 2e-3 * max|ref| + 1e-4 (the project's
bound for this comparison), prompt pass 1e-2 * max|ref| + 1e-3 (PF_TOL of tests/test_gpu_engine.py), and under teacher
forcing the engine's argmax is an id whose reference logit lies within the decode bound of the reference maximum.
"""
import numpy as np
import pytest
import torch

from tests import kv_shift_reference as KR

pytestmark = pytest.mark.gpu

N_PROMPT, N_FORCED, MAX_CTX = 40, 8, 128
ORIG = 64
ROPE = {
    "llama3": dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                   original_max_position_embeddings=ORIG),
    "linear": dict(rope_type="linear", factor=4.0),
    "yarn": dict(rope_type="yarn", factor=4.0, original_max_position_embeddings=ORIG),
}
TINY = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
            head_dim=64, vocab_size=320, rms_norm_eps=1e-5, tie_word_embeddings=False)
# the fused qkv + attention launch's geometry: hidden 4096 (32 K tiles), head_dim 128
WIDE = dict(TINY, hidden_size=4096, num_attention_heads=2, num_key_value_heads=1, head_dim=128)
KINDS = ("llama3", "linear", "yarn", "qwen2", "qwen3", "qwen3_tied", "qwen2_wide", "qwen3_wide")


def _fp_model(kind):
    from transformers import LlamaConfig, LlamaForCausalLM, Qwen2Config, Qwen2ForCausalLM, Qwen3Config, Qwen3ForCausalLM

    torch.manual_seed(17)
    geom = WIDE if kind.endswith("_wide") else TINY
    if kind in ROPE:
        mpe = {"llama3": 512, "linear": 256, "yarn": 256}[kind]
        model = LlamaForCausalLM(LlamaConfig(**geom, max_position_embeddings=mpe,
                                             rope_parameters=dict(ROPE[kind], rope_theta=10000.0)))
    elif kind.startswith("qwen2"):
        model = Qwen2ForCausalLM(Qwen2Config(**geom, max_position_embeddings=256))
    else:
        model = Qwen3ForCausalLM(Qwen3Config(**dict(geom, tie_word_embeddings=kind == "qwen3_tied"),
                                             max_position_embeddings=256))
    g = torch.Generator().manual_seed(23)
    for name, p in model.named_parameters():
        if name.endswith("_proj.bias"):
            torch.nn.init.normal_(p, std=0.5, generator=g)
        elif "norm" in name:
            with torch.no_grad():
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
    model.generation_config.eos_token_id = None  # random weights: never stop early
    return model.float().eval()


class Case:
    """one quantised model, its reference rows (computed once, read-only) and an engine over it"""

    def __init__(self, kind, path):
        from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM, RtnConfig

        self.kind = kind
        _fp_model(kind).save_pretrained(str(path))
        self.qmodel = AutoModelForCausalLM.from_pretrained(
            str(path), quantization_config=RtnConfig(bits=4, group_size=128, scale_dtype="fp16"))
        rng = np.random.default_rng(5)
        self.prompt = [int(t) for t in rng.integers(3, 320, N_PROMPT)]
        ids = torch.tensor([self.prompt], device="cuda")
        with torch.no_grad():
            out = self.qmodel._woq_hf_generate(ids, max_new_tokens=N_FORCED, do_sample=False)
            self.forced = out[0, N_PROMPT:].tolist()
            self.ref = self.qmodel(out).logits[0].float().cpu().numpy()  # row p: the logits after position p
        self.ref.setflags(write=False)
        assert len(self.forced) == N_FORCED

    def engine(self):
        from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers

        return optimize_transformers(self.qmodel, max_ctx=MAX_CTX, kv_dtype=torch.float16)


_CASES = {}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    def get(kind):
        if kind not in _CASES:
            _CASES[kind] = Case(kind, tmp_path_factory.mktemp(kind))
        return _CASES[kind]

    yield get
    _CASES.clear()


def _dec_bound(ref):
    return 2e-3 * float(np.abs(ref).max()) + 1e-4


def _step(eng, token, pos):
    eng.token.fill_(int(token))
    eng.pos.fill_(int(pos))
    eng.step(greedy=False)
    return eng.logits.float().cpu().numpy()


def _check_engine(case, eng):
    """the three checks of every model: step-by-step decode, teacher-forced greedy agreement, prompt pass"""
    ref = case.ref
    seq = case.prompt + case.forced
    worst = 0.0
    for p in range(N_PROMPT + N_FORCED):
        got = _step(eng, seq[p], p)
        if p in (0, 1, N_PROMPT - 1):
            err = float(np.abs(got - ref[p]).max())
            worst = max(worst, err / _dec_bound(ref[p]))
            assert err <= _dec_bound(ref[p]), (case.kind, "decode step", p, err, _dec_bound(ref[p]))
        if p >= N_PROMPT:  # fed the reference's token: the engine's pick is one the reference (nearly) ties for
            a = int(got.argmax())
            assert ref[p][a] >= ref[p].max() - _dec_bound(ref[p]), (case.kind, "teacher-forced step", p, a,
                                                                   int(ref[p].argmax()))
    got = eng.prefill(case.prompt, greedy=False)[0].float().cpu().numpy()
    r = ref[N_PROMPT - 1]
    perr, pbound = float(np.abs(got - r).max()), 1e-2 * float(np.abs(r).max()) + 1e-3
    print("\n%s: decode worst err/bound %.3f, prompt pass err/bound %.3f" % (case.kind, worst, perr / pbound))
    assert perr <= pbound, (case.kind, "prompt pass", perr, pbound)
    assert eng.status() == 0


@pytest.mark.parametrize("kind", ["llama3", "linear", "yarn", "qwen2", "qwen3", "qwen3_tied"])
def test_engine_matches_the_hf_module_path(cases, kind):
    """llama3, qwen2 and qwen3 raise in optimize_transformers without this feature (rope scaling / model_type)"""
    case = cases(kind)
    eng = case.engine()
    assert eng.uses_xq()
    if kind == "qwen3_tied":
        assert case.qmodel.config.tie_word_embeddings
        assert case.qmodel.lm_head.weight.data_ptr() == case.qmodel.model.embed_tokens.weight.data_ptr()
    _check_engine(case, eng)


@pytest.mark.parametrize("kind", ["qwen2", "qwen3"])
def test_fp32_activation_step_carries_the_extras(cases, kind, monkeypatch):
    monkeypatch.setenv("WOQ_ENGINE_XQ", "0")
    case = cases(kind)
    eng = case.engine()
    assert not eng.uses_xq()
    _check_engine(case, eng)


@pytest.mark.parametrize("kind", ["qwen2_wide", "qwen3_wide"])
def test_fused_qkv_attention_launch_carries_the_extras(cases, kind):
    case = cases(kind)
    eng = case.engine()
    assert eng.uses_fused_attn()
    _check_engine(case, eng)
    # the fused launch and the separate launches: the same bits
    seq = case.prompt
    logits = {}
    for fuse in (True, False):
        eng.set_fuse_attn(fuse)
        assert eng.uses_fused_attn() == fuse
        logits[fuse] = [_step(eng, seq[p], p) for p in range(6)]
    for p in (0, 5):
        assert np.array_equal(logits[True][p].view(np.uint32), logits[False][p].view(np.uint32)), (kind, p)
    # a replayed graph gives the eager tokens
    eng.set_fuse_attn(True)
    tokens = {}
    for mode in ("eager", "graph"):
        eng.prefill(case.prompt[:8], greedy=True)
        first = int(eng.token.item())
        if mode == "graph":
            eng.capture(greedy=True)
            for _ in range(6):
                eng.replay(1)
        else:
            for _ in range(6):
                eng.step(greedy=True)
        tokens[mode] = [first] + eng.token_log()[8:14].tolist()
    assert tokens["graph"] == tokens["eager"] and eng.status() == 0


@pytest.mark.parametrize("kind", ["qwen2", "qwen3"])
def test_model_generate_goes_through_the_engine(cases, kind):
    case = cases(kind)
    q = case.qmodel
    if hasattr(q, "woq_engine"):
        del q.woq_engine
    ids = torch.tensor([case.prompt[:12]], device="cuda")
    out = q.generate(ids, max_new_tokens=6, do_sample=False)
    assert getattr(q, "woq_engine", None) is not None and tuple(out.shape) == (1, 18)
    del q.woq_engine


def test_streaming_request_on_llama3_tables_matches_the_shift_reference(cases):
    """The K re-rotation by table row n_discard holds for per-dimension frequencies: a streaming request on the
    llama3-scaled model runs, and a shift of its cache equals tests/kv_shift_reference.py's float64 operation applied
    with THAT model's table row — K within one fp16 unit (the streaming engine test's bound for the shift), V bit for bit."""
    from intel_extension_for_transformers_amd.runtime.engine import (StreamingConfig, build_rope_tables,
                                                                     optimize_transformers, rope_scaling_of)

    case = cases("llama3")
    ctx, keep, discard = 32, 4, 14
    eng = optimize_transformers(case.qmodel, max_ctx=ctx, kv_dtype=torch.float16)
    cfg = case.qmodel.config
    cos, sin = build_rope_tables(ctx, 64, 10000.0, "cpu", rope_scaling=rope_scaling_of(cfg)[1],
                                 max_position_embeddings=cfg.max_position_embeddings)
    plain = build_rope_tables(ctx, 64, 10000.0, "cpu")
    assert not torch.equal(cos[discard], plain[0][discard])  # the scaled row is not the plain one
    for p in range(ctx):  # fill the cache
        _step(eng, (case.prompt + case.forced)[p], p)
    k0, v0 = KR.bits_of(eng.kv_cache("k")[0]), KR.bits_of(eng.kv_cache("v")[0])  # [layers][ctx][kv heads][D]
    eng.kv_shift(keep, discard, ctx, move_pos=False)
    k1, v1 = KR.bits_of(eng.kv_cache("k")[0]), KR.bits_of(eng.kv_cache("v")[0])
    want_k, want_v = KR.shift_reference(k0, v0, "fp16", cos[discard].numpy().astype(np.float64),
                                        sin[discard].numpy().astype(np.float64), keep, discard, ctx)
    assert KR.ulp_distance(k1[:, keep:ctx - discard], want_k, "fp16").max() <= KR.MAX_ULP
    assert np.array_equal(v1[:, keep:ctx - discard], want_v) and np.array_equal(k1[:, :keep], k0[:, :keep])
    # and whole requests past the cache run, the same tokens however they are launched
    stream = StreamingConfig(ctx_size=ctx, n_keep=keep, n_discard=discard)
    outs = [eng.generate(case.prompt[:6], 60, burst=b, streaming=stream) for b in (16, 5)]
    assert len(outs[0]) == 60 and outs[0] == outs[1] and eng.status() == 0 and eng.discarded() == 0


def test_refusals_name_their_cause(cases, tmp_path):
    from intel_extension_for_transformers_amd.runtime.engine import (StreamingConfig, WoqDecoderEngine,
                                                                     optimize_transformers)

    # yarn tables are scaled by an attention factor: no rolling cache over them
    eng = cases("yarn").engine()
    assert eng.rope_attention_factor != 1.0
    with pytest.raises(RuntimeError, match="attention factor"):
        eng.generate([5, 6, 7], 4, streaming=StreamingConfig(ctx_size=32, n_keep=4, n_discard=8))
    with pytest.raises(RuntimeError, match="attention factor"):
        eng.kv_shift(1, 1, 4)
    # mixed layer_types
    q = cases("qwen2").qmodel
    saved = q.config.layer_types
    q.config.layer_types = ["full_attention", "sliding_attention"]
    try:
        with pytest.raises(RuntimeError, match="layer_types"):
            optimize_transformers(q, max_ctx=64)
    finally:
        q.config.layer_types = saved
    # two of the three biases
    k_proj = q.model.layers[1].self_attn.k_proj
    bias = k_proj.bias
    k_proj.bias = None
    try:
        with pytest.raises(RuntimeError, match="k_proj.bias missing"):
            optimize_transformers(q, max_ctx=64)
    finally:
        k_proj.bias = bias
    # extras on a tensor-parallel engine
    tp = WoqDecoderEngine(256, 512, 4, 2, 64, 1, 320, max_ctx=64, tp_rank=0, tp_size=2)
    with pytest.raises(RuntimeError, match="tensor-parallel"):
        tp.set_layer_extras(0, qkv_bias=torch.zeros(512))
    good = cases("qwen2").engine()
    # half a q / k norm, on one GPU
    with pytest.raises(RuntimeError, match="q_norm and k_norm"):
        good.set_layer_extras(0, q_norm=torch.ones(64))
