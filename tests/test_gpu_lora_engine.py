"""The decode engine with unmerged LoRA adapters installed (`WoqDecoderEngine.set_lora`, csrc/woq_engine.hip +
csrc/woq_lora.hip), stage by stage and against float64.

The model is the tiny 2-layer Llama of tests/test_gpu_qlora_model.py (hidden 128, inter 256, 4 heads of 64, int4 g32)
wrapped by `get_peft_model` (r 4, alpha 8) with lora_A and lora_B both drawn (tests/lora_twin.py `random_adapters`, seed
0): a fresh adapter has B = 0 and would show nothing. Two adapters: all seven targets, and q_proj / v_proj only.

Stages. The engine's decode step (by phase and as one step) and its prompt pass must equal, byte for byte, the probe
chain of tests/lora_stage_shadow.py, in which the delta probe's output is the `bias` of the existing GEMV probes and the
rows probes stand where the engine places them: the XQ step (separate qkv and attention launches: the plan this model
gets), the fp32-activation step (WOQ_ENGINE_XQ=0), a prompt pass and its second chunk, an eager burst against a replayed
graph. The fused qkv + attention launch needs more K tiles than hidden 128 has, so that form runs on the hidden-4096
geometry of tests/test_gpu_attention_fullgeom.py with drawn adapters of rank 8.

float64. Last-position logits of the prompt pass and of the decode step after it against tests/lora_twin.py (dense
dequantised weights + s B A, the engine's fp16 head), under the measure tests/test_gpu_engine.py applies to the
adapter-less engine — max|got - ref| <= 2e-3 max|ref| + 1e-4 for a decode step, 1e-2 max|ref| + 1e-3 for a prompt pass —
plus the twin's derived LoRA term; and the same logits must differ from the adapter-less engine's by more than that.
(On an MI355X: error 0.08 / 0.15 of the tolerance for the prompt pass / the decode step with all seven targets, the
adapter's effect 119 / 481 times it.)

State: `clear_lora()` gives the adapter-less bytes back; another adapter of the same targets keeps the captured graph
(`engine.captured`, as the guide tests read it, and a replay that runs); on / off drop it; every refusal leaves the next
step's bytes as they were.
"""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import engine_stage_shadow as S
from tests import lora_stage_shadow as LS
from tests import lora_twin as TW

pytestmark = pytest.mark.gpu

PROMPT = [98, 106, 15, 76, 10, 36]
ALL7, QV = TW.PROJ, ("q_proj", "v_proj")
R_, ALPHA = 4, 8


def _wrapped(targets, seed=0, fp=None):
    """-> (the tiny model quantised and wrapped with drawn adapters on `targets`, the adapters as numpy)"""
    from intel_extension_for_transformers_amd.transformers import LoraConfig, get_peft_model, prepare_model_for_kbit_training
    from tests.test_gpu_qlora_model import _quantised, _tiny_llama

    q = _quantised(fp if fp is not None else _tiny_llama())
    q = get_peft_model(prepare_model_for_kbit_training(q), LoraConfig(r=R_, lora_alpha=ALPHA, target_modules=list(targets)))
    shapes = {t: (m.in_features, m.out_features) for n, m in q.model.layers[0].named_modules()
              for t in [n.rpartition(".")[2]] if t in TW.PROJ}
    ad = TW.random_adapters(shapes, len(q.model.layers), targets, R_, ALPHA, seed)
    with torch.no_grad():
        for name, m in q.named_modules():
            if hasattr(m, "lora_A"):
                parts = name.split(".")
                a, b, _ = ad[(int(parts[parts.index("layers") + 1]), parts[-1])]
                m.lora_A["default"].weight.copy_(torch.from_numpy(a))
                m.lora_B["default"].weight.copy_(torch.from_numpy(b))
    return q.eval(), ad


def _engine(targets, seed=0):
    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers

    q, ad = _wrapped(targets, seed)
    eng = optimize_transformers(q, max_ctx=64, adapters="unmerged")
    assert eng.lora_on and q.woq_engine is eng and q._woq_engine_off is False
    return q, eng, ad


def _torch_entries(ad):
    return {k: (torch.from_numpy(a), torch.from_numpy(b), s) for k, (a, b, s) in ad.items()}


def _check_decode(eng, ad, xq, case):
    assert eng.uses_xq() == xq, case
    w, lw = S.Wiring(eng), LS.LoraWiring(eng, _torch_entries(ad))
    for which in ("k", "v"):  # rows the step must not read, and its own row, hold finite garbage
        eng.kv_cache(which).view(torch.uint8)[:, :, int(eng.pos.item()):] = 0x3C
    torch.cuda.synchronize()
    snap = S.snapshot(eng)
    phases, after = S.engine_decode_trace(eng, by_phase=True)
    assert eng.status() == 0
    S.restore(eng, snap)
    whole, after2 = S.engine_decode_trace(eng, by_phase=False)
    assert S.first_difference(S.whole_step_view(phases), whole) is None, (case, "phases != step()")
    assert all(np.array_equal(after[x], after2[x]) for x in ("k", "v")), (case, "phases != step(): cache")
    S.restore(eng, snap)
    st = S.ShadowState(snap, eng.device)
    shadow = LS.shadow_decode_step(w, lw, st, xq, S.attn_options(eng))
    assert int(st.status.item()) == 0
    diff = S.first_difference(phases, shadow)
    assert diff is None, (case, "engine != probe chain, first at", diff)
    for which, t in (("k", st.k), ("v", st.v)):
        assert np.array_equal(S._raw(t), after[which]), (case, which, "caches differ")
    return phases


@pytest.mark.parametrize("targets", [ALL7, QV], ids=["all-seven", "q-v"])
def test_xq_step_separate_launches_equals_probe_chain(targets):
    _, eng, ad = _engine(targets)
    assert eng.attn_plan()["form"] == L.ATTN_PER_HEAD  # hidden 128: below what the fused launch covers
    eng.prefill(PROMPT, greedy=True)
    with_adapter = _check_decode(eng, ad, True, "xq step %d targets" % len(targets))
    # ... and the chain notices an adapter that is left out: the same step without the delta probes differs
    st = S.ShadowState(S.snapshot(eng), eng.device)  # (_check_decode put the state back)
    plain = LS.shadow_decode_step(S.Wiring(eng), LS.LoraWiring(eng, {}), st, True, S.attn_options(eng))
    assert S.first_difference(with_adapter, plain) is not None


@pytest.mark.parametrize("targets", [ALL7, QV], ids=["all-seven", "q-v"])
def test_fp32_activation_step_equals_probe_chain(targets, monkeypatch):
    monkeypatch.setenv("WOQ_ENGINE_XQ", "0")
    _, eng, ad = _engine(targets)
    eng.prefill(PROMPT, greedy=True)
    _check_decode(eng, ad, False, "fp32 step %d targets" % len(targets))


@pytest.mark.parametrize("targets", [ALL7, QV], ids=["all-seven", "q-v"])
def test_xq_step_fused_qkv_attention_equals_probe_chain(targets):
    from tests.test_gpu_attention_fullgeom import build_attention_geometry

    eng = build_attention_geometry(kv_heads=8, max_ctx=256, max_batch=1)[0]
    shapes = {t: eng._lora_shape(t) for t in TW.PROJ}
    ad = TW.random_adapters(shapes, eng.cfg.layers, targets, 8, 16, seed=3, b_scale=0.02)
    eng.set_lora(_torch_entries(ad))
    assert eng.lora_on and eng.attn_plan()["form"] == L.ATTN_FUSED
    eng.prefill(np.random.default_rng(41).integers(0, 512, 20).tolist(), greedy=True)
    _check_decode(eng, ad, True, "fused launch %d targets" % len(targets))


@pytest.mark.parametrize("targets", [ALL7, QV], ids=["all-seven", "q-v"])
def test_prompt_pass_and_its_second_chunk_equal_probe_chain(targets):
    _, eng, ad = _engine(targets)
    w, lw = S.Wiring(eng), LS.LoraWiring(eng, _torch_entries(ad))
    tokens = PROMPT + [7, 300 % 128, 12, 45, 99, 3, 64]  # 13 rows: ragged against every tile
    for which in ("k", "v"):
        eng.kv_cache(which).view(torch.uint8)[:] = 0x3C
    torch.cuda.synchronize()
    for start, chunk in ((0, tokens[:8]), (8, tokens[8:])):
        snap = S.snapshot(eng)
        got, _ = S.engine_prefill_trace(eng, chunk, start)
        st = S.ShadowState(snap, eng.device)
        want = LS.shadow_prefill(w, lw, st, chunk, start)
        diff = S.first_difference(got, want)
        assert diff is None, ("prompt pass from %d" % start, "engine != probe chain, first at", diff)


def test_eager_burst_equals_replayed_graph():
    _, eng, _ = _engine(ALL7)
    eng.launch = "graph"
    eng.prefill(PROMPT, greedy=True)
    snap = S.snapshot(eng)
    eng.capture(greedy=True)
    eng.replay_graph(11)  # one launch of the 8-step graph and three single steps
    torch.cuda.synchronize()
    a = (eng.token_log()[:24].clone(), eng.logits.clone(), S._raw(eng.kv_cache("k")), S._raw(eng.kv_cache("v")))
    S.restore(eng, snap)
    eng.run(11, greedy=True)
    torch.cuda.synchronize()
    assert eng.status() == 0
    assert torch.equal(a[0], eng.token_log()[:24]) and torch.equal(a[1].view(torch.int32), eng.logits.view(torch.int32))
    assert np.array_equal(a[2], S._raw(eng.kv_cache("k"))) and np.array_equal(a[3], S._raw(eng.kv_cache("v")))


@pytest.mark.parametrize("targets", [ALL7, QV], ids=["all-seven", "q-v"])
def test_last_position_logits_against_the_float64_twin(targets):
    from tests.test_gpu_qlora_model import _deq

    q, eng, ad = _engine(targets)
    twin = TW.twin_from_quantised(q, _deq, ad)
    assert sorted(TW.adapters_of(q)) == sorted(ad)
    worst = {}
    # the prompt pass, then one decode step fed the twin's own next token
    got_pf = eng.prefill(PROMPT, greedy=False)[0].double().cpu().numpy()
    ref_all, ltol = twin.forward(PROMPT)
    ref_pf = ref_all[-1]
    tol_pf = 1e-2 * np.abs(ref_pf).max() + 1e-3 + ltol
    nxt = int(ref_pf.argmax())
    eng.token.fill_(nxt)
    eng.pos.fill_(len(PROMPT))
    eng.step(greedy=False)
    got_dec = eng.logits.double().cpu().numpy()
    ref_dec_all, ltol2 = twin.forward(PROMPT + [nxt])
    ref_dec = ref_dec_all[-1]
    tol_dec = 2e-3 * np.abs(ref_dec).max() + 1e-4 + ltol2
    worst["prompt pass"] = float(np.abs(got_pf - ref_pf).max() / tol_pf)
    worst["decode step"] = float(np.abs(got_dec - ref_dec).max() / tol_dec)
    # the adapter is not ignored: without it the engine's logits leave the tolerance by far
    eng.clear_lora()
    assert not eng.lora_on
    base_pf = eng.prefill(PROMPT, greedy=False)[0].double().cpu().numpy()
    eng.token.fill_(nxt)
    eng.pos.fill_(len(PROMPT))
    eng.step(greedy=False)
    base_dec = eng.logits.double().cpu().numpy()
    effect = (float(np.abs(got_pf - base_pf).max() / tol_pf), float(np.abs(got_dec - base_dec).max() / tol_dec))
    print("\n%d targets: worst err / tolerance %s; adapter's effect / tolerance: prompt pass %.1f, decode step %.1f"
          % (len(targets), ", ".join("%s %.3f" % kv for kv in worst.items()), *effect))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert min(effect) > 1.0, effect


def _step_bytes(eng):
    """the bytes one greedy step from a fixed state leaves (state restored afterwards)"""
    eng.prefill(PROMPT, greedy=True)
    snap = S.snapshot(eng)
    tr, _ = S.engine_decode_trace(eng, by_phase=False)
    S.restore(eng, snap)
    return tr


def test_clear_returns_the_adapterless_bytes_and_graphs_follow_the_targets():
    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers
    from tests.test_gpu_qlora_model import _quantised, _tiny_llama

    plain = optimize_transformers(_quantised(_tiny_llama()), max_ctx=64)
    want_plain = _step_bytes(plain)
    q, eng, ad = _engine(ALL7)
    first = _step_bytes(eng)
    assert S.first_difference(first, want_plain) is not None
    # another adapter of the same targets and rank: the captured graph stays and replays the new values
    eng.launch = "graph"
    eng.prefill(PROMPT, greedy=True)
    eng.capture(greedy=True)
    assert eng.captured
    q2, ad2 = _wrapped(ALL7, seed=5)
    eng.set_lora(q2)
    assert eng.captured and eng.lora_on
    second = _step_bytes(eng)
    assert S.first_difference(second, first) is not None
    eng.prefill(PROMPT, greedy=True)
    eng.replay_graph(1)
    torch.cuda.synchronize()
    assert S._raw(eng.logits).tobytes() == dict(second)["head"]["logits"].tobytes()
    # an adapter with fewer targets changes which launches a step holds: the graph goes
    eng.set_lora(_wrapped(QV, seed=5)[0])
    assert not eng.captured
    with pytest.raises(RuntimeError, match="not captured"):
        eng.replay_graph(1)
    eng.capture(greedy=True)
    eng.clear_lora()
    assert not eng.captured and not eng.lora_on
    with pytest.raises(RuntimeError, match="not captured"):
        eng.replay_graph(1)
    assert S.first_difference(_step_bytes(eng), want_plain) is None
    # and on again: the first adapter's bytes
    eng.set_lora(q)
    assert not eng.captured and S.first_difference(_step_bytes(eng), first) is None


def test_refusals_leave_the_engine_as_it_was():
    from intel_extension_for_transformers_amd.runtime import WoqDecoderEngine
    from tests.test_gpu_engine import _tiny

    _, eng, ad = _engine(QV)
    want = _step_bytes(eng)
    shapes = {t: eng._lora_shape(t) for t in TW.PROJ}
    big = _torch_entries(TW.random_adapters(shapes, 2, QV, 8, 16, seed=1))
    with pytest.raises(RuntimeError, match="QBits.*r_max"):  # reserved at rank 4
        eng.set_lora(big)
    assert S.first_difference(_step_bytes(eng), want) is None
    with pytest.raises(RuntimeError, match="QBits.*r_max"):  # the native check itself
        a, b, s = big[(0, "q_proj")]
        L.check(L.lib().woq_engine_set_lora(eng._h, 0, 0, a.cuda().data_ptr(), b.cuda().data_ptr(), 8, s))
    assert S.first_difference(_step_bytes(eng), want) is None
    bad = dict(_torch_entries(ad))
    a, b, s = bad[(1, "v_proj")]
    bad[(1, "v_proj")] = (a[:, :64].contiguous(), b, s)
    with pytest.raises(RuntimeError, match="QBits.*lora_A"):  # a shape mismatch, before anything is copied
        eng.set_lora(bad)
    with pytest.raises(RuntimeError, match="QBits: bad layer index"):
        L.check(L.lib().woq_engine_set_lora(eng._h, 2, 0, None, None, 0, 0.0))
    with pytest.raises(RuntimeError, match="QBits.*once"):
        L.check(L.lib().woq_engine_lora_reserve(eng._h, 4))
    assert S.first_difference(_step_bytes(eng), want) is None and eng.lora_on

    one = {(0, "q_proj"): _torch_entries(ad)[(0, "q_proj")]}
    # set before reserve
    fresh = _tiny(128, False, "fp16", seed=2)[0]
    with pytest.raises(RuntimeError, match="QBits.*woq_engine_lora_reserve"):
        L.check(L.lib().woq_engine_set_lora(fresh._h, 0, 0, None, None, 0, 0.0))
    # fp8-weight layers: their engine GEMV takes no bias
    fp8 = _tiny(128, False, "fp16", seed=2, weight_dtype="fp8_e4m3")[0]
    fp8.token.fill_(5)
    fp8.pos.fill_(0)
    fp8.step(greedy=False)
    before = S._raw(fp8.logits).tobytes()
    shapes8 = {t: fp8._lora_shape(t) for t in TW.PROJ}
    with pytest.raises(RuntimeError, match="QBits: fp8-weight layers"):
        fp8.set_lora(_torch_entries(TW.random_adapters(shapes8, 2, QV, 4, 8, seed=1)))
    assert not fp8.lora_on
    fp8.pos.fill_(0)
    fp8.step(greedy=False)
    assert S._raw(fp8.logits).tobytes() == before
    # a tensor-parallel engine, and a layer that is not set
    c = eng.cfg
    tp = WoqDecoderEngine(c.hidden, c.inter, c.heads, c.kv_heads, c.head_dim, c.layers, c.vocab, max_ctx=64, tp_rank=0, tp_size=2)
    with pytest.raises(RuntimeError, match="QBits: LoRA adapters run on one GPU"):
        tp.set_lora(one)
    bare = WoqDecoderEngine(c.hidden, c.inter, c.heads, c.kv_heads, c.head_dim, c.layers, c.vocab, max_ctx=64)
    with pytest.raises(RuntimeError, match="QBits: woq_engine_set_lora comes after woq_engine_set_layer"):
        bare.set_lora(one)
    assert not bare.lora_on and not tp.lora_on
