"""Sparse mixture-of-experts layers on the engine: random-init Mixtral (E 4, k 2), Qwen3-MoE (E 8, k 3, no renorm) and a
Qwen3-MoE whose layer 0 is dense, at the geometry of tests/test_gpu_moe_model.py with 128 positions and head_dim 64
(the smallest the engine's attention takes), int4 g32. The
reference is that file's float64 twin (dequantised weights, HF's eager expert loop); every comparison is under the
model-level bound 2e-3 * max|ref| + 1e-4 of tests/test_gpu_model_coverage.py. Precondition, on the CPU: in the twin, at
every sparse layer and position used, p_k - p_(k+1) >= 1e-3 (router logits are of order 0.2, the bound moves them by
about 1e-4), so the engine's fp32 routing picks the twin's experts.
"""
import numpy as np
import pytest
import torch

from tests import test_gpu_moe_model as M

pytestmark = pytest.mark.gpu

GEOM = dict(M.GEOM, max_position_embeddings=128, head_dim=64)  # the engine's attention takes head_dim 64 or 128
STEPS = 8
# kind -> (model seed, 7-token prompt, 70-token prompt): fixed inputs for which the routing-margin precondition holds
# (with 8 experts and 70 rows no seed meets it under an arbitrary prompt: the tokens were picked position by position
# against the twin's margins; the condition itself is asserted in _twin_logits on every run)
INPUTS = {
    "mixtral": (1, [21, 44, 77, 119, 21, 72, 33],
        [21, 44, 77, 119, 21, 72, 107, 21, 41, 82, 4, 44, 65, 107, 21, 44, 89, 10, 44, 77, 118, 21, 65, 89, 10, 44, 77,
        118, 21, 49, 89, 10, 44, 89, 118, 21, 65, 89, 21, 44, 87, 118, 21, 65, 100, 21, 44, 87, 118, 21, 65,
        118, 21, 44, 87, 10, 44, 65, 118, 21, 44, 87, 10, 44, 87, 118, 21, 65, 87, 10]),
    "qwen3_moe": (1, [16, 39, 75, 121, 35, 68, 114],
        [16, 39, 75, 121, 35, 68, 114, 23, 59, 84, 117, 45, 64, 105, 9, 59, 87, 118, 43, 64, 105, 14, 68, 105, 11, 35,
        69, 120, 35, 63, 92, 14, 35, 92, 119, 30, 75, 104, 17, 37, 78, 121, 18, 63, 96, 18, 46, 86, 6, 43, 78,
        103, 14, 54, 92, 119, 42, 78, 103, 16, 66, 104, 6, 45, 66, 120, 18, 70, 94, 1]),
    "qwen3_moe_dense0": (1, [12, 38, 74, 114, 25, 72, 24],
        [12, 38, 74, 114, 25, 72, 111, 25, 43, 79, 116, 38, 76, 116, 24, 59, 103, 118, 38, 82, 104, 25, 57, 99, 13, 42,
        78, 111, 24, 55, 89, 17, 55, 82, 111, 19, 55, 111, 11, 57, 76, 111, 19, 76, 111, 19, 58, 76, 118, 26,
        74, 111, 11, 57, 82, 122, 30, 76, 111, 19, 57, 103, 13, 48, 82, 111, 11, 48, 103, 9]),
}
_BUILT = {}


def _config(kind):
    from transformers import MixtralConfig, Qwen3MoeConfig

    if kind == "mixtral":
        return MixtralConfig(**GEOM, intermediate_size=96, num_local_experts=4, num_experts_per_tok=2)
    return Qwen3MoeConfig(**GEOM, intermediate_size=96, moe_intermediate_size=96, num_experts=8, num_experts_per_tok=3,
                          norm_topk_prob=False, mlp_only_layers=[0] if kind == "qwen3_moe_dense0" else [])


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    def get(kind):
        from transformers import AutoModelForCausalLM as HF

        from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers
        from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM, RtnConfig

        if kind not in _BUILT:
            path = str(tmp_path_factory.mktemp(kind))
            torch.manual_seed(INPUTS[kind][0])
            HF.from_config(_config(kind)).float().save_pretrained(path)
            q = AutoModelForCausalLM.from_pretrained(path, quantization_config=RtnConfig(bits=4, group_size=32))
            _BUILT[kind] = (q, M._twin(path, q), optimize_transformers(q, max_ctx=128))
        return _BUILT[kind]

    yield get
    _BUILT.clear()


def _twin_logits(twin, tokens):
    """float64 logits [T, vocab] of the twin, after asserting the routing-margin precondition at every sparse layer"""
    gaps = []

    def hook(mod, args, out):
        p = torch.softmax(out[0].double(), dim=-1).sort(dim=-1, descending=True).values
        gaps.append(float((p[:, mod.top_k - 1] - p[:, mod.top_k]).min()))

    hooks = [m.register_forward_hook(hook) for m in twin.modules() if type(m).__name__.endswith("TopKRouter")]
    try:
        with torch.no_grad():
            ref = twin(torch.tensor([tokens])).logits[0].numpy()
    finally:
        for h in hooks:
            h.remove()
    assert gaps and min(gaps) >= 1e-3, gaps
    return ref


@pytest.mark.parametrize("kind", ["mixtral", "qwen3_moe", "qwen3_moe_dense0"])
def test_prompt_pass_and_greedy_steps_match_the_twin(built, kind):
    q, twin, eng = built(kind)
    # all-sparse models hand activations over as XQ blocks (the combine emits them); the dense layer's I = 96 keeps the
    # third model on the fp32-activation step, where the combine only adds
    assert eng.uses_xq() == (kind != "qwen3_moe_dense0")
    _, prompt7, prompt70 = INPUTS[kind]
    for prompt, what in ((prompt7, "7 tokens, grouped form"), (prompt70, "70 tokens, prompt form")):
        got = eng.prefill(prompt)[0].cpu().numpy()
        M._within(got, _twin_logits(twin, prompt)[-1], "%s prompt pass (%s)" % (kind, what))
    runs = {}
    for mode in ("eager", "graph"):
        eng.prefill(prompt7)  # greedy: the first new token and its position are in place
        toks, rows = [int(eng.token.item())], []
        if mode == "graph":
            eng.capture(greedy=True)
        for _ in range(STEPS):
            eng.replay_graph(1) if mode == "graph" else eng.run(1, greedy=True)
            torch.cuda.synchronize()
            rows.append(eng.logits.cpu().numpy())
            toks.append(int(eng.token.item()))
        runs[mode] = (toks, np.stack(rows))
    toks, rows = runs["eager"]
    ref = _twin_logits(twin, prompt7 + toks[:-1])
    for i in range(STEPS):  # step i fed toks[i] at position 7 + i: the twin's row 7 + i over the engine's own tokens
        M._within(rows[i], ref[len(prompt7) + i], "%s step %d" % (kind, i))
    assert runs["graph"][0] == toks
    assert np.array_equal(runs["graph"][1].view(np.uint32), rows.view(np.uint32))


@pytest.mark.parametrize("case", ["nf4_experts", "lora_down_proj", "tp_mixtral", "tp_qwen3_moe"])
def test_refusals_carry_a_qbits_message(built, case):
    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers
    from intel_extension_for_transformers_amd.runtime.tp import tp_supports

    if case.startswith("tp_"):
        ok, reason = tp_supports(_config(case[3:]))
        assert not ok and reason.startswith("QBits:")
        return
    q, _, eng = built("mixtral")
    with pytest.raises(RuntimeError, match="QBits:"):
        if case == "nf4_experts":
            experts = next(iter(M._experts_of(q).values()))
            experts.weight_dtype = "nf4"
            try:
                optimize_transformers(q, max_ctx=128)
            finally:
                experts.weight_dtype = "int4_clip"
        else:
            eng.set_lora({(1, "down_proj"): (torch.zeros(2, 96), torch.zeros(128, 2), 1.0)})
