"""The float64 statement of AWQ (tests/awq_reference.py) checked against itself and against the RTN reference, and the
scale folding of quantization/awq.py checked to be function-preserving on tiny fp32 models. No GPU needed."""
import copy

import numpy as np
import pytest
import torch

from tests import awq_reference as A
from tests import gptq_reference as G
from tests import quant_reference as Q

SHAPES = [(256, 96, 64), (200, 70, 32)]  # the second: a short last group


@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("K,N,group", SHAPES)
def test_loss_from_h_is_the_loss_from_the_activations(K, N, group, asym):
    w, X = A.salient(K, N, seed=K)
    H, a = A.stats(X)
    for i in (0, 7, 19):
        D = A.scale_delta(w, A.scale_of(a, i), group, 4, asym)["D"]
        lh, lx = A.loss_from_h(D, H), A.loss_from_x(D, X)
        assert abs(lh - lx) <= 1e-12 * lx  # two float64 evaluations of one number


@pytest.mark.parametrize("bits,asym", [(4, False), (4, True), (8, False), (8, True)])
@pytest.mark.parametrize("K,N,group", SHAPES)
def test_candidate_zero_is_plain_rtn(K, N, group, bits, asym):
    w, X = A.salient(K, N, seed=1)
    H, a = A.stats(X)
    rtn = Q.quantize(w, group, A.WNAME[bits], asym)
    s0 = A.scale_of(a, 0)
    assert (s0 == 1.0).all()
    r = A.scale_delta(w, s0, group, bits, asym)
    assert np.array_equal(r["D"], rtn["deq"] - w) and np.array_equal(r["code"], rtn["code"])
    # clip candidate 0 clamps nothing: its loss is RTN's, cell by cell, and a search of one candidate returns w
    c = A.clip_search(w, H, group, bits, asym, n_cand=1)
    assert np.array_equal(c["w_out"], w.astype(np.float64)) and (c["best"] == 0).all()
    d = rtn["deq"] - w
    g, n_groups = Q.group_of(K, group)
    for gi in range(n_groups):
        rows = slice(gi * g, min(K, (gi + 1) * g))
        assert np.array_equal(c["losses"][0, gi], (d[rows] * (H[rows, rows] @ d[rows])).sum(0))
    full = A.clip_search(w, H, group, bits, asym)
    assert np.array_equal(full["losses"][0], c["losses"][0])
    picked = np.take_along_axis(full["losses"], full["best"][None], 0)[0]
    assert (picked <= full["losses"][0]).all()
    if bits == 4:  # with 16 levels giving up the range's ends pays in many cells (with 256 it rarely does)
        assert (full["best"] > 0).mean() > 0.3


def test_auto_scale_is_never_worse_than_rtn_and_finds_the_salient_channels():
    w, X = A.salient(256, 96, seed=3)
    H, a = A.stats(X)
    r = A.auto_scale([w], H, a, 64, 4, False)
    assert r["losses"][r["best"]] <= r["losses"][0] and r["best"] > 0
    assert r["losses"][0] / r["losses"][r["best"]] > 1.5


@pytest.mark.parametrize("K,N,group", SHAPES)
def test_h_scaled_is_the_gram_matrix_of_the_scaled_input(K, N, group):
    w, X = A.salient(K, N, seed=5)
    H, a = A.stats(X)
    s = A.scale_of(a, 9)
    H2, _ = A.stats(X.astype(np.float64) / s)
    Hs = A.h_scaled(H, s)
    assert np.abs(Hs - H2).max() <= 1e-12 * np.abs(H2).max()
    # and the clip loss under it is the output error of the scaled linear on the scaled input
    ws = w.astype(np.float64) * s[:, None]
    lo, hi = A.clamp_of(ws, group, False, 0.8)
    d = Q.quantize(np.clip(ws, lo, hi), group, "int4_clip", False)["deq"] - ws
    g, n_groups = Q.group_of(K, group)
    rows = slice(g, min(K, 2 * g))
    dz = np.zeros_like(d)
    dz[rows] = d[rows]
    want = A.loss_from_x(dz, X.astype(np.float64) / s)
    got = float((d[rows] * (Hs[rows, rows] @ d[rows])).sum())
    assert abs(got - want) <= 1e-11 * want


def test_correlated_inputs_are_clipped():
    """on the GPTQ family's inputs the clip search clips most cells and beats RTN clearly (what the GPU test relies on)"""
    w, H = G.correlated(256, 96, seed=256)
    r = A.clip_search(w, H, 32, 4, False)
    picked = np.take_along_axis(r["losses"], r["best"][None], 0)[0]
    assert (r["best"] > 0).mean() > 0.5 and r["losses"][0].sum() / picked.sum() > 1.2


# ---- scale folding ---------------------------------------------------------------------------------------------------
def _tiny(kind):
    from transformers import LlamaConfig, LlamaForCausalLM, Qwen2Config, Qwen2ForCausalLM

    torch.manual_seed(0)
    kw = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=2 if kind == "gqa" else 4, vocab_size=256, max_position_embeddings=128,
              rms_norm_eps=1e-5, tie_word_embeddings=False)
    if kind == "qwen2":
        model = Qwen2ForCausalLM(Qwen2Config(**kw))
        assert model.model.layers[0].self_attn.q_proj.bias is not None
        for layer in model.model.layers:  # zero-initialised biases would hide a bias that is not folded
            for p in (layer.self_attn.q_proj, layer.self_attn.k_proj, layer.self_attn.v_proj):
                torch.nn.init.normal_(p.bias, std=0.5)
    else:
        model = LlamaForCausalLM(LlamaConfig(head_dim=64, **kw))
    return model.float().eval()


@pytest.mark.parametrize("kind", ["mha", "gqa", "qwen2"])
def test_scale_folding_preserves_the_function(kind):
    from intel_extension_for_transformers_amd.transformers.llm.quantization import awq
    from intel_extension_for_transformers_amd.transformers.llm.quantization.calibration import (
        ABSORB_GROUPS, absorb_groups, block_linears as _block_linears)

    model = _tiny(kind)
    ids = torch.randint(0, 256, (2, 24), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = model(ids).logits.double()
    folded = copy.deepcopy(model)
    gen = torch.Generator().manual_seed(3)
    for block in folded.model.layers:
        groups = absorb_groups(block, _block_linears(block, "model.layers", []), "test", "AWQ")
        assert groups == ([0, 2, 3] if kind == "gqa" else [0, 1, 2, 3])  # grouped-query attention: no o_proj scale
        scales = {}
        for gi in groups:
            k = block.get_submodule(ABSORB_GROUPS[gi][0][0]).in_features
            scales[gi] = torch.exp(torch.empty(k).uniform_(-1.5, 1.5, generator=gen))  # 0.22 .. 4.5
        before = {n: p.detach().clone() for n, p in block.named_parameters()}
        awq.apply_scales(block, scales)
        changed = {n for n, p in block.named_parameters() if not torch.equal(p, before[n])}
        expect = {"input_layernorm.weight", "post_attention_layernorm.weight", "self_attn.q_proj.weight",
                  "self_attn.k_proj.weight", "self_attn.v_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight",
                  "mlp.down_proj.weight"}
        if kind != "gqa":
            expect |= {"self_attn.o_proj.weight"} | ({"self_attn.v_proj.bias"} if kind == "qwen2" else set())
        assert changed == expect  # q / k / v biases (but v's under the o_proj scale) and everything else untouched
    with torch.no_grad():
        got = folded(ids).logits.double()
    # Folding replaces w by fl(w s) and g by fl(g / s): one fp32 rounding (2^-24 relative) on each factor of every
    # product x g w that feeds a linear. The four folds of a layer touch the inputs of its seven linears and the
    # outputs of two; a relative perturbation of 2 * 2^-24 per folded linear, plus the changed rounding of the fp32
    # dot products themselves (sqrt(K) 2^-24 for random signs, K <= 256), passes through the residual stream to the
    # logits with gain about one. Per layer: 9 * 2 * 2^-24 + 7 * 16 * 2^-24 = 130 * 2^-24, two layers, and a factor 4
    # for the worst element over the mean: 2 * 4 * 130 * 2^-24 = 6.2e-5 of the logits' scale.
    bound = 2 * 4 * 130 * 2.0 ** -24 * want.abs().max().item()
    err = (got - want).abs().max().item()
    print("%s: max |dlogit| %.3g, bound %.3g" % (kind, err, bound))
    assert err <= bound
