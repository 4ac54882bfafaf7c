"""tests/woq_backward_reference.py against independent statements of the same gradient, and the plumbing of the new
entry points; no GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import woq_backward_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("wname,asym,act_order", [("int4_clip", False, False), ("int4_clip", True, True),
                                                  ("int8", True, False), ("nf4", False, False)])
def test_reference_vs_central_differences(wname, asym, act_order):
    """f(x) = sum(G * (x W)) is linear in x, so a central difference is its gradient up to float64 rounding"""
    K, N, group, M = 96, 17, 32, 3
    d = R.weight(K, N, group, wname, asym, act_order)
    rng = np.random.default_rng(1)
    x, G = rng.standard_normal((M, K)), rng.standard_normal((M, N))
    dX, S = R.backward(G, d["W"], d["shuffle"])
    f = lambda v: float((G * R.forward(v, d["W"], d["shuffle"])).sum())  # noqa: E731
    h = 2.0 ** -8 * max(1.0, float(np.abs(d["W"]).max()))
    num = np.empty_like(dX)
    for m in range(M):
        for k in range(K):
            e = np.zeros_like(x)
            e[m, k] = h
            num[m, k] = (f(x + e) - f(x - e)) / (2 * h)
    # rounding of the two evaluations: at most (terms) x 2^-53 of the sum of magnitudes F each, divided by 2h
    F = float((np.abs(G) @ np.abs(d["W"]).T).sum()) * (float(np.abs(x).max()) + h)
    assert np.abs(num - dX).max() <= M * N * K * 2.0 ** -53 * F / h
    assert (S >= np.abs(dX) * (1 - 1e-12)).all()
    assert (np.abs(dX - dX) <= R.bound(G, d["W"], S)).all()  # the float64 statement meets its own bound


def test_unshuffle_vs_index_select_autograd():
    """the act-order un-shuffle is the transpose of index_select: torch's own autograd says the same"""
    K, N, group, M = 128, 24, 32, 5
    d = R.weight(K, N, group, "int4_clip", True, True)
    assert sorted(d["shuffle"].tolist()) == list(range(K)) and not np.array_equal(d["shuffle"], np.arange(K))
    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.standard_normal((M, K))).requires_grad_(True)
    G = rng.standard_normal((M, N))
    y = torch.index_select(x, 1, torch.from_numpy(d["shuffle"].copy())) @ torch.from_numpy(d["W"].copy())
    (torch.from_numpy(G) * y).sum().backward()
    dX, _ = R.backward(G, d["W"], d["shuffle"])
    assert np.abs(x.grad.numpy() - dX).max() <= 1e-12 * np.abs(dX).max()
    # convert_idx is the stable sort of the raw g_idx by group
    assert np.array_equal(d["shuffle"], np.argsort(d["g_idx"], kind="stable"))


def test_abi_and_binding_carry_the_backward_entry_points():
    """include/woq_hip.h, _lib.EXPORTS, qbits.__all__, INTEGRATION.md and the Makefile name the two entry points; the
    ABI version stays 4"""
    import ctypes

    from intel_extension_for_transformers_amd import _lib, qbits

    header = open(os.path.join(ROOT, "include", "woq_hip.h")).read()
    declared = set(re.findall(r"WOQ_API[^;(]*?\b(woq_\w+)\s*\(", header))
    new = {"woq_linear_backward", "woq_linear_backward_workspace"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    assert declared == set(_lib.EXPORTS)
    assert "#define WOQ_ABI_VERSION 4" in header
    assert {"woq_linear_backward", "woq_linear_backward_workspace"} <= set(qbits.__all__)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integration for n in new)
    makefile = open(os.path.join(ROOT, "intel_extension_for_transformers_amd", "csrc", "Makefile")).read()
    assert "woq_linear_bwd.hip" in makefile
    if os.path.exists(_lib.LIB_PATH):
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for n in new:
            getattr(lib, n)


def test_matmul_kbit_training_form_no_longer_raises_not_implemented():
    """do_dequant=True goes through MatMulKBit; without a device it fails on the missing device, not on a missing
    training form"""
    from intel_extension_for_transformers_amd.transformers.llm.quantization.autograd import MatMulKBit, matmul_kbit

    assert issubclass(MatMulKBit, torch.autograd.Function)
    a = torch.zeros(2, 32, requires_grad=True)
    blob = torch.zeros(1024, dtype=torch.int8)
    try:
        matmul_kbit(a, blob, None, None, "fp32", "int4_clip", "fp32", "sym", do_dequant=True)
    except NotImplementedError:
        pytest.fail("the training form still raises NotImplementedError")
    except RuntimeError as e:
        assert "QBits:" in str(e)
    else:
        pytest.fail("a host blob was accepted")
    # the flag with nothing to differentiate (no grad on A or a bias, or grad mode off) is not a training call
    for grad_mode, act in ((True, a.detach()), (False, a)):
        with torch.set_grad_enabled(grad_mode), pytest.raises(NotImplementedError, match="do_dequant=False"):
            matmul_kbit(act, blob, None, None, "fp32", "int4_clip", "fp32", "sym", do_dequant=True)


def test_lora_config_and_exports():
    from intel_extension_for_transformers_amd import transformers as T

    for n in ("LoraConfig", "QuantizedLoraLinearQBits", "prepare_model_for_kbit_training", "get_peft_model"):
        assert n in T.__all__ and getattr(T, n) is not None
    c = T.LoraConfig()
    assert (c.r, c.lora_alpha, c.lora_dropout, c.bias, c.task_type) == (8, 16, 0.0, "none", "CAUSAL_LM")
    assert c.target_modules == ["k_proj", "o_proj", "q_proj", "v_proj"] and c.to_dict()["peft_type"] == "LORA"
    with pytest.raises(ValueError, match="bias"):
        T.LoraConfig(bias="lora_only")
