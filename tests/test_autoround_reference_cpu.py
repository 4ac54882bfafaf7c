"""AutoRound without a GPU: the float64 reference (tests/autoround_reference.py) against torch.autograd and against the
RTN reference, the learning-rate schedule, what a request can be refused for before a device is touched, and the three
entry points in the header and the binding."""
import os
import re

import numpy as np
import pytest
import torch

from tests import autoround_reference as R
from tests import quant_reference as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WNAME = {4: "int4_clip", 8: "int8"}


def _ste(x):
    return (torch.round(x) - x).detach() + x


def _autograd(w, V, alpha, beta, gout, group, bits, asym):
    """the straight-through expressions of the issue in float64 torch -> (W~, dV, dalpha, dbeta)"""
    w = torch.tensor(np.asarray(w, np.float64))
    V = torch.tensor(np.asarray(V, np.float64), requires_grad=True)
    alpha = torch.tensor(np.asarray(alpha, np.float64), requires_grad=True)
    beta = torch.tensor(np.asarray(beta, np.float64), requires_grad=True)
    K, N = w.shape
    g, G = R.group_of(K, group)
    L, qmax, off = R.consts(bits)
    parts = []
    for gi in range(G):
        rows = slice(gi * g, min(K, (gi + 1) * g))
        v = w[rows]
        mn = torch.clamp(v.min(0).values, max=0.0)
        mx = torch.clamp(v.max(0).values, min=0.0)
        if asym:
            lo, hi = alpha[gi] * mn, beta[gi] * mx
            s0 = (hi - lo) / L
            s = torch.where(s0 == 0, torch.ones_like(s0), s0)
            z = torch.clamp(_ste(-lo / s), 0, L)
            c = torch.clamp(_ste(v / s + V[rows]) + z, 0, L)
            parts.append((c - z) * s)
        else:
            a, b = beta[gi] * mx, alpha[gi] * (-mn)
            s0 = torch.where(a >= b, a, b) / qmax
            s = torch.where(s0 == 0, torch.ones_like(s0), s0)
            c = torch.clamp(_ste(v / s + V[rows]), -off, qmax)
            parts.append(c * s)
    wq = torch.cat(parts)
    (wq * torch.tensor(np.asarray(gout, np.float64))).sum().backward()
    return wq.detach().numpy(), V.grad.numpy(), alpha.grad.numpy(), beta.grad.numpy()


@pytest.mark.parametrize("asym", [True, False])
@pytest.mark.parametrize("K,N,group,bits", [(200, 24, 64, 4), (96, 17, 32, 8), (160, 12, -1, 4)])
def test_reference_gradients_equal_autograd(K, N, group, bits, asym):
    """the closed-form gradients against torch.autograd of the straight-through expressions, float64, to 1e-12
    relative; (200, 64) has a short last group"""
    w, V, alpha, beta, gout = R.inputs(K, N, group, bits, asym, seed=3)
    f = R.forward(w, V, alpha, beta, group, bits, asym)
    gr = R.gradients(w, V, alpha, beta, gout, group, bits, asym, f)
    wq, dV, dalpha, dbeta = _autograd(w, V, alpha, beta, gout, group, bits, asym)
    assert np.array_equal(wq, f["deq"])
    assert f["clipped"].any() and (~f["clipped"]).any()
    for name, ref, auto in (("dV", gr["dV"], dV), ("dalpha", gr["dalpha"], dalpha), ("dbeta", gr["dbeta"], dbeta)):
        err = np.abs(ref - auto).max() / np.abs(auto).max()
        print("%s bits %d asym %d: max |ref - autograd| / max |autograd| = %.3g" % (name, bits, asym, err))
        assert np.abs(ref - auto).max() <= 1e-12 * np.abs(auto).max(), name
    assert (gr["dalpha"][0, 0], gr["dbeta"][0, 0]) == (0.0, 0.0)  # the all-zero cell: s was replaced by 1
    if not asym:
        assert (gr["dalpha"] == 0)[f["beta_side"]].all() and (gr["dbeta"] == 0)[~f["beta_side"]].all()
    # the bound's sums dominate the gradients they bound
    assert (np.abs(gr["dalpha"]) <= gr["sum_a"] * (1 + 1e-12)).all()
    assert (np.abs(gr["dbeta"]) <= gr["sum_b"] * (1 + 1e-12)).all()


@pytest.mark.parametrize("asym", [True, False])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("K,N,group", Q.SHAPES)
def test_neutral_parameters_are_rtn(K, N, group, bits, asym):
    """V = 0, alpha = beta = 1 is the package's RTN rule, exactly, on the RTN tests' own input families"""
    w, _, _ = Q.families(K, N, group, WNAME[bits], asym)
    G = R.group_of(K, group)[1]
    f = R.forward(w, np.zeros((K, N)), np.ones((G, N)), np.ones((G, N)), group, bits, asym)
    ref = Q.quantize(w, group, WNAME[bits], asym)
    assert np.array_equal(f["deq"], ref["deq"]) and np.array_equal(f["s"], ref["s"])
    if asym:
        assert np.array_equal(f["z"], ref["z"])


def test_inputs_are_what_the_kernel_tests_expect():
    for asym in (True, False):
        w, V, alpha, beta, gout = R.inputs(256, 48, 32, 4, asym, seed=0)
        assert all(a.dtype == np.float32 for a in (w, V, alpha, beta, gout))
        assert (w[:32, 0] == 0).all() and (w[:32, 1] > 0).all() and (w[-32:, 2] < 0).all()
        assert (V == 0.5).mean() > 0.05 and (V == -0.5).mean() > 0.05 and np.abs(V).max() == 0.5
        assert 0.1 < (alpha == 1).mean() < 0.3 and alpha.min() >= 0.5 and beta.min() >= 0.5
        w2 = R.inputs(256, 48, 32, 4, asym, seed=0)[0]
        assert np.array_equal(w, w2)


def test_sign_step_and_schedule():
    from intel_extension_for_transformers_amd.transformers import AutoRoundConfig
    from intel_extension_for_transformers_amd.transformers.llm.quantization import autoround

    p = np.array([0.49, -0.5, 0.0, 0.2, 1.0])
    grad = np.array([-1e-30, 3.0, 0.0, 2.0, -0.0])
    assert np.array_equal(R.sign_step(p, grad, 0.05, -0.5, 0.5), np.array([0.5, -0.5, 0.0, 0.2 - 0.05, 0.5]))
    assert R.schedule(0.005, 0, 200) == 0.005 and R.schedule(0.005, 100, 200) == 0.0025
    assert R.schedule(0.005, 199, 200) == pytest.approx(0.005 / 200)
    assert R.default_lrs(None, None, 200) == (0.005, 0.005) and R.default_lrs(0.01, None, 200) == (0.01, 0.01)
    assert R.default_lrs(None, 0.02, 50) == (0.02, 0.02) and R.default_lrs(0.01, 0.1, 50) == (0.01, 0.1)
    # the driver's own statement of both
    for kw in (dict(), dict(lr=0.01), dict(minmax_lr=0.02, iters=50), dict(lr=0.01, minmax_lr=0.1, iters=50)):
        c = AutoRoundConfig(**kw)
        iters, lr, mm = autoround.learning_rates(c)
        assert iters == c.iters and (lr, mm) == R.default_lrs(c.lr, c.minmax_lr, c.iters)
    assert autoround.learning_rates(AutoRoundConfig(iters=0)) == (0, 0.0, 0.0)
    for t in (0, 1, 77, 199):
        assert autoround.schedule(0.005, t, 200) == R.schedule(0.005, t, 200)


# ---- refusals, before a device is touched ------------------------------------------------------------------------------
class _Blocks(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.model = torch.nn.Module()
        self.model.layers = torch.nn.ModuleList([torch.nn.Linear(32, 32)])
        self.lm_head = torch.nn.Linear(32, 2)


class _Flat(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.linear = torch.nn.Linear(32, 2)


IDS = [torch.zeros(2, 8, dtype=torch.long)]


def _cfg(**kw):
    from intel_extension_for_transformers_amd.transformers import AutoRoundConfig

    c = AutoRoundConfig(**kw)
    c.post_init_hip()
    return c


def _convert(model, cfg):
    from intel_extension_for_transformers_amd.transformers.llm.quantization.utils import convert_to_quantized_model

    return convert_to_quantized_model(model, cfg, device="cuda")


@pytest.mark.parametrize("option", ["use_double_quant", "layer_wise", "quant_lm_head"])
def test_unsupported_options_raise_by_name(option):
    with pytest.raises(NotImplementedError, match=option):
        _convert(_Blocks(), _cfg(calib_dataloader=IDS, **{option: True}))


def test_float_weight_types_raise():
    with pytest.raises(NotImplementedError, match="nf4"):
        _convert(_Blocks(), _cfg(calib_dataloader=IDS, weight_dtype="nf4", sym=True))


def test_model_without_decoder_blocks_is_named():
    with pytest.raises(NotImplementedError, match="_Flat"):
        _convert(_Flat(), _cfg(calib_dataloader=IDS))


def test_no_calibration_data_raises_as_awq_does():
    for kw in (dict(), dict(dataset="wikitext2")):
        with pytest.raises(NotImplementedError) as e:
            _convert(_Blocks(), _cfg(**kw))
        assert str(e.value).startswith("AutoRoundConfig calibration is not part of the MI355X hot path without "
                                       "calibration data")
        assert "calib_dataloader" in str(e.value)


def test_teq_keeps_raising():
    from intel_extension_for_transformers_amd.transformers import TeqConfig

    c = TeqConfig()
    c.post_init_hip()
    with pytest.raises(NotImplementedError, match="calibration is not part"):
        _convert(_Blocks(), c)


def test_calibration_data_is_kept_by_reference_and_not_serialised():
    from intel_extension_for_transformers_amd.transformers import AutoRoundConfig

    c = _cfg(calib_dataloader=IDS, n_samples=3, seq_len=5)
    assert c.calib_dataloader is IDS and "calib_dataloader" not in c.to_dict()
    assert "calib_dataloader" not in c.to_json_string(use_diff=False)
    back = AutoRoundConfig.from_dict(c.to_dict())
    assert back.calib_dataloader is None and back.iters == c.iters and back.group_size == c.group_size
    assert AutoRoundConfig().calib_dataloader is None


def test_abi_and_binding_carry_the_autoround_entry_points():
    """include/woq_hip.h, _lib.EXPORTS, qbits.__all__ and INTEGRATION.md name the three entry points; the ABI version
    stays 4"""
    import ctypes

    from intel_extension_for_transformers_amd import _lib, qbits

    header = open(os.path.join(ROOT, "include", "woq_hip.h")).read()
    declared = set(re.findall(r"WOQ_API[^;(]*?\b(woq_\w+)\s*\(", header))
    new = {"woq_autoround_forward", "woq_autoround_step", "woq_autoround_codes"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    assert declared == set(_lib.EXPORTS)
    assert "#define WOQ_ABI_VERSION 4" in header
    assert {"autoround_forward", "autoround_step", "autoround_codes"} <= set(qbits.__all__)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integration for n in new)
    makefile = open(os.path.join(ROOT, "intel_extension_for_transformers_amd", "csrc", "Makefile")).read()
    assert "woq_autoround.hip" in makefile
    if os.path.exists(_lib.LIB_PATH):
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for n in new:
            getattr(lib, n)
