"""No-GPU checks around the native sampler (csrc/woq_sample.hip): the numpy Philox restatement the GPU tests compare the
device words with reproduces Random123's known answers; the float64 reference sampler keeps exactly what
`DeviceSampler.processed` (pinned against Hugging Face's classes in tests/test_api_cpu.py) keeps; the C ABI and the ctypes
binding carry the new entry points."""
import os
import re

import numpy as np
import torch

from tests import sampler_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_known_answers():
    """Random123 kat_vectors, philox4x32 with 10 rounds."""
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
              "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in cases:
        assert " ".join("%08x" % w for w in R.philox4x32_10(ctr, key)) == want
    u = R.uniform_at(0, 0)
    assert u == (0x6627E8D5 >> 8) * 2.0 ** -24 and 0.0 <= u < 1.0 and float(np.float32(u)) == u


def test_reference_keeps_what_device_sampler_keeps():
    """Random logits, seen sets over negative and positive logits, -inf entries and a planted tie at the k-th value: the
    reference's kept set == the finite entries of DeviceSampler.processed (same fp32 scores, so no tolerance). Cases
    whose nucleus boundary lies within 1e-4 of 1 - top_p are not asked (fp32 softmax + cumsum vs float64); the seeds
    below have none."""
    from intel_extension_for_transformers_amd.runtime.engine import DeviceSampler

    rng = np.random.default_rng(7)
    for vocab, kw in [(1000, dict(temperature=0.1, top_k=40, top_p=0.75, repetition_penalty=1.1)),
                      (3001, dict(temperature=0.9, top_k=8, top_p=0.95, repetition_penalty=1.1)),
                      (3001, dict(temperature=0.7, top_k=1, top_p=1.0, repetition_penalty=1.3)),
                      (5000, dict(temperature=1.3, top_k=1024, top_p=0.9, repetition_penalty=1.0)),
                      (777, dict(temperature=2.0, top_k=50, top_p=0.5, repetition_penalty=1.2))]:
        for trial in range(4):
            logits = (4 * rng.standard_normal(vocab)).astype(np.float32)
            if trial & 1:
                logits[rng.choice(vocab, vocab // 10, replace=False)] = -np.inf
            hist = rng.choice(vocab, 60, replace=False)
            if trial & 2:  # a 3-way tie at the k-th value among unseen ids
                k = kw["top_k"]
                free = np.setdiff1d(np.argsort(-logits, kind="stable")[:k + 40], hist, assume_unique=False)
                order = free[np.argsort(-logits[free], kind="stable")]
                logits[order[k:k + 2]] = logits[order[k - 1]]
            s = R.scores_f32(logits, hist, kw["repetition_penalty"], kw["temperature"], True)
            ref = R.choose(s, kw["top_k"], kw["top_p"], max_candidates=1 << 30)
            assert ref.boundary_margin > 1e-4, (vocab, kw, trial, ref.boundary_margin)
            got = DeviceSampler(do_sample=True, **kw).processed(torch.from_numpy(logits), torch.from_numpy(hist))
            kept = torch.nonzero(torch.isfinite(got)).reshape(-1).numpy()
            # the nucleus may cut through a group of tied scores: which of the tied ids stay then depends on the sort's
            # tie order (torch.sort: unspecified; the native sampler and this reference: id ascending) — the kept
            # VALUES are the same either way, the ids are compared when the cut does not split a tie
            assert np.array_equal(np.sort(s[kept]), np.sort(s[ref.ids])), (vocab, kw, trial)
            full = R.choose(s, kw["top_k"], 1.0, max_candidates=1 << 30)
            split = ref.n_kept < full.n_kept and s[full.ids[ref.n_kept]] == s[ref.ids[-1]]
            if not split:
                assert set(kept.tolist()) == set(int(i) for i in ref.ids), (vocab, kw, trial)
                # the penalised, scaled scores themselves are the same fp32 values on the kept ids
                assert np.array_equal(got.numpy()[ref.ids], s[ref.ids])
    # penalty-only: the argmax of the same fp32 scores
    logits = (4 * rng.standard_normal(2000)).astype(np.float32)
    hist = np.argsort(-logits)[:5]
    s = R.scores_f32(logits, hist, 1.3, 1.0, False)
    got = DeviceSampler(do_sample=False, repetition_penalty=1.3).processed(torch.from_numpy(logits), torch.from_numpy(hist))
    assert np.array_equal(got.numpy(), s) and int(got.argmax()) == int(np.argmax(s))


def test_abi_and_binding_carry_the_sampler_entry_points():
    """include/woq_hip.h, _lib.EXPORTS and the experimental pair name the sampler's entry points; the ctypes struct has
    the header's layout (eight 4-byte fields)."""
    import ctypes

    from intel_extension_for_transformers_amd import _lib

    header = open(os.path.join(ROOT, "include", "woq_hip.h")).read()
    declared = set(re.findall(r"WOQ_API[^;(]*?\b(woq_\w+)\s*\(", header))
    new = {"woq_engine_set_sampler", "woq_engine_sampler_seen", "woq_engine_sampler_seen_ptr"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    exp = open(os.path.join(ROOT, "include", "woq_hip_experimental.h")).read()
    assert re.search(r"WOQ_API int woq_probe_sample\(", exp) and "woq_probe_sample" in _lib.EXPERIMENTAL_EXPORTS
    assert re.search(r"WOQ_API int woq_probe_gemv_f32\(", exp) and "woq_probe_gemv_f32" in _lib.EXPERIMENTAL_EXPORTS
    assert re.search(r"WOQ_API int woq_probe_gemm_plan\(", exp) and "woq_probe_gemm_plan" in _lib.EXPERIMENTAL_EXPORTS
    assert re.search(r"WOQ_API int woq_probe_gemm_f16\(", exp) and "woq_probe_gemm_f16" in _lib.EXPERIMENTAL_EXPORTS
    for n in ("woq_probe_attn_decode_plan", "woq_engine_attn_plan"):
        assert re.search(r"WOQ_API int %s\(" % n, exp) and n in _lib.EXPERIMENTAL_EXPORTS
    assert "#define WOQ_ABI_VERSION 4" in header and "struct woq_sampler_config" in header
    assert ctypes.sizeof(_lib.SamplerConfig) == 32
    cfg = _lib.sampler_config(True, 0.1, 40, 0.75, 1.1, seed=(7 << 32) | 9)
    assert (cfg.do_sample, cfg.top_k, cfg.seed_lo, cfg.seed_hi) == (1, 40, 9, 7)
    assert abs(cfg.temperature - 0.1) < 1e-7 and abs(cfg.repetition_penalty - 1.1) < 1e-6
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integration for n in new)
    if os.path.exists(_lib.LIB_PATH):
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for n in new | {"woq_probe_sample", "woq_probe_gemv_f32", "woq_probe_gemm_plan", "woq_probe_gemm_f16",
                        "woq_probe_attn_decode_plan", "woq_engine_attn_plan"}:
            getattr(lib, n)
