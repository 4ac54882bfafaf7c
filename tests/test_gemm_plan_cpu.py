"""The prompt pass's GEMM plan (csrc/woq_gemm_f16.hip plan_gemm_f16) on the host, through woq_probe_gemm_plan: which
kernel form a call gets, that the pack pass's layout follows from the same decision, and that the workspace the
caller-side sizing function answers always holds the call. No device is touched. The expected forms are the tables the
GPU tests assert against the form log (tests/test_gpu_prefill_gemm_forms.py), imported, not restated."""
import os

import pytest

from intel_extension_for_transformers_amd import _lib as L
from tests.test_gpu_prefill_gemm_forms import (CHILD_CASES, DISPATCH, F_RING, F_RING_RAW, F_TALL, HS, RAW, RING, TALL,
                                               TALL_CASES)

pytestmark = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libwoq_hip.so not built (python __graft_entry__.py)")

DT = {"fp32": L.F32, "bf16": L.BF16, "fp16": L.F16}
CT = {"fp32": L.C_FP32, "bf16": L.C_BF16}


def _plan(M, N, K, quant, act, compute="bf16", lda=None, **kw):
    """the plan of a woq_linear call over `quant` = (group, asym, scale type) int4, or "nf4" as _nf4_blob packs it
    (group 128, fp32 scales); rows of `act` with stride K unless `lda` says otherwise"""
    wtype = L.W_INT4_CLIP
    if quant == "nf4":
        wtype, quant = L.W_NF4, (128, False, "fp32")
    group, asym, st = quant
    return L.probe_gemm_plan(K, N, group, wtype, DT[st], CT[compute], asym, False, M, DT[act],
                             K if lda is None else lda, **kw)


def _cases():
    """(what, expected form, plan arguments) of every call the GPU tests pin to a form, plus the switch and raw-A
    boundary variants"""
    out = []
    for what, M, N, K, quant, act, compute, form in DISPATCH:
        out.append((what, form, dict(M=M, N=N, K=K, quant=quant, act=act, compute=compute)))
    for M, N, K, quant, act, _ in TALL_CASES:
        form = F_RING if (M, N) == (2560, 12288) else F_TALL  # test_tall_gemm_ragged_rows_vs_oracle
        out.append(("tall M=%d N=%d K=%d %s %s" % (M, N, K, quant, act), form, dict(M=M, N=N, K=K, quant=quant, act=act)))
    for M, N, quant, act, wbits, form in CHILD_CASES:
        if wbits != 4:
            continue
        args = dict(M=M, N=N, K=512, quant=quant, act=act)
        out.append(("child M=%d N=%d %s %s, tall_raw" % (M, N, quant, act), form, dict(args, tall_raw=True)))
        out.append(("child M=%d N=%d %s %s" % (M, N, quant, act), form & ~TALL if form & RAW else form, args))
    # test_engine_prompt_pass_on_tall_gemm_vs_oracle: Llama-2-7B geometry, 2829 rows, fp16 scales; qkv and gate/up read
    # fp32 rows through RMSNorm, o and down take the fp16 rows of the attention / the SiLU * mul epilogue
    engine = [("qkv", 12288, 4096, "fp32", True), ("o", 4096, 4096, "fp16", False),
              ("gate/up", 22016, 4096, "fp32", True), ("down", 4096, 11008, "fp16", False)]
    for group, asym in [(128, False), (32, True)]:
        for (name, N, K, act, norm), form in zip(engine, [F_TALL, F_RING_RAW, F_TALL, F_RING_RAW]):
            out.append(("engine %s g%d" % (name, group), form,
                        dict(M=2829, N=N, K=K, quant=(group, asym, "fp16"), act=act, has_norm=norm)))
    seam = next(d for d in DISPATCH if d[0] == "seam 2561: tall")
    out.append(("WOQ_GEMM_TALL=0 on a tall row", F_RING,
                dict(M=seam[1], N=seam[2], K=seam[3], quant=seam[4], act=seam[5], compute=seam[6], tall=False)))
    raw = next(d for d in DISPATCH if d[0] == "ring, raw A")
    assert raw[7] == F_RING_RAW
    args = dict(M=raw[1], N=raw[2], K=raw[3], quant=raw[4], act=raw[5], compute=raw[6])
    out.append(("raw A, pointer not 16-byte aligned: packed", F_RING, dict(args, aligned=False)))
    out.append(("raw A, lda % 8 != 0: packed", F_RING, dict(args, lda=raw[3] + 4)))
    return out


CASES = _cases()


@pytest.mark.parametrize("what,form,args", CASES, ids=[c[0] for c in CASES])
def test_plan_form_and_pack_layout(what, form, args):
    """the dispatch map, and for every case the coupling the kernels rely on: half-tile images exactly for the ring
    kernels, no row blocks in the pack pass exactly for raw-A, raw / ring only on the hand-scheduled loop, 256-row
    tiles only over the ring layout"""
    p = _plan(**args)
    assert p["form"] == form, (what, p)
    f = p["form"]
    assert p["half_tiles"] == (1 if f & RING else 0), (what, p)
    assert p["row_blocks"] == (0 if f & RAW else -(-args["M"] // 128) * 128), (what, p)
    assert not f & (RAW | RING) or f & HS, (what, p)
    assert not f & TALL or f & RING, (what, p)


def test_workspace_sizing_holds_every_call():
    """over row counts around the split-K and tile seams and the projection shapes of 7B / 70B models (and one small
    odd-tile K): the call's workspace never exceeds what gemm_f16_workspace_bytes_blob answers for it, split-K
    partials stay inside the share the sizing reserves for them (nz * workgroups <= 512 -> at most 32 of the 40 MiB),
    and a split has at least two slices"""
    n = 0
    for M in (17, 64, 100, 128, 129, 200, 256, 2049):
        for K, N in ((4096, 4096), (4096, 12288), (4096, 22016), (11008, 4096), (8192, 57344), (640, 1024)):
            for kind in ("int4", "nf4", "fp8"):
                for compute in ("bf16", "fp32"):  # planes 1 | 2
                    quant = "nf4" if kind == "nf4" else (128, False, "fp16")
                    p = _plan(M, N, K, quant, "fp32", compute, fp8=kind == "fp8")
                    what = (M, K, N, kind, compute, p)
                    assert p["ws_total"] <= p["ws_sized"], what
                    assert p["part_bytes"] <= p["splitk_ws"] == 40 << 20, what
                    assert p["part_bytes"] <= 32 << 20, what
                    split = bool(p["form"] & L.GEMM_FORM_SPLITK)
                    assert p["nz"] >= 2 if split else p["nz"] == 1, what
                    assert (p["part_bytes"] > 0) == split, what
                    assert bool(p["form"] & L.GEMM_FORM_FRAG) == (kind != "int4"), what
                    n += split
    assert n > 0  # the sweep reaches split-K calls
