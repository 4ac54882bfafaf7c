"""The refusals of `woq_moe_forward`, `woq_moe_prompt_forward` and `woq_moe_backward` (csrc/woq_moe.hip,
woq_moe_prompt.hip, woq_moe_bwd.hip) and the three workspace sizes, through ctypes on the built library, with no device.

Every refusal case is a call with exactly one defect and pins the return code and the exact `woq_last_error()` text.
Pointers are plain integers of the right alignment and headers are filled on the host as include/woq_blob.h
woq_header_init / woq_fp8_headers fill them. No case may reach a launch: every case but the workspace-size one also passes
`workspace_bytes = 0`, so a check that went missing is caught by the last check instead of launching kernels on made-up
addresses, and the whole file is skipped where a device is present.
"""
import ctypes
import os

import pytest
import torch

from intel_extension_for_transformers_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available() or not os.path.exists(_lib.LIB_PATH),
                                reason="made-up device addresses: runs only where no kernel can launch, on a built library")

H, I, E, TOPK, T = 128, 96, 8, 3, 5
FORWARD, PROMPT, BACKWARD = "woq_moe_forward", "woq_moe_prompt_forward", "woq_moe_backward"
SLOT_LIMIT = {FORWARD: 8192, PROMPT: 65536, BACKWARD: 65536}
WORKSPACE_FN = {FORWARD: "woq_moe_workspace", PROMPT: "woq_moe_prompt_workspace", BACKWARD: "woq_moe_backward_workspace"}


def _round_up(x, m):
    return (x + m - 1) // m * m


def _header(K, N, group=128, weight_type=_lib.W_INT4_CLIP, scale_type=_lib.F16, asym=False):
    """include/woq_blob.h woq_header_init, no act-order"""
    h = _lib.BlobHeader()
    group = K if group <= 0 or group > K else group
    h.magic, h.version, h.K, h.N, h.group = 0x31485157, 2, K, N, group
    h.Kpad, h.Npad, h.n_groups = _round_up(K, 128), _round_up(N, 16), (K + group - 1) // group
    h.weight_type, h.scale_type, h.flags = weight_type, scale_type, 1 if asym else 0
    h.scale_mode = 0 if h.n_groups == 1 or group % 128 == 0 else 1
    tiles_n, tiles_k = h.Npad // 16, h.Kpad // 128
    n_scale = tiles_n * h.n_groups * 16 if h.scale_mode == 0 else tiles_n * tiles_k * 64
    h.off_q = 256
    h.off_scale = h.off_q + tiles_n * tiles_k * 1024
    off = _round_up(h.off_scale + n_scale * (4 if scale_type == _lib.F32 else 2), 256)
    if asym:
        h.off_zp, off = off, _round_up(off + n_scale, 256)
    h.total_bytes = off
    return h


def _fp8_header(K, N):
    """include/woq_blob.h woq_fp8_headers: the outer header of [HI int4 blob][LO int4 blob, with zero points]"""
    hi, lo = _header(K, N), _header(K, N, asym=True)
    hi.weight_type, hi.off_q, hi.off_scale = _lib.W_FP8_E4M3, 256, 256 + hi.total_bytes
    hi.total_bytes = 256 + hi.total_bytes + lo.total_bytes
    return hi


def _base(fn, hidden=H, inter=I):
    gu, dn = _header(hidden, 2 * inter), _header(inter, hidden)
    a = dict(x=0x10000, x_dtype=_lib.F32, ldx=hidden, idx=0x20000, idx64=1, w=0x30000, T=T, top_k=TOPK, E=E,
             gu=0x400000, gu_hdr=gu, gu_stride=gu.total_bytes, dn=0x800000, dn_hdr=dn, dn_stride=dn.total_bytes,
             out=0x50000, out_dtype=_lib.F32, ldo=hidden, ws=0x1000000, ws_bytes=0)
    if fn == BACKWARD:
        a.update(grad=0x60000, grad_dtype=_lib.F32, ldg=hidden, grad_w=0x70000)
    return a


def _call(fn, a):
    L = _lib.lib()
    hp = lambda h: None if h is None else ctypes.byref(h)
    if fn == BACKWARD:
        rc = L.woq_moe_backward(a["grad"], a["grad_dtype"], a["ldg"], a["x"], a["x_dtype"], a["ldx"], a["idx"], a["idx64"],
                                a["w"], a["T"], a["top_k"], a["E"], a["gu"], hp(a["gu_hdr"]), a["gu_stride"], a["dn"],
                                hp(a["dn_hdr"]), a["dn_stride"], a["out"], a["out_dtype"], a["ldo"], a["grad_w"], a["ws"],
                                a["ws_bytes"], None)
    else:
        rc = getattr(L, fn)(a["x"], a["x_dtype"], a["ldx"], a["idx"], a["idx64"], a["w"], a["T"], a["top_k"], a["E"], a["gu"],
                            hp(a["gu_hdr"]), a["gu_stride"], a["dn"], hp(a["dn_hdr"]), a["dn_stride"], a["out"],
                            a["out_dtype"], a["ldo"], a["ws"], a["ws_bytes"], None)
    return rc, L.woq_last_error().decode()


def _need(fn, a, hidden=H, inter=I):
    return getattr(_lib.lib(), WORKSPACE_FN[fn])(a["T"], a["top_k"], a["E"], hidden, inter)


def _set(field, value):
    return lambda a: a.__setitem__(field, value)


def _hdr_set(which, field, value):
    return lambda a: setattr(a[which], field, value)


def _shape(hidden, inter):  # the sound call of another (hidden, inter)
    return lambda a: a.update(_base(BACKWARD if "grad" in a else FORWARD, hidden, inter))


def _gate_up_n(a):  # gate/up blobs of another inter than the down blobs'
    a["gu_hdr"] = _header(H, 2 * I + 32)
    a["gu_stride"] = a["gu_hdr"].total_bytes


# name -> (mutation of the base call, the text, with {fn} the entry point's name)
SHARED = {
    "null_header": (_set("gu_hdr", None), "QBits: {fn}: null header"),
    "null_down_header": (_set("dn_hdr", None), "QBits: {fn}: null header"),
    "weight_type": (_hdr_set("gu_hdr", "weight_type", _lib.W_INT3_CLIP),
                    "QBits: woq_moe_forward takes int4 / int3 / int2, nf4 / fp4, int8 and fp8 expert blobs"),
    "act_order": (_hdr_set("dn_hdr", "off_shuffle", 4096), "QBits: woq_moe_forward: act-order expert blobs are not built"),
    "stride_small": (lambda a: a.__setitem__("gu_stride", a["gu_stride"] - 16),
                     "QBits: woq_moe_forward: the expert stride is smaller than a blob or no multiple of 16"),
    "stride_odd": (lambda a: a.__setitem__("dn_stride", a["dn_stride"] + 8),
                   "QBits: woq_moe_forward: the expert stride is smaller than a blob or no multiple of 16"),
    "kn_relation": (_gate_up_n, "QBits: {fn}: gate/up blobs must be [K = hidden, N = 2 * inter] against down blobs "
                                "[K = inter, N = hidden]"),
    "hidden_mod_4": (_shape(126, I), "QBits: {fn}: the hidden size must be a multiple of 4"),
    "x_dtype": (_set("x_dtype", 7), "QBits: unsupported qbits data type."),
    "out_dtype": (_set("out_dtype", 3), "QBits: unsupported qbits data type."),
    "experts": (_set("E", 1025), "QBits: {fn} takes at most 1024 experts and {slots} routed slots (T * top_k) per call"),
    "null_x": (_set("x", 0), "QBits: {fn}: null tensor"),
    "null_topk_w": (_set("w", 0), "QBits: {fn}: null tensor"),
    "null_workspace": (_set("ws", 0), "QBits: {fn}: null tensor"),
    "ldx": (_set("ldx", H - 4), "QBits: {fn}: leading dimension smaller than hidden"),
    "ldo": (_set("ldo", H - 4), "QBits: {fn}: leading dimension smaller than hidden"),
    "x_misaligned": (_set("x", 0x10004), "QBits: {fn}: activation rows must be aligned to four elements"),
    "ldx_misaligned": (_set("ldx", H + 2), "QBits: {fn}: activation rows must be aligned to four elements"),
}
INTER_MOD_16 = {FORWARD: "QBits: woq_moe_forward: the intermediate size must be a multiple of 16 (gate tile tn pairs with up "
                         "tile tn + inter / 16)",
                PROMPT: "QBits: woq_moe_prompt_forward: the intermediate size must be a multiple of 16 (gate tile tn pairs "
                        "with up tile tn + inter / 16)",
                BACKWARD: ("QBits: woq_moe_backward: the intermediate size must be a multiple of 16",
                           "QBits: woq_moe_backward: the intermediate size must be a multiple of 16 (gate tile tn pairs "
                           "with up tile tn + inter / 16)")}  # either wording: the forward's parenthetical may be shared
BLOB_ALIGNED = {FORWARD: "QBits: woq_moe_forward: blobs and workspace must be 16-byte aligned",
                PROMPT: "QBits: woq_moe_prompt_forward: blobs and workspace must be 16-byte aligned",
                BACKWARD: "QBits: woq_moe_backward: blobs must be 16-byte and the workspace 256-byte aligned"}
CASES = [(fn, name) for fn in (FORWARD, PROMPT, BACKWARD) for name in
         list(SHARED) + ["inter_mod_16", "slots", "blob_misaligned", "workspace_misaligned", "workspace_short"]]
CASES += [(BACKWARD, n) for n in ("fp8_blobs", "rows_65536", "grad_dtype", "null_grad", "ldg", "workspace_16_aligned")]


def _case(fn, name):
    """-> (the call's arguments, the accepted texts)"""
    a = _base(fn)
    if name in SHARED:
        mutate, text = SHARED[name]
        mutate(a)
    elif name == "inter_mod_16":
        _shape(H, 88)(a)
        text = INTER_MOD_16[fn]
    elif name == "slots":
        a["T"] = SLOT_LIMIT[fn] // TOPK + 1
        text = SHARED["experts"][1]
    elif name == "blob_misaligned":
        a["gu"] += 8
        text = BLOB_ALIGNED[fn]
    elif name == "workspace_misaligned":
        a["ws"] += 8
        text = BLOB_ALIGNED[fn]
    elif name == "workspace_short":
        need = _need(fn, a)
        a["ws_bytes"] = need - 1
        text = "QBits: {fn}: the workspace holds %d bytes, this call needs %d (%s)" % (need - 1, need, WORKSPACE_FN[fn])
    elif name == "fp8_blobs":
        a["dn_hdr"] = _fp8_header(I, H)
        a["dn_stride"] = a["dn_hdr"].total_bytes
        text = "QBits: woq_moe_backward: fp8 expert blobs are not built; they take the dequantise-and-matmul arm"
    elif name == "rows_65536":
        a["T"], a["top_k"] = 65536, 1
        text = SHARED["experts"][1]
    elif name == "grad_dtype":
        a["grad_dtype"] = 7
        text = "QBits: unsupported qbits data type."
    elif name == "null_grad":
        a["grad"] = 0
        text = "QBits: {fn}: null tensor"
    elif name == "ldg":
        a["ldg"] = H - 4
        text = "QBits: {fn}: leading dimension smaller than hidden"
    elif name == "workspace_16_aligned":
        a["ws"] += 16
        text = BLOB_ALIGNED[fn]
    texts = text if isinstance(text, tuple) else (text,)
    return a, [t.format(fn=fn, slots=SLOT_LIMIT[fn]) for t in texts]


@pytest.mark.parametrize("fn,name", CASES)
def test_single_defect_is_refused_with_its_text(fn, name):
    a, texts = _case(fn, name)
    assert name == "workspace_short" or a["ws_bytes"] == 0
    rc, msg = _call(fn, a)
    assert rc == 1 and msg in texts, (fn, name, rc, msg)


@pytest.mark.parametrize("fn", [FORWARD, PROMPT, BACKWARD])
def test_sound_call_reaches_the_workspace_check_and_no_rows_return_zero(fn):
    a = _base(fn)
    rc, msg = _call(fn, a)
    need = _need(fn, a)
    assert need > 0 and rc == 1
    assert msg == "QBits: %s: the workspace holds 0 bytes, this call needs %d (%s)" % (fn, need, WORKSPACE_FN[fn])
    for t in (0, -3):  # no rows: 0 before the pointer checks
        a = _base(fn)
        a.update(T=t, x=0, ws=0)
        assert _call(fn, a)[0] == 0
    a = _base(fn)  # ... and after the header and dtype checks
    a.update(T=0, x_dtype=7)
    assert _call(fn, a) == (1, "QBits: unsupported qbits data type.")


# (T, top_k, E, hidden, inter) -> woq_moe_workspace, woq_moe_prompt_workspace, woq_moe_backward_workspace
WORKSPACES = {
    (1, 2, 8, 4096, 14336): (148480, 148736, 8899584),
    (5, 3, 8, 128, 96): (14592, 14848, 119680),
    (37, 2, 4, 256, 160): (124672, 124928, 454656),
    (300, 8, 128, 2048, 768): (27057920, 27057408, 59944448),
}


@pytest.mark.parametrize("shape", list(WORKSPACES))
def test_workspace_sizes(shape):
    L = _lib.lib()
    got = tuple(getattr(L, WORKSPACE_FN[fn])(*shape) for fn in (FORWARD, PROMPT, BACKWARD))
    assert got == WORKSPACES[shape], (shape, got)


def test_workspace_of_a_shape_over_a_limit_is_zero():
    L = _lib.lib()
    for fn in (FORWARD, PROMPT, BACKWARD):
        ws = getattr(L, WORKSPACE_FN[fn])
        assert ws(SLOT_LIMIT[fn] // 2, 2, 8, 128, 96) > 0
        assert ws(SLOT_LIMIT[fn] // 2 + 1, 2, 8, 128, 96) == 0
        assert ws(4, 2, 1025, 128, 96) == 0 and ws(4, 2, 1024, 128, 96) > 0
        for bad in ((0, 2, 8, 128, 96), (4, 0, 8, 128, 96), (4, 2, 0, 128, 96), (4, 2, 8, 0, 96), (4, 2, 8, 128, 0)):
            assert ws(*bad) == 0
    assert L.woq_moe_backward_workspace(65536, 1, 8, 128, 96) == 0 and L.woq_moe_backward_workspace(65535, 1, 8, 128, 96) > 0
