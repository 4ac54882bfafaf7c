"""Reference for the prompt pass's MFMA GEMM with its fused RMSNorm and epilogues (csrc/woq_gemm_f16.hip: pack_row's
norm branch, gemm_epilogue, splitk_reduce_kernel; csrc/woq_gemm_f16p.h / woq_gemm_f16t.h behind the same epilogue), as
`woq_probe_gemm_f16` runs it: numpy, float64. Shared by tests/test_gemm_f16_reference_cpu.py (no GPU: the forms the case
list claims, what the band would catch) and tests/test_gpu_prefill_gemm_epilogues.py.

The operation, per activation row (x taken exactly as the kernel receives it, after its own dtype rounding): with
y_k = x_k g_k (g = the RMSNorm weight, 1 without a norm) taken at k' = shuffle[k] under act-order,
inv = rsqrt(mean_K(x^2) + eps) (1 without a norm; the mean is over K, not Kpad),
    lin_n = inv * sum_k y_k' W_deq[k, n] + bias_n,
for epi 1 SiLU(gate) * up over the interleaved 16-column tiles (gate tile, up tile, gate tile, ...; N / 2 outputs), then
+ residual, then for an fp16 output the clamp to +-65504, then the output type's rounding. W_deq is the oracle's
dequantisation of the blob (scales after their own dtype rounding).

Band (`reference(...)["tol"]`), every number the project's own:
  pre-epilogue value   A = 2e-3 * rowmax|inv * y . W_deq| + 1e-5, the one-product bound of this GEMM
                       (test_gpu_parity.py test_woq_linear_prefill_f16_operand_variants, test_gpu_prefill_gemm_forms.py);
                       1e-4 * rowmax + 1e-5 for the fp32-class form (test_woq_linear_prefill_gemm_vs_oracle). The row
                       maximum is over all N weight columns (gate and up tiles alike), without the bias.
  epi 1                A through SiLU * mul in float64, the formula of tests/gemv_f32_reference.py:
                       (|SiLU'(g)| + A / 2) A |u| + |SiLU(g)| A + A A   (SiLU'' <= 1 / 2)
  residual             one fp32 rounding of the sum, 2^-24 |sum|
  output type          bf16 2^-8 |ref|, fp16 2^-10 |ref| (ref after the clamp)
The comparison target is `exp`, the value before the output type's rounding. Nothing here is taken from a kernel's output.

Forms: `expect` of a case = (GEMM_FORM_* bits, K slices, half-tile images, rows of the pack pass) as
`woq_probe_gemm_plan` reports them, and `pack` = (MODE, chunks cached per thread) of the pack pass, which pack_f16_kernel
picks on the device: `pack_mode` restates that choice (MODE 0 fp32 rows, 1 16-bit rows, 2 gathered / unaligned rows;
2 / 4 / 8 register-cached chunks of 8 values per thread, 0 = two sweeps; None = raw-A rows, no pack pass over them).
`kper` restates the plan's tiles per K slice for the dropped-slice corruption; the CPU file checks it against the plan's
slice count.

Inputs (`build`): weights from tests/gemv_f32_reference.py `_weight` (seed 0, RTN-quantised by the oracle from
0.05 N(0, 1), gate / up fused by `fuse_gate_up`); rows N(0, 1) at distinct scales with, from M = 4 on, row 0 all zero,
row 1 at 1e-4 (eps dominates the mean; with a norm only), row 2 with one element times 30, row 3 times 2^12 (2^4 without
a norm, where nothing takes the factor out again); with a second row block, its first row has the times-30 element too.
Norm weights 1 + 0.1 N(0, 1), bias N(0, 1), residual 4 N(0, 1). The fp16 term of the band is relative, so it does not
cover a result below fp16's normal range (2^-14) whose bound A is smaller than the subnormal step 2^-24: a 1e-4 row
without a norm behind SiLU * mul gives products of 1e-8, which no fp16 store can represent. The inputs keep away from
that, and the CPU file checks for every case that the correctly rounded reference lies inside the band. For bf16 the
term 2^-8 |ref| IS the format's largest half step, so a bf16 case whose bound A is small (the all-zero row: the bias
alone) reaches 0.9 of the band by rounding alone; the GPU file prints that share beside every ratio.
"""
import functools

import numpy as np

from oracle import woq_oracle as orc
from tests import gemv_f32_reference as G
from tests.gemv_f32_reference import _silu, _silu_d, inv_rows

F32 = np.float32
EPS = 1e-5
REL, REL_FP32, ABS = 2e-3, 1e-4, 1e-5
OUT_EPS = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -10}
F16_MAX = 65504.0
REFUSAL = "QBits: the SiLU*mul epilogue needs whole gate / up column-tile pairs"

FRAG, SPLITK, FP32C, HS, RING, TALL, RAW = 1, 2, 4, 8, 16, 32, 64  # _lib.GEMM_FORM_*
G128, G32A, G128B = (128, False, "fp16"), (32, True, "fp32"), (128, True, "bf16")


def round_act(x, act):
    """fp32 values -> what the kernel receives as `act` rows, as fp32"""
    x = np.asarray(x, F32)
    if act == "bf16":
        return orc.bf16_round(x)
    return x.astype(np.float16).astype(F32) if act == "fp16" else x


# ---- the operation ---------------------------------------------------------------------------------------------------
def activation(x, g=None, shuffle=None):
    """-> y [M, K] float64: x g gathered at shuffle[k]"""
    y = np.asarray(x, F32).astype(np.float64)
    if g is not None:
        y = y * np.asarray(g, F32).astype(np.float64)
    return y if shuffle is None else y[:, shuffle]


def pre_band(pre, fp32_class=False):
    """the bound of the pre-epilogue value inv * y . W_deq: [M, 1]"""
    return (REL_FP32 if fp32_class else REL) * np.abs(pre).max(axis=1, keepdims=True) + ABS


def epilogue(pre, A, bias=None, residual=None, epi=0, out="fp32", clamp=True):
    """pre [M, N] float64 and its bound A (broadcastable) -> dict(exp, tol, unclamped [M, n_out])"""
    if epi == 1 and (pre.shape[1] % 32 != 0 or (-(-pre.shape[1] // 16)) % 2 != 0):
        raise RuntimeError(REFUSAL)
    lin = pre if bias is None else pre + np.asarray(bias, F32).astype(np.float64)
    a = np.broadcast_to(A, lin.shape)
    if epi == 1:
        v, a = lin.reshape(len(lin), -1, 2, 16), a.reshape(len(lin), -1, 2, 16)
        gate, up, ag, au = v[:, :, 0], v[:, :, 1], a[:, :, 0], a[:, :, 1]
        lin = (_silu(gate) * up).reshape(len(pre), -1)
        a = ((np.abs(_silu_d(gate)) + 0.5 * ag) * ag * np.abs(up) + np.abs(_silu(gate)) * au + ag * au).reshape(len(pre), -1)
    if residual is not None:
        lin = lin + np.asarray(residual, F32).astype(np.float64)
        a = a + 2.0 ** -24 * np.abs(lin)
    exp = np.clip(lin, -F16_MAX, F16_MAX) if (out == "fp16" and clamp) else lin
    return dict(exp=exp, tol=a + OUT_EPS[out] * np.abs(exp), unclamped=lin)


def reference(x, W64, shuffle=None, g=None, eps=EPS, bias=None, residual=None, epi=0, out="fp32", fp32_class=False,
              K_mean=None, y=None, clamp=True):
    """x [M, K] as the kernel receives it -> dict(exp, tol, unclamped [M, n_out], pre [M, N], A [M, 1], inv [M]). K_mean,
    y and clamp are for the corruptions of the CPU file: the divisor of the mean, another gathered activation, no clamp."""
    if epi == 1 and (W64.shape[1] % 32 != 0 or (-(-W64.shape[1] // 16)) % 2 != 0):
        raise RuntimeError(REFUSAL)
    inv = inv_rows(x, g, eps, K_mean)
    y = activation(x, g, shuffle) if y is None else y
    pre = (y @ W64) * inv[:, None]
    A = pre_band(pre, fp32_class)
    r = epilogue(pre, A, bias, residual, epi, out, clamp)
    r.update(pre=pre, A=A, inv=inv)
    return r


def saturated(t):
    """elements of reference(...) an fp16 store must leave at exactly +-65504: beyond it by more than the bound"""
    return np.abs(t["unclamped"]) - (t["tol"] - OUT_EPS["fp16"] * np.abs(t["exp"])) > F16_MAX


def round_out(v, out):
    """float64 -> the output type's nearest value, as float64"""
    if out == "fp16":
        return np.asarray(v).astype(np.float16).astype(np.float64)
    return orc.bf16_round(np.asarray(v).astype(F32)).astype(np.float64) if out == "bf16" else np.asarray(v, np.float64)


# ---- forms -----------------------------------------------------------------------------------------------------------
def pack_mode(K, act, lda, shuffle, aligned=True, raw=False):
    """pack_f16_kernel's choice for the activation rows -> (MODE, cached chunks per thread), None for raw-A rows"""
    if raw:
        return None
    kpad = (K + 127) // 128 * 128
    esz = 4 if act == "fp32" else 2
    if shuffle or not aligned or (lda * esz) % 16 != 0 or K % 8 != 0:
        return (2, 0)
    per_thread = (kpad // 8 + 255) // 256
    return (0 if act == "fp32" else 1, next((n for n in (2, 4, 8) if per_thread <= n), 0))


def kper(M, N, K):
    """plan_gemm_f16's K tiles per slice for an int4 call (0 = no split)"""
    tiles_k, nb_m, nb_n = (K + 127) // 128, (M + 127) // 128, ((N + 15) // 16 * 16 + 127) // 128
    wgs = nb_m * nb_n
    if wgs > (256 if nb_m == 1 else 64) or tiles_k < 8:
        return 0
    want = min(16, max(2, 512 // wgs))
    per = max(4, ((tiles_k + want - 1) // want + 1) & ~1)
    return per if (tiles_k + per - 1) // per >= 2 else 0


# ---- the cases -------------------------------------------------------------------------------------------------------
def case(name, M, N, K, expect, pack, quant=G128, wname="int4_clip", act="fp32", out="fp16", norm=True, epi=0, bias=False,
         residual="none", shuffle=False, lda_pad=0, ldo_pad=2, ld_res_pad=0, out_off=0, fp32_class=False, rows="mixed",
         kind=""):
    """N = weight columns (epi 1: N / 2 outputs). residual: "none" | "alias" (the engine's: residual = out) | "separate"
    (row stride n_out + ld_res_pad). lda = K + lda_pad, ldo = n_out + ldo_pad, out_off = elements the output pointer sits
    behind the buffer's start. rows: "mixed" (module docstring) | "hot" (fp16 saturation). kind: the kernel behind the
    epilogue, for the summary of worst ratios."""
    return dict(name=name, M=M, N=N, K=K, expect=expect, pack=pack, quant=quant, wname=wname, act=act, out=out, norm=norm,
                epi=epi, bias=bias, residual=residual, shuffle=shuffle, lda_pad=lda_pad, ldo_pad=ldo_pad,
                ld_res_pad=ld_res_pad, out_off=out_off, fp32_class=fp32_class, rows=rows, kind=kind)


def _norm_cases():
    """the pack pass's norm branch: rows fp32 (MODE 0) / bf16 (MODE 1) x cached chunks 2 / 4 / 8 / two sweeps x epi 0 / 1;
    K != Kpad; MODE 2 by row stride and by act-order; M = 1, 40, 130"""
    out = []
    splits = {512: 1, 5120: 10, 11008: 15, 16512: 13}
    for act, mode in (("fp32", 0), ("bf16", 1)):
        for K, nc in ((512, 2), (5120, 4), (11008, 8), (16512, 0)):
            for epi in (0, 1):
                form = (HS | RING, 1, 1, 128) if K == 512 else (SPLITK, splits[K], 0, 128)
                out.append(case("norm %s K%d epi%d" % (act, K, epi), 40, 96, K, form, (mode, nc), act=act, epi=epi,
                                bias=True, kind="pack norm"))
    for epi in (0, 1):
        out.append(case("norm K480 (Kpad 512) epi%d" % epi, 40, 96, 480, (HS | RING, 1, 1, 128), (0, 2), epi=epi, bias=True,
                        kind="pack norm"))
        out.append(case("norm odd row stride epi%d" % epi, 40, 96, 512, (HS | RING, 1, 1, 128), (2, 0), epi=epi, bias=True,
                        lda_pad=1, kind="pack norm"))
        out.append(case("norm act-order epi%d" % epi, 40, 96, 512, (HS | RING, 1, 1, 128), (2, 0), epi=epi, bias=True,
                        shuffle=True, kind="pack norm"))
    out += [
        case("norm odd row stride K5120", 40, 96, 5120, (SPLITK, 10, 0, 128), (2, 0), bias=True, lda_pad=1, kind="pack norm"),
        case("norm act-order bf16 K5120 epi1", 40, 96, 5120, (SPLITK, 10, 0, 128), (2, 0), act="bf16", epi=1, shuffle=True,
             kind="pack norm"),
        case("norm M1 K512", 1, 96, 512, (HS | RING, 1, 1, 128), (0, 2), bias=True, kind="pack norm"),
        case("norm M1 K5120 epi1", 1, 96, 5120, (SPLITK, 10, 0, 128), (0, 4), epi=1, kind="pack norm"),
        case("norm M130 K512 epi1", 130, 96, 512, (HS | RING, 1, 1, 256), (0, 2), epi=1, bias=True, kind="pack norm"),
        case("norm M130 K512", 130, 96, 512, (HS | RING, 1, 1, 256), (0, 2), bias=True, kind="pack norm"),
        case("norm M130 K5120", 130, 96, 5120, (SPLITK, 10, 0, 256), (0, 4), bias=True, kind="pack norm"),
    ]
    return out


def _form_cases():
    """every kernel behind the shared epilogue x {norm + epi 0 -> fp16, norm + epi 1 -> fp16, fp16 rows + in-place
    residual -> fp32}. The raw-A form takes no norm: its first two are the same epilogues on raw fp16 rows."""
    out = []

    def three(what, K, form_norm, form_f16, pack_norm, pack_f16, kind, M=40, N=96, **kw):
        out.append(case(what + " norm epi0", M, N, K, form_norm, pack_norm, bias=True, kind=kind, **kw))
        out.append(case(what + " norm epi1", M, N, K, form_norm, pack_norm, epi=1, kind=kind, **kw))
        out.append(case(what + " f16 rows residual in place", M, N, K, form_f16, pack_f16, act="fp16", out="fp32",
                        norm=False, residual="alias", kind=kind, **kw))

    three("ring", 480, (HS | RING, 1, 1, 128), (HS | RING, 1, 1, 128), (0, 2), (1, 2), "ring")
    three("f16s K384", 384, (0, 1, 0, 128), (0, 1, 0, 128), (0, 2), (1, 2), "compiler-scheduled")
    three("two-tile g32a", 512, (HS, 1, 0, 128), (HS | RAW, 1, 0, 0), (0, 2), None, "hand-scheduled, no ring", quant=G32A)
    three("two-tile g32a K480", 480, (HS, 1, 0, 128), (HS, 1, 0, 128), (0, 2), (1, 2), "hand-scheduled, no ring", quant=G32A)
    raw = (HS | RING | RAW, 1, 1, 0)
    out += [
        case("raw-A epi0 bias", 40, 96, 512, raw, None, act="fp16", norm=False, bias=True, kind="raw-A"),
        case("raw-A epi1", 40, 96, 512, raw, None, act="fp16", norm=False, epi=1, kind="raw-A"),
        case("raw-A residual in place", 40, 96, 512, raw, None, act="fp16", out="fp32", norm=False, residual="alias",
             kind="raw-A"),
        case("raw-A M130 residual in place g128 asym bf16 scales", 130, 96, 512, (HS | RING | RAW, 1, 1, 0), None, quant=G128B,
             act="fp16", out="fp32", norm=False, residual="alias", kind="raw-A"),
    ]
    three("split-K K1024", 1024, (SPLITK, 2, 0, 128), (SPLITK, 2, 0, 128), (0, 2), (1, 2), "split-K")
    three("split-K K4096", 4096, (SPLITK, 8, 0, 128), (SPLITK, 8, 0, 128), (0, 2), (1, 2), "split-K")
    three("split-K M130 N256", 4096, (SPLITK, 8, 0, 256), (SPLITK, 8, 0, 256), (0, 2), (1, 2), "split-K", M=130, N=256)
    three("split-K g32a K1024", 1024, (SPLITK, 2, 0, 128), (SPLITK, 2, 0, 128), (0, 2), (1, 2), "split-K", quant=G32A)
    for wname, quant in (("nf4", (128, False, "fp32")), ("fp4_e2m1", (32, False, "fp16")), ("fp8_e4m3", (128, False, "fp16"))):
        three("frag " + wname, 512, (FRAG, 1, 0, 128), (FRAG, 1, 0, 128), (0, 2), (1, 2), "fragment image", wname=wname,
              quant=quant)
    out += [
        case("frag nf4 M130 K384 epi1", 130, 96, 384, (FRAG, 1, 0, 256), (0, 2), wname="nf4", quant=(128, False, "fp32"),
             epi=1, bias=True, kind="fragment image"),
        case("fp32-class norm", 40, 96, 512, (FP32C, 1, 0, 128), (0, 2), out="fp32", bias=True, fp32_class=True,
             kind="fp32-class"),
        case("fp32-class norm epi1 residual", 40, 96, 512, (FP32C, 1, 0, 128), (0, 2), out="fp32", epi=1, residual="separate",
             fp32_class=True, kind="fp32-class"),
    ]
    return out


def _edge_cases():
    """epilogue edges: gate/up pairing at N = 32 / 288 (the last column workgroup holds one tile pair), partly live last
    tiles (N = 40, 17), residual behind SiLU * mul, a residual stride of its own — on the direct and the split-K path"""
    ring, sk = (HS | RING, 1, 1, 128), (SPLITK, 2, 0, 128)
    out = []
    for what, K, form in (("direct", 512, ring), ("split-K", 1024, sk)):
        kind = "edges, " + what
        out += [
            case("%s epi1 N32" % what, 40, 32, K, form, (0, 2), epi=1, bias=True, kind=kind),
            case("%s epi1 N288 bias" % what, 40, 288, K, form, (0, 2), epi=1, bias=True, kind=kind),
            case("%s epi1 N288 bf16 out" % what, 40, 288, K, form, (0, 2), epi=1, out="bf16", kind=kind),
            case("%s epi1 residual separate" % what, 40, 96, K, form, (0, 2), epi=1, out="fp32", bias=True, residual="separate",
                 ld_res_pad=6, kind=kind),
            case("%s epi0 N40" % what, 40, 40, K, form, (0, 2), bias=True, kind=kind),
            case("%s epi0 N17 residual" % what, 40, 17, K, form, (0, 2), out="fp32", bias=True, residual="separate",
                 ld_res_pad=4, kind=kind),
            case("%s epi0 N40 bf16 rows bf16 out no norm" % what, 40, 40, K, form, (1, 2), act="bf16", out="bf16", norm=False,
                 kind=kind),
        ]
    return out


# the scalar store path of gemm_epilogue, forced each way on the same inputs as a paired-store call (`base`): the
# results must agree bit for bit
SCALAR_BASES = [
    case("pairs: norm epi1 fp16 out", 40, 96, 512, (HS | RING, 1, 1, 128), (0, 2), epi=1, bias=True, kind="scalar stores"),
    case("pairs: norm epi0 bf16 out", 130, 96, 512, (HS | RING, 1, 1, 256), (0, 2), out="bf16", bias=True,
         kind="scalar stores"),
    case("pairs: raw-A residual separate", 40, 96, 512, (HS | RING | RAW, 1, 1, 0), None, act="fp16", out="fp32", norm=False,
         residual="separate", kind="scalar stores"),
    case("pairs: f16s K384 residual in place", 40, 96, 384, (0, 1, 0, 128), (1, 2), act="fp16", out="fp32", norm=False,
         residual="alias", kind="scalar stores"),
    case("pairs: frag nf4 epi1", 40, 96, 512, (FRAG, 1, 0, 128), (0, 2), wname="nf4", quant=(128, False, "fp32"), epi=1,
         kind="scalar stores"),
    case("pairs: split-K residual separate", 40, 96, 1024, (SPLITK, 2, 0, 128), (1, 2), act="fp16", out="fp32", norm=False,
         residual="separate", kind="scalar stores"),
]


def scalar_variants(c):
    """the calls that leave the paired stores: odd ldo, odd ld_res (a separate residual), an output pointer off the pair
    alignment (an in-place residual moves with it)"""
    out = [dict(c, name=c["name"] + " / odd ldo", ldo_pad=3), dict(c, name=c["name"] + " / out pointer off", out_off=1)]
    if c["residual"] == "separate":
        out.append(dict(c, name=c["name"] + " / odd ld_res", ld_res_pad=1))
    return out


# residual == out against the same call with a separate copy of the residual: direct path and splitk_reduce_kernel
ALIAS_CASES = [
    case("alias: ring packed", 40, 96, 480, (HS | RING, 1, 1, 128), (1, 2), act="fp16", out="fp32", norm=False,
         residual="alias", kind="alias"),
    case("alias: raw-A M130", 130, 96, 512, (HS | RING | RAW, 1, 1, 0), None, act="fp16", out="fp32", norm=False, bias=True,
         residual="alias", kind="alias"),
    case("alias: split-K", 40, 96, 4096, (SPLITK, 8, 0, 128), (1, 2), act="fp16", out="fp32", norm=False, residual="alias",
         kind="alias"),
    case("alias: split-K M130 odd ldo", 130, 96, 1024, (SPLITK, 2, 0, 256), (1, 2), act="fp16", out="fp32", norm=False,
         residual="alias", ldo_pad=3, kind="alias"),
]

# fp16 saturation: rows hot enough that the reference leaves +-65504 in 1 % .. 50 % of the elements, both signs; the
# same inputs with a bf16 / fp32 output are not clamped
SATURATION = [
    case("saturation direct", 40, 96, 512, (HS | RING, 1, 1, 128), (0, 2), norm=False, bias=True, rows="hot", kind="saturation"),
    case("saturation split-K", 40, 96, 1024, (SPLITK, 2, 0, 128), (0, 2), norm=False, bias=True, rows="hot", kind="saturation"),
    case("saturation direct scalar stores", 40, 96, 512, (HS | RING, 1, 1, 128), (0, 2), norm=False, rows="hot", ldo_pad=3,
         kind="saturation"),
]

# the fragment image in a caller workspace of exactly the plan's bytes, and one byte less (per-call scratch)
WORKSPACE = [
    case("workspace nf4", 40, 96, 512, (FRAG, 1, 0, 128), (0, 2), wname="nf4", quant=(128, False, "fp32"), epi=1, bias=True,
         kind="workspace"),
    case("workspace fp8", 40, 96, 512, (FRAG, 1, 0, 128), (0, 2), wname="fp8_e4m3", quant=(128, False, "fp16"), bias=True,
         kind="workspace"),
]

# 256-row tiles (csrc/woq_gemm_f16t.h), at the sizes tests/test_gpu_prefill_gemm_forms.py uses: the qkv form, and gate/up
# with nb_m128 = 18, where the second 128-row image of the last workgroup holds one live row
TALL_CASES = [
    case("tall norm epi0 M2049", 2049, 22016, 256, (HS | RING | TALL, 1, 1, 2176), (0, 2), kind="256-row tiles"),
    case("tall norm epi1 M2177", 2177, 22016, 256, (HS | RING | TALL, 1, 1, 2304), (0, 2), epi=1, kind="256-row tiles"),
]

REFUSED = case("epi1 N48 refused", 40, 48, 512, None, None, epi=1)

CASES = _norm_cases() + _form_cases() + _edge_cases()
ALL = CASES + SCALAR_BASES + ALIAS_CASES + SATURATION + WORKSPACE + TALL_CASES
BY_NAME = {c["name"]: c for c in ALL}
assert len(BY_NAME) == len(ALL)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def weight(c):
    """-> tests/gemv_f32_reference.py `_weight`'s dict (blob, W64 [K, N], shuffle, ...) for the case's blob"""
    cols = c["N"] // 2 if c["epi"] == 1 else c["N"]
    return G._weight(c["K"], cols, c["quant"], c["wname"], "bf16", c["epi"], c["shuffle"])


@functools.lru_cache(maxsize=None)
def _rows(M, K, act, norm, kind):
    rng = np.random.Generator(np.random.PCG64(0).jumped())  # seed 0, a stream apart from the weights'
    x = rng.standard_normal((M, K)).astype(F32)
    if kind == "hot":  # |out| ~ s sqrt(K) 0.05: from a fifth of 65504 to three times it
        x *= (65504.0 / (0.05 * np.sqrt(K)) * np.geomspace(0.2, 3.0, M)).astype(F32)[:, None]
    else:
        for m in range(4 if M >= 4 else 0, M):
            x[m] *= F32([1, 0.25, 3, 0.01, 7][m % 5])
        if M >= 4:
            x[0] = 0
            if norm:
                x[1] = x[1] / np.abs(x[1]).max() * F32(4e-4)
            x[2, K // 3] *= 30
            x[3] *= F32(2.0 ** 12 if norm else 2.0 ** 4)
        if M > 128:
            x[128, (2 * K) // 3] *= 30
    x = round_act(x, act)
    g = (1 + 0.1 * rng.standard_normal(K)).astype(F32)
    return x, g, rng.standard_normal(22016).astype(F32), (4 * rng.standard_normal((M, 288))).astype(F32)


def build(c):
    """the case's inputs: dict(x [M, K], g | None, bias | None, residual [M, n_out] | None, n_out, + weight's entries)"""
    d = dict(weight(c))
    x, g, b, r = _rows(c["M"], c["K"], c["act"], c["norm"], c["rows"])
    n_out = c["N"] // 2 if c["epi"] == 1 else c["N"]
    assert d["W64"].shape == (c["K"], c["N"])
    d.update(x=x, g=g if c["norm"] else None, bias=b[:c["N"]] if c["bias"] else None,
             residual=np.ascontiguousarray(r[:, :n_out]) if c["residual"] != "none" else None, n_out=n_out)
    return d


def terms(c, d, rows=None, **kw):
    """reference(...) of case c on its inputs d (rows: a slice of the rows)"""
    s = slice(None) if rows is None else rows
    args = dict(shuffle=d["shuffle"], g=d["g"], bias=d["bias"], residual=None if d["residual"] is None else d["residual"][s],
                epi=c["epi"], out=c["out"], fp32_class=c["fp32_class"])
    args.update(kw)
    return reference(d["x"][s], d["W64"], **args)
