"""The RTN quantiser kernels alone (csrc/woq_pack.hip rtn_kernel, rtn_lut_kernel, rtn_fp8_kernel) against
tests/quant_reference.py, the rule in float64. Public path only: `qbits.quantize_to_packed_weight`, then
`acquire_packed_weight_info(blob, 9)` (scales) / `(blob, 10)` (zero points) and `dequantize_packed_weight` in both
orientations.

Types: int4_clip, int8, int3_clip, int2_clip (sym and asym), nf4, fp4_e2m1, fp4_e2m1_bnb, fp8_e4m3 and fp8_e5m2 (fp32
and fp8_e8m0 scales); fp16 / bf16 scale storage on int4_clip, int8 and fp8_e4m3. Shapes [K, N], group
(`quant_reference.SHAPES`): (128, 24, 32), (160, 24, 64) with a tail group of 32 rows, (96, 17, 128) where group > K
means per channel and N is ragged, (512, 20, -1); the weight handed over as [K, N] and as [N, K]. Every matrix holds
every input family of `quant_reference.families` (seed 0): 0.05 N(0, 1); one-sided U[1, 1.1], -U[0.2, 0.9], U[0, 1)
touching zero; constant 0.3, constant -2.5, all zero, all zero but one, +0 / -0 mixed; N(0, 1) 2^e with a planted
+-3 2^e, e over -20 .. 20 (4 .. 8 with 16-bit scales); exact rounding ties under a planted range whose scale is 1.

Asserted per case, bounds from `quant_reference.bounds` (none taken from a kernel's output):
  scale    |s_dev - s_ref| <= (2^-22 + u) s_ref, u = 0 / 2^-11 / 2^-8 for fp32 / fp16 / bf16 storage; 1 for an all-zero
           group; fp8_e8m0: the power of two demanded (a neighbour only within 2^-23 relative of a power of two)
  elem     integer types, every element: |W' - w| <= (0.5 + levels (2^-22 + u)) s_dev
  zp       equal to the reference's, or a neighbour where -lo / s is within levels 2^-22 of a tie
  near     table / fp8: W' / s_dev is a table value and no finite entry is nearer to w / s_dev by more than
           2^-22 max|table|
  ties     in the tie cells W' equals the rule exactly: half to even (integers), lowest code (fp4_e2m1, fp8)
  lockstep the blob equals the oracle's quantise + repack byte for byte; two runs give the same bytes;
           dequantize(transpose=True) is the transpose of dequantize(transpose=False)

`test_one_sided_weight_through_woq_linear`: what a user sees — a [64, 256] weight 1 + 0.05 N(0, 1), asym int4 at
group 32, through `woq_linear` at M = 1 and M = 40 against x @ w in float64, within sum_k |x_k| 0.5 s_dev[group(k)]
plus the routes' own tolerance (2e-6 sum |x||w| + 1e-5, tests/test_gpu_parity.py). With the asym scale taken over
(max - min) every code of such a weight saturated and the product was off by orders of magnitude.

Largest err / bound observed on an MI355X (printed under -s), [K, N] and [N, K] alike; the bounds are the derived
ones above, not fitted to these. elem is 1 - 1e-5 with fp32 scales because the exact ties sit at half a step; near is
0 everywhere (the chosen entry was always a nearest one); no zero point moved off the reference's.
  type / scales          scale   elem  | type / scales          scale   elem
  int4_clip fp32 sym     0.210  1.000  | int4_clip fp16 sym     0.871  0.989
  int4_clip fp32 asym    0.340  1.000  | int4_clip fp16 asym    0.953  0.994
  int8      fp32 sym     0.244  1.000  | int8      fp16 sym     0.905  0.870
  int8      fp32 asym    0.409  1.000  | int8      fp16 asym    0.843  0.930
  int3_clip fp32 sym     0.166  1.000  | int4_clip bf16 sym     0.894  0.933
  int3_clip fp32 asym    0.369  1.000  | int4_clip bf16 asym    0.937  0.956
  int2_clip fp32 sym     0      1.000  | int8      bf16 sym     0.882  0.577
  int2_clip fp32 asym    0.357  1.000  | int8      bf16 asym    0.938  0.941
  nf4, fp4_e2m1_bnb      0             | fp8_e4m3  fp16         0.871
  fp4_e2m1               0.166         | fp8_e4m3  bf16         0.894
  fp8_e4m3 / e5m2 fp32   0.210         | fp8 with fp8_e8m0 scales: the power of two demanded, no neighbour taken
  woq_linear on the one-sided weight: 0.115 (M = 1), 0.152 (M = 40)
Before the stored scale was used to pick the fp8 codes (rtn_fp8_kernel), fp8_e4m3 with fp16 scales missed `near` by
1.2e4 times its slop (0.0029 max|table|, seen on the CPU oracle, which is byte-identical): an element whose
quotient by the fp32 scale lay next to a midpoint was not the nearest to what dequantisation multiplies by.
"""
import numpy as np
import pytest
import torch

from tests import quant_reference as Q
from tests.test_quant_reference_cpu import TYPES, case_input, oracle_quantize, type_id

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qbits():
    from intel_extension_for_transformers_amd import qbits as q

    return q


def _device(qbits, wt, transpose, K, N, group, wname, sname, asym):
    """-> (blob bytes, scales [G, N], zero points 0 .. levels [G, N] or None, W' [K, N], W' transposed [N, K])"""
    blob = qbits.quantize_to_packed_weight(torch.from_numpy(wt).cuda(), transpose, group, "fp32", wname, sname, asym)
    s = qbits.acquire_packed_weight_info(blob, 9).cpu().numpy()
    z = None
    if asym:
        z = qbits.acquire_packed_weight_info(blob, 10).cpu().numpy().astype(np.int64) + 2 ** (Q.INT_BITS[wname] - 1)
    W = torch.full((K, N), np.nan, dtype=torch.float32, device="cuda")
    qbits.dequantize_packed_weight(blob, W, False, "fp32", wname, sname)
    Wt = torch.full((N, K), np.nan, dtype=torch.float32, device="cuda")
    qbits.dequantize_packed_weight(blob, Wt, True, "fp32", wname, sname)
    return blob.cpu().numpy().view(np.uint8), s, z, W.cpu().numpy(), Wt.cpu().numpy()


@pytest.mark.parametrize("transpose", [False, True], ids=["kn", "nk"])
@pytest.mark.parametrize("typ", TYPES, ids=type_id)
def test_quantize_kernels_against_reference(qbits, typ, transpose):
    wname, sname, asym = typ
    worst = {}
    for K, N, group in Q.SHAPES:
        w, fam, e = case_input(K, N, group, wname, sname, asym)
        wt = np.ascontiguousarray(w.T) if transpose else w
        blob, s, z, W, Wt = _device(qbits, wt, transpose, K, N, group, wname, sname, asym)
        rep = Q.check(w, group, wname, sname, asym, s, z, W, fam)
        for k, v in rep.items():
            worst[k] = max(worst.get(k, 0), v)
        assert np.array_equal(Wt, W.T), "orientation"
        assert np.array_equal(blob, oracle_quantize(wt, transpose, group, wname, sname, asym)[0]), "lockstep"
        again = _device(qbits, wt, transpose, K, N, group, wname, sname, asym)[0]
        assert np.array_equal(blob, again), "determinism"
    print("\n%s %s: largest err / bound %s" % (type_id(typ), "nk" if transpose else "kn", worst))


def test_one_sided_weight_through_woq_linear(qbits):
    rng = np.random.default_rng(0)
    N, K, group = 64, 256, 32
    w = (1 + 0.05 * rng.standard_normal((N, K))).astype(np.float32)  # nn.Linear layout
    blob = qbits.quantize_to_packed_weight(torch.from_numpy(w).cuda(), True, group, "fp32", "int4_clip", "fp32", True)
    s = qbits.acquire_packed_weight_info(blob, 9).cpu().numpy().astype(np.float64)  # [G, N]
    sk = np.repeat(s, group, axis=0)  # [K, N]
    w64 = w.astype(np.float64).T
    for M in (1, 40):  # the decode GEMV and the MFMA GEMM
        x = rng.standard_normal((M, K)).astype(np.float32)
        out = torch.zeros(M, N, dtype=torch.float32, device="cuda")
        qbits.woq_linear(torch.from_numpy(x).cuda(), blob, torch.empty(0), out, "fp32", "int4_clip", "fp32", True)
        ax = np.abs(x).astype(np.float64)
        bound = ax @ (0.5 * sk) + 2e-6 * (ax @ np.abs(w64)) + 1e-5
        err = np.abs(out.cpu().numpy() - x.astype(np.float64) @ w64)
        print("\nM = %d: largest err / bound %.4f (err %.4g of max|ref| %.4g)" % (
            M, (err / bound).max(), err.max(), np.abs(x.astype(np.float64) @ w64).max()))
        assert (err <= bound).all(), M
