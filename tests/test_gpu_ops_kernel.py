"""The four element ops behind the C ABI alone (csrc/woq_ops.hip rmsnorm_kernel, rope_kernel, silu_mul_kernel,
gelu_kernel) against tests/ops_reference.py, float64, through the public wrappers `qbits.rmsnorm`, `qbits.rope`,
`qbits.silu_mul`, `qbits.gelu`. No product code calls these (the engine fuses its own norms and rotations), so this file
and the one golden shape of test_ops_vs_oracle_and_hf_golden are all that watches them.

Cases (`ops_reference`): rmsnorm d 1 .. 8200 (whole waves idle, d no multiple of 256, 33 trips per thread) x rows
1 / 3 / 65 x eps 1e-5 / 1e-6 x five in -> out type pairs, every row family in one matrix (N(0, 1) 2^-e, 1, 2^e; all
zero; one-hot; constant; last element large); rope (tokens, heads, D) with D / 2 of 1, 3, 32 and 64, one partial block,
3.75 blocks and whole blocks, positions that repeat, step back and touch both table ends, fp32 / fp16 / bf16 in place;
silu_mul and gelu (tanh and erf) at n around the 256-thread block and around 524288 = 2048 x 256, where the grid-stride
loop takes its second and third trip, with the specials (+-0 .. +-1e4, NaN) in the first block, the last block and
across that boundary.

Every output lives between guard elements in a buffer pre-filled with NaN (fp32) or a large finite pattern (16-bit).
Asserted after each call: every element inside the band derived in ops_reference (none taken from a kernel's output)
and, the sharper form for 16-bit storage, between the roundings of ref - b32 and ref + b32 (`ops_reference.inside`);
the guards unchanged; every input byte-identical; a second call gives the same bytes; an all-zero RMSNorm row gives
zeros; RoPE at position 0 leaves x bit-identical; NaN in gives NaN out; silu_mul / gelu in place give the bytes of the
out-of-place call; zero rows / tokens / elements touch nothing.

Refusals: every malformed argument raises RuntimeError "QBits: ..." on the host. Those tests run with the library
handle replaced by an object that fails on any use, so a missing check shows as a failure, never as a launch.

Largest err / band observed on an MI355X (printed under -s) and, beside it, what the correctly rounded reference alone
uses of the same band; the bands are the derived ones, not fitted to these. No numeric case failed and no kernel was
changed.
  op, types              kernel  reference alone
  rmsnorm fp32 -> fp32   0.314   0.095
  rmsnorm bf16 -> fp32   0.313   0.095
  rmsnorm fp16 -> fp16   0.999   0.999
  rmsnorm bf16 -> bf16   1.000   1.000
  rmsnorm fp32 -> bf16   1.000   1.000
  rope fp32              0.567   0.327
  rope fp16              0.999   0.999
  rope bf16              1.000   1.000
  silu_mul fp32          1.000   0.248   (0.400 outside the flush region)
  silu_mul fp16, bf16    1.000   1.000
  gelu tanh fp32         0.122   0.062
  gelu erf fp32          0.059   0.028
  gelu tanh fp16 / bf16  1.000 / 0.999   the same
  gelu erf fp16 / bf16   1.000 / 0.998   the same
Every figure above 0.5:
  16-bit outputs, ~1.0: the reference's own storage rounding. A float64 value next to a rounding tie of the out type is
    half an ulp from its rounded self, and the half ulp is all but the whole band there; the rounded reference alone
    reaches the same figure. What the kernel adds is held by `inside`: the stored value is the rounded reference except
    within b32 of a tie.
  silu_mul fp32, 1.000: the kernel, by construction. At gate -89, -104, -1e4 expf overflows, the kernel returns a zero
    and the band there is |ref| itself (<= 89 |up| / FLT_MAX). Elsewhere 0.400 of 9 u |ref|.
  rope fp32, 0.567: the kernel: two rounded products and a rounded sum use up to 2 u of the 3 u (|a c| + |b s|); the
    fp32 restatement reads 0.57 - 0.60 on the same inputs.
"""
import numpy as np
import pytest
import torch

from tests import ops_reference as R

pytestmark = pytest.mark.gpu

TORCH = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
GUARD = 64
GARBAGE = 0x7BCD  # fp16 63904, bf16 1.3e36: large, finite, no value a kernel here produces


@pytest.fixture(scope="module")
def qbits():
    from intel_extension_for_transformers_amd import qbits as q

    return q


def dev(values, fmt):
    """float64 values (already representable in fmt) -> device tensor of that type, bit-exact"""
    bits = np.ascontiguousarray(R.to_bits(values, fmt))
    if fmt == "bf16":
        return torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(bits).cuda()


def host(t, fmt):
    """device tensor -> float64 values, exactly"""
    if fmt == "bf16":
        return R.widen(t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), fmt)
    return t.cpu().numpy().astype(np.float64)


def raw(t):
    """the tensor's bytes as an integer tensor (NaN-safe comparison)"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).clone()


def guarded(shape, fmt):
    """(buffer, view): a contiguous tensor of `shape` with GUARD elements of fill on both sides, itself filled too"""
    n = int(np.prod(shape))
    buf = torch.empty(n + 2 * GUARD, dtype=TORCH[fmt], device="cuda")
    if fmt == "fp32":
        buf.fill_(float("nan"))
    else:
        buf.view(torch.int16).fill_(GARBAGE)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf, fmt):
    fresh, _ = guarded((buf.numel() - 2 * GUARD,), fmt)
    a, b = raw(buf), raw(fresh)
    return torch.equal(a[:GUARD], b[:GUARD]) and torch.equal(a[-GUARD:], b[-GUARD:])


def untouched(view, fmt):
    fresh, _ = guarded((view.numel(),), fmt)
    return torch.equal(raw(view).reshape(-1), raw(fresh)[GUARD:GUARD + view.numel()])


def check(name, out, ref, b32, band, fmt):
    got = host(out, fmt)
    r = R.ratio(got, ref, band, fmt)
    worst = float(r.max()) if r.size else 0.0
    own = R.ratio(R.stored(ref, fmt), ref, band, fmt)  # what the correctly rounded reference alone uses of the band
    print("RATIO %s %.3f (rounded reference alone %.3f)" % (name, worst, float(own.max()) if own.size else 0.0))
    assert worst <= 1.0, (name, worst, np.unravel_index(int(r.argmax()), r.shape))
    ok = R.inside(got, ref, b32, fmt)  # the same band without the half ulp: between the roundings of ref -+ b32
    assert np.all(ok), (name, np.unravel_index(int(np.argmin(ok)), ok.shape))
    return worst


# ---- rmsnorm ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.RMS_D)
@pytest.mark.parametrize("types", R.RMS_TYPES, ids=lambda t: "%s-%s" % t)
def test_rmsnorm(qbits, types, d):
    in_fmt, out_fmt = types
    x64, w64 = R.rmsnorm_inputs(d, in_fmt)
    w = torch.from_numpy(w64.astype(np.float32)).cuda()
    worst = 0.0
    for rows in R.RMS_ROWS:
        x = dev(x64[:rows], in_fmt)
        x0, w0 = raw(x), raw(w)
        for eps in R.RMS_EPS:
            ref, b32 = R.rmsnorm_ref(x64[:rows], w64, eps)
            buf, out = guarded((rows, d), out_fmt)
            assert qbits.rmsnorm(x, w, eps, out=out) is out
            worst = max(worst, check("rmsnorm %s->%s d=%d rows=%d eps=%g" % (in_fmt, out_fmt, d, rows, eps), out, ref,
                                     b32, R.rmsnorm_band(ref, b32, out_fmt), out_fmt))
            zero = ~np.any(x64[:rows] != 0, axis=-1)
            assert np.all(host(out, out_fmt)[zero] == 0)
            assert guards_intact(buf, out_fmt)
            assert torch.equal(raw(x), x0) and torch.equal(raw(w), w0)
            buf2, out2 = guarded((rows, d), out_fmt)
            qbits.rmsnorm(x, w, eps, out=out2)
            assert torch.equal(raw(buf2), raw(buf))
    print("RATIO-MAX rmsnorm %s->%s %.3f" % (in_fmt, out_fmt, worst))
    # an allocated out has x's type; a 16-bit weight is widened, not reinterpreted
    y = qbits.rmsnorm(x, w.to(torch.bfloat16), 1e-5)
    assert y.dtype == x.dtype and y.shape == x.shape
    ref, b32 = R.rmsnorm_ref(x64, R.to_storage(w64, "bf16"), 1e-5)
    check("rmsnorm %s bf16 weight d=%d" % (in_fmt, d), y, ref, b32, R.rmsnorm_band(ref, b32, in_fmt), in_fmt)


@pytest.mark.parametrize("fmt", R.DTYPES)
def test_rmsnorm_zero_rows_is_a_no_op(qbits, fmt):
    buf, out = guarded((0, 257), fmt)
    w = torch.ones(257, device="cuda")
    assert qbits.rmsnorm(torch.empty(0, 257, dtype=TORCH[fmt], device="cuda"), w, 1e-5, out=out) is out
    torch.cuda.synchronize()
    assert untouched(buf, fmt)


# ---- rope ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.DTYPES)
@pytest.mark.parametrize("shape", R.ROPE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rope(qbits, shape, fmt):
    x64, pos_np = R.rope_inputs(shape, fmt)
    cos_np, sin_np = R.rope_tables(shape[2])
    pos, cos, sin = torch.from_numpy(pos_np.copy()).cuda(), torch.from_numpy(cos_np.copy()).cuda(), torch.from_numpy(sin_np.copy()).cuda()
    p0, c0, s0 = raw(pos), raw(cos), raw(sin)
    ref, b32 = R.rope_ref(x64, pos_np, cos_np, sin_np)
    xin = dev(x64, fmt)
    buf, x = guarded(shape, fmt)
    x.copy_(xin)
    assert qbits.rope(x, pos, cos, sin) is x
    check("rope %s %s" % (fmt, shape), x, ref, b32, R.rope_band(ref, b32, fmt), fmt)
    assert guards_intact(buf, fmt)
    assert torch.equal(raw(pos), p0) and torch.equal(raw(cos), c0) and torch.equal(raw(sin), s0)
    at0 = torch.from_numpy(pos_np == 0).cuda()
    assert torch.equal(raw(x)[at0], raw(xin)[at0])  # position 0: cos 1, sin 0
    buf2, x2 = guarded(shape, fmt)
    x2.copy_(xin)
    qbits.rope(x2, pos, cos, sin)
    assert torch.equal(raw(buf2), raw(buf))
    x2.copy_(xin)
    qbits.rope(x2, torch.zeros_like(pos), cos, sin)
    assert torch.equal(raw(x2), raw(xin)) and guards_intact(buf2, fmt)


@pytest.mark.parametrize("fmt", R.DTYPES)
def test_rope_zero_tokens_is_a_no_op(qbits, fmt):
    cos, sin = (torch.from_numpy(t.copy()).cuda() for t in R.rope_tables(6))
    buf, x = guarded((0, 2, 6), fmt)
    assert qbits.rope(x, torch.empty(0, dtype=torch.int32, device="cuda"), cos, sin) is x
    torch.cuda.synchronize()
    assert untouched(buf, fmt)


# ---- silu_mul and gelu -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.ELEM_N)
@pytest.mark.parametrize("fmt", R.DTYPES)
def test_silu_mul(qbits, fmt, n):
    a64, b64 = R.elementwise_inputs(n, fmt)
    ref, b32 = R.silu_mul_ref(a64, b64)
    gate, up = dev(a64, fmt), dev(b64, fmt)
    g0, u0 = raw(gate), raw(up)
    buf, out = guarded((n,), fmt)
    assert qbits.silu_mul(gate, up, out=out) is out
    band = R.silu_mul_band(ref, b32, fmt)
    check("silu_mul %s n=%d" % (fmt, n), out, ref, b32, band, fmt)
    kept = ~(-a64 > R.LOG_FLT_MAX)  # where expf overflows the result is a zero and err / band is 1 by construction
    print("RATIO silu_mul-unflushed %s n=%d %.3f" % (fmt, n, R.ratio(host(out, fmt), ref, band, fmt)[kept].max(initial=0.0)))
    assert np.all(host(out, fmt)[~kept & ~np.isnan(ref)] == 0)
    assert np.array_equal(np.isnan(host(out, fmt)), np.isnan(ref))
    assert guards_intact(buf, fmt)
    assert torch.equal(raw(gate), g0) and torch.equal(raw(up), u0)
    for which in ("fresh", "gate", "up"):  # a second call, then in place on either input
        buf2, out2 = guarded((n,), fmt)
        g, u = gate, up
        if which == "gate":
            out2.copy_(gate)
            g = out2
        elif which == "up":
            out2.copy_(up)
            u = out2
        qbits.silu_mul(g, u, out=out2)
        assert torch.equal(raw(buf2), raw(buf)), which
    y = qbits.silu_mul(gate, up)
    assert y.dtype == gate.dtype and torch.equal(raw(y), raw(out))


@pytest.mark.parametrize("form", ["tanh", "erf"])
@pytest.mark.parametrize("n", R.ELEM_N)
@pytest.mark.parametrize("fmt", R.DTYPES)
def test_gelu(qbits, fmt, form, n):
    v64, _ = R.elementwise_inputs(n, fmt)
    ref, b32 = R.gelu_ref(v64, form)
    x = dev(v64, fmt)
    x0 = raw(x)
    buf, out = guarded((n,), fmt)
    assert qbits.gelu(x, form, out=out) is out
    check("gelu %s %s n=%d" % (form, fmt, n), out, ref, b32, R.gelu_band(ref, b32, fmt), fmt)
    assert np.array_equal(np.isnan(host(out, fmt)), np.isnan(ref))
    assert guards_intact(buf, fmt)
    assert torch.equal(raw(x), x0)
    for which in ("fresh", "in place"):
        buf2, out2 = guarded((n,), fmt)
        if which == "in place":
            out2.copy_(x)
        qbits.gelu(out2 if which == "in place" else x, form, out=out2)
        assert torch.equal(raw(buf2), raw(buf)), which
    if form == "erf":
        assert torch.equal(raw(qbits.gelu(x, "none")), raw(out))
    else:
        assert torch.equal(raw(qbits.gelu(x)), raw(out))  # the default is the tanh form


@pytest.mark.parametrize("fmt", R.DTYPES)
def test_elementwise_zero_elements_is_a_no_op(qbits, fmt):
    e = torch.empty(0, dtype=TORCH[fmt], device="cuda")
    for call in (lambda o: qbits.silu_mul(e, e, out=o), lambda o: qbits.gelu(e, "tanh", out=o), lambda o: qbits.gelu(e, "erf", out=o)):
        buf, out = guarded((0,), fmt)
        assert call(out) is out
        torch.cuda.synchronize()
        assert untouched(buf, fmt)


# ---- refusals: on the host, before anything is launched --------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("a refused call reached the library: %s" % name)


@pytest.fixture
def refusing(qbits, monkeypatch):
    """qbits with the library handle taken away: a wrapper that lets a bad argument through fails here, on the host"""
    from intel_extension_for_transformers_amd import _lib

    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    return qbits


def _refused(fn):
    with pytest.raises(RuntimeError, match="QBits:"):
        fn()


def test_rope_refusals(refusing):
    q = refusing
    T, H, D = 5, 3, 8
    x = torch.randn(T, H, D, device="cuda")
    x0 = raw(x)
    pos = torch.arange(T, dtype=torch.int32, device="cuda")
    cos, sin = torch.ones(64, D // 2, device="cuda"), torch.zeros(64, D // 2, device="cuda")
    wide = torch.ones(64, D, device="cuda")
    _refused(lambda: q.rope(x, pos.long(), cos, sin))
    _refused(lambda: q.rope(x, pos.cpu(), cos, sin))
    _refused(lambda: q.rope(x, pos[:T - 1], cos, sin))
    _refused(lambda: q.rope(x, torch.arange(2 * T, dtype=torch.int32, device="cuda")[::2], cos, sin))
    _refused(lambda: q.rope(x, pos, cos.half(), sin))
    _refused(lambda: q.rope(x, pos, cos, sin.half()))
    _refused(lambda: q.rope(x, pos, wide, wide))  # second dimension D, not D / 2
    _refused(lambda: q.rope(x, pos, cos, torch.zeros(64, D // 2 - 1, device="cuda")))
    _refused(lambda: q.rope(x, pos, cos, sin[:32]))
    _refused(lambda: q.rope(x, pos, wide[:, ::2], sin))  # the right shape, strided
    _refused(lambda: q.rope(x, pos, cos, wide[:, ::2]))
    _refused(lambda: q.rope(x, pos, cos.reshape(-1), sin.reshape(-1)))
    _refused(lambda: q.rope(x, pos, cos.cpu(), sin))
    _refused(lambda: q.rope(torch.randn(T, H, 7, device="cuda"), pos, cos, sin))  # odd D
    _refused(lambda: q.rope(torch.randn(T, H, 2 * D, device="cuda")[:, :, ::2], pos, cos, sin))
    _refused(lambda: q.rope(x.permute(1, 0, 2), pos[:H], cos, sin))
    _refused(lambda: q.rope(x.reshape(T * H, D), pos, cos, sin))
    _refused(lambda: q.rope(x.cpu(), pos, cos, sin))
    _refused(lambda: q.rope(x.double(), pos, cos, sin))
    assert torch.equal(raw(x), x0)


def test_rmsnorm_refusals(refusing):
    q = refusing
    x = torch.randn(3, 64, device="cuda")
    w = torch.ones(64, device="cuda")
    _refused(lambda: q.rmsnorm(x, w[:63], 1e-5))
    _refused(lambda: q.rmsnorm(x, torch.ones(65, device="cuda"), 1e-5))
    _refused(lambda: q.rmsnorm(x, torch.ones(1, device="cuda"), 1e-5))
    _refused(lambda: q.rmsnorm(x, torch.ones(3, 64, device="cuda"), 1e-5))
    _refused(lambda: q.rmsnorm(x, w.cpu(), 1e-5))
    _refused(lambda: q.rmsnorm(x, w.half()[:32], 1e-5))
    _refused(lambda: q.rmsnorm(x, w, 1e-5, out=torch.empty(3, 32, device="cuda")))
    _refused(lambda: q.rmsnorm(x, w, 1e-5, out=torch.empty(2, 64, device="cuda")))
    _refused(lambda: q.rmsnorm(x, w, 1e-5, out=torch.empty(64, 3, device="cuda")))
    _refused(lambda: q.rmsnorm(x, w, 1e-5, out=torch.empty(3, 128, device="cuda")[:, ::2]))
    _refused(lambda: q.rmsnorm(x, w, 1e-5, out=torch.empty(64, 3, device="cuda").t()))
    _refused(lambda: q.rmsnorm(x, w, 1e-5, out=torch.empty(3, 64)))
    _refused(lambda: q.rmsnorm(x, w, 1e-5, out=torch.empty(3, 64, dtype=torch.float64, device="cuda")))
    _refused(lambda: q.rmsnorm(x, w, 1e-5, out=torch.empty(3, 64, dtype=torch.int16, device="cuda")))
    _refused(lambda: q.rmsnorm(x, w, 1e-5, out=torch.empty(3, 64, dtype=torch.float8_e4m3fn, device="cuda")))
    _refused(lambda: q.rmsnorm(x.cpu(), w, 1e-5))
    _refused(lambda: q.rmsnorm(x.double(), w, 1e-5))


def test_silu_mul_refusals(refusing):
    q = refusing
    g = torch.randn(300, device="cuda")
    _refused(lambda: q.silu_mul(g, g.half()))
    _refused(lambda: q.silu_mul(g.bfloat16(), g.half()))
    _refused(lambda: q.silu_mul(g, g[:299]))
    _refused(lambda: q.silu_mul(g, torch.randn(301, device="cuda")))
    _refused(lambda: q.silu_mul(g, g.cpu()))
    _refused(lambda: q.silu_mul(g, g, out=torch.empty(300, dtype=torch.float16, device="cuda")))
    _refused(lambda: q.silu_mul(g.half(), g.half(), out=torch.empty(300, device="cuda")))
    _refused(lambda: q.silu_mul(g, g, out=torch.empty(299, device="cuda")))
    _refused(lambda: q.silu_mul(g, g, out=torch.empty(600, device="cuda")[::2]))
    _refused(lambda: q.silu_mul(g, g, out=torch.empty(300)))
    _refused(lambda: q.silu_mul(g.cpu(), g.cpu()))
    _refused(lambda: q.silu_mul(g.double(), g.double()))


def test_gelu_refusals(refusing):
    q = refusing
    x = torch.randn(300, device="cuda")
    _refused(lambda: q.gelu(x, "tanh", out=torch.empty(300, dtype=torch.bfloat16, device="cuda")))
    _refused(lambda: q.gelu(x.half(), "erf", out=torch.empty(300, device="cuda")))
    _refused(lambda: q.gelu(x, "tanh", out=torch.empty(299, device="cuda")))
    _refused(lambda: q.gelu(x, "tanh", out=torch.empty(600, device="cuda")[::2]))
    _refused(lambda: q.gelu(x, "tanh", out=torch.empty(300)))
    for word in ("Tanh", "gelu_new", "", None, True, 1):
        _refused(lambda: q.gelu(x, word))
    _refused(lambda: q.gelu(x.cpu()))
    _refused(lambda: q.gelu(x.double()))
