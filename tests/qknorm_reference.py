"""float64 reference of the attention kernels with a per-head q / k RMSNorm in front of RoPE (Qwen3), for
tests/test_gpu_qknorm_kernels.py. It extends tests/attn_reference.py: the norm is HF's Qwen3RMSNorm,
x * rsqrt(mean(x^2) + eps) * w over head_dim, applied to every q head and every k head before the rotation; rotation,
storage rounding and attention are attn_reference's.
"""
import numpy as np

from tests import attn_reference as R


def qk_norm(x, w, eps):
    """RMSNorm of x [..., D] over its last axis with weights w [D], float64."""
    x = np.asarray(x, dtype=np.float64)
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps) * np.asarray(w, dtype=np.float64)


def ulp(x, fmt):
    """the spacing of `fmt` at |x| (float64): one unit of the format's last place, the subnormal spacing below its
    smallest normal"""
    m, emin, _ = R.FORMATS[fmt]
    x = np.abs(np.asarray(x, dtype=np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(x))
    e = np.where(np.isfinite(e), np.maximum(e, emin), emin)
    return np.exp2(e - m)


def _e4m3_table():
    v = np.empty(256)
    for c in range(256):
        s, e, m = (-1.0 if c & 0x80 else 1.0), (c >> 3) & 15, c & 7
        v[c] = np.nan if (e == 15 and m == 7) else s * (m / 8 * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
    return v


E4M3 = _e4m3_table()


def encode(x, fmt):
    """values exact in `fmt` ("fp16" | "fp8") -> raw storage (uint16 / uint8)"""
    x = np.asarray(x, dtype=np.float64)
    if fmt == "fp16":
        return x.astype(np.float16).view(np.uint16)
    mag = np.searchsorted(E4M3[:127], np.abs(x))
    assert np.array_equal(E4M3[np.minimum(mag, 126)], np.abs(x)), "value not exact in e4m3"
    return (mag | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def decode(raw, fmt):
    return raw.view(np.float16).astype(np.float64) if fmt == "fp16" else E4M3[raw]


def normed_rotated(x, w, eps, cos, sin):
    """x [..., D] -> RMSNorm with w, then rotate_half RoPE with cos / sin [..., D / 2]; float64, unrounded"""
    return R.rotate(qk_norm(x, w, eps), cos, sin)


def decode_attention(qkv, K, V, pos, heads, kv_heads, HD, q_w, k_w, eps, cos, sin):
    """One decode step. qkv fp32 [(heads + 2 kv) * HD] un-normalised, un-rotated; K, V [pos + 1, kv, HD] = the cache AS
    STORED after the step (row `pos` = the appended one). Returns (out [heads, HD], the float64 normalised and rotated
    new k [kv, HD] before storage rounding)."""
    rep = heads // kv_heads
    q = np.asarray(qkv[:heads * HD], dtype=np.float64).reshape(heads, HD)
    k = np.asarray(qkv[heads * HD:(heads + kv_heads) * HD], dtype=np.float64).reshape(kv_heads, HD)
    qr = normed_rotated(q, q_w, eps, cos[pos], sin[pos])
    kr = normed_rotated(k, k_w, eps, cos[pos], sin[pos])
    out = np.concatenate([R.attend(qr[h][None], K[:, h // rep], V[:, h // rep], [pos], 0)[0] for h in range(heads)])
    return out, kr
