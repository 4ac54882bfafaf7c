"""float64 restatement of Hugging Face's RoPE parameterisations (transformers/modeling_rope_utils.py: `default`,
`linear`, `llama3`, `yarn`) for tests/test_rope_scaling_cpu.py: the inverse frequencies, the angle position * inv_freq
and cos / sin times the attention factor, every step in float64 (numpy) from the config's Python numbers.
"""
import math

import numpy as np


def inv_freq(head_dim, theta, rs=None, max_position_embeddings=None):
    """(inv_freq float64 [head_dim / 2], attention factor) for an HF rope_scaling / rope_parameters dict `rs`."""
    rs = rs or {}
    rtype = rs.get("rope_type") or rs.get("type") or "default"
    dim = head_dim
    base = 1.0 / float(theta) ** (np.arange(0, dim, 2, dtype=np.float64) / dim)
    if rtype == "default":
        return base, 1.0
    factor = rs.get("factor")
    if rtype == "linear":
        return base / factor, 1.0
    orig = rs.get("original_max_position_embeddings") or max_position_embeddings
    if rtype == "llama3":
        low_f, high_f = rs["low_freq_factor"], rs["high_freq_factor"]
        wavelen = 2 * math.pi / base
        out = np.where(wavelen > orig / low_f, base / factor, base)
        smooth = (orig / wavelen - low_f) / (high_f - low_f)
        smoothed = (1 - smooth) * out / factor + smooth * out
        medium = ~(wavelen < orig / high_f) & ~(wavelen > orig / low_f)
        return np.where(medium, smoothed, out), 1.0
    assert rtype == "yarn", rtype
    if factor is None:
        factor = max_position_embeddings / orig

    def mscale_of(scale, mscale=1):
        return 1.0 if scale <= 1 else 0.1 * mscale * math.log(scale) + 1.0

    att = rs.get("attention_factor")
    if att is None:
        ms, ms_all = rs.get("mscale"), rs.get("mscale_all_dim")
        att = mscale_of(factor, ms) / mscale_of(factor, ms_all) if ms and ms_all else mscale_of(factor)
    beta_fast, beta_slow = rs.get("beta_fast") or 32, rs.get("beta_slow") or 1

    def correction_dim(rot):
        return (dim * math.log(orig / (rot * 2 * math.pi))) / (2 * math.log(theta))

    low, high = correction_dim(beta_fast), correction_dim(beta_slow)
    if rs.get("truncate", True):
        low, high = math.floor(low), math.ceil(high)
    low, high = max(low, 0), min(high, dim - 1)
    if low == high:
        high += 0.001
    ramp = np.clip((np.arange(dim // 2, dtype=np.float64) - low) / (high - low), 0, 1)
    ext = 1 - ramp
    return (base / factor) * (1 - ext) + base * ext, float(att)


def tables(positions, head_dim, theta, rs=None, max_position_embeddings=None):
    """(cos, sin) float64 [len(positions), head_dim / 2], times the attention factor"""
    f, att = inv_freq(head_dim, theta, rs, max_position_embeddings)
    ang = np.asarray(positions, dtype=np.float64)[:, None] * f[None, :]
    return np.cos(ang) * att, np.sin(ang) * att
