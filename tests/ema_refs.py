"""The model-EMA update (C ABI dyt_ema_update) restated in numpy: three fp32 roundings, no fused multiply-add

    ema' = fl( fl(d * ema) + fl(o * param) ),   d = (float)decay,  o = (float)(1. - decay) with the difference formed in double

-- torch's ``decay * ema_v + (1. - decay) * model_v`` on fp32 tensors (timm ModelEmaV2), to which tests/test_ema_refs_host.py pins it bit
for bit.  Plus what the tests share: the decays, the planted special values, the inputs and the bitwise comparison (NaN by position)."""
import numpy as np

DECAYS = (0.0, 0.5, 0.9, 0.9998, 0.99996, 1.0)
# +-0, +-inf, NaN, two fp32 denormals (1e-45 rounds to the smallest one), +-3e38 (d * x + o * y overflows for some pairs)
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-42, 1e-45, 3e38, -3e38], dtype=np.float32)


def scalars(decay):
    """(d, o) as the C floats the kernel receives."""
    decay = float(decay)
    return np.float32(decay), np.float32(1.0 - decay)


def ema_ref(ema, param, decay):
    d, o = scalars(decay)
    e, p = np.asarray(ema, dtype=np.float32), np.asarray(param, dtype=np.float32)
    with np.errstate(all="ignore"):
        a = d * e          # float32 scalar x float32 array: one rounding per element
        b = o * p
        out = a + b
    assert out.dtype == np.float32
    return out


def same_bits(a, b):
    """Bit for bit, a NaN matching any NaN at the same position (payloads and signs of NaNs are not compared)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def first_difference(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32).reshape(-1), np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
    bad = np.flatnonzero((np.isnan(a) != np.isnan(b)) | (~np.isnan(a) & ~np.isnan(b) & (a.view(np.uint32) != b.view(np.uint32))))
    return None if bad.size == 0 else (int(bad[0]), float(a[bad[0]]), float(b[bad[0]]), int(bad.size))


def draws(n, seed, scale=1.0, plant=True):
    """(ema, param): normal draws x scale with the special values planted at fixed strides where they fit -- each special meets a normal
    value, and over the first len(SPECIALS)^2 positions of a long enough array every special meets every special."""
    g = np.random.default_rng(seed)
    e = (g.standard_normal(n) * scale).astype(np.float32)
    p = (g.standard_normal(n) * scale).astype(np.float32)
    if plant:
        k = len(SPECIALS)
        for i in range(min(n, k * k)):      # pairs (special, special): i // k on the ema side, i % k on the param side
            e[i], p[i] = SPECIALS[(i // k) % k], SPECIALS[i % k]
        for j in range(k):                  # (special, normal) and (normal, special) further on
            if k * k + 2 * j + 1 < n:
                e[k * k + 2 * j] = SPECIALS[j]
                p[k * k + 2 * j + 1] = SPECIALS[j]
    return e, p
