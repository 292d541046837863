"""numpy statement of the per-read normalisation of include/vbz_gpu.h (vbz_gpu_normalization): the statistics from the read's sorted
16-bit values, in float64 with every operation rounded once (Python floats: no fused multiply-add), and the constants they give."""
import numpy as np

MED_MAD, QUANTILE = 1, 2
FLT_MIN = float(np.finfo(np.float32).tiny)

# (method, quantile_a, quantile_b, shift_mul, scale_mul, shift_min, scale_min)
BONITO = (MED_MAD, 0.0, 0.0, 1.0, 1.4826, float("-inf"), FLT_MIN)
DORADO = (QUANTILE, 0.2, 0.9, 0.51, 0.53, 10.0, 1.0)
EXTREMES = (QUANTILE, 0.0, 1.0, 1.0, 0.25, -1e30, 1e-3)
SAME_Q = (QUANTILE, 0.5, 0.5, 2.0, 3.0, float("-inf"), 2.0 ** -100)
PARAMS = [BONITO, DORADO, EXTREMES, SAME_Q]


def f64(v):
    """a float32 field as the device reads it: rounded to float32, then widened"""
    return float(np.float64(np.float32(v)))


def quantile(s, q):
    """numpy's quantile (method "linear") of the sorted float64 values s at the float32 q, restated"""
    T = len(s)
    h = f64(q) * float(T - 1)
    j = int(np.floor(h))
    t = h - j
    a = float(s[j])
    b = float(s[min(j + 1, T - 1)])
    d = b - a
    return a + d * t if t < 0.5 else b - d * (1.0 - t)


def median_sorted(s):
    T = len(s)
    return (float(s[(T - 1) // 2]) + float(s[T // 2])) / 2.0


def stats(x, norm):
    """(c, w) of the read's values x (int16 or uint16 numpy array) under norm"""
    T = len(x)
    if T == 0:
        return 0.0, 0.0
    s = np.sort(x.astype(np.float64))
    if norm[0] == MED_MAD:
        c = median_sorted(s)
        w = median_sorted(np.sort(np.abs(s - c)))
        return c, w
    qa, qb = quantile(s, norm[1]), quantile(s, norm[2])
    return qa + qb, qb - qa


def constants(c, w, norm):
    """-> (shift, scale, store offset, store scale), float32 each: shift = max(shift_min, shift_mul c), scale = max(scale_min,
    scale_mul w), the store's offset = -shift and scale' = float32(1 / float64(scale))"""
    _, _, _, smul, kmul, smin, kmin = norm
    shift = np.float32(max(f64(smin), f64(smul) * c))
    scale = np.float32(max(f64(kmin), f64(kmul) * w))
    inv = np.float32(1.0 / np.float64(scale))
    return shift, scale, np.float32(-shift), inv


def shift_scale(x, norm):
    """the two float32 values the table gets for read x"""
    shift, scale, _, _ = constants(*stats(x, norm), norm)
    return shift, scale
