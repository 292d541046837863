"""The numpy statement of the normalisation statistics (tests/norm_ref.py) held to np.median and np.quantile on random reads (CPU)."""
import numpy as np
import pytest

import norm_ref as R


def reads(seed):
    rng = np.random.default_rng(seed)
    out = []
    for T in (1, 2, 3, 4, 5, 7, 8, 100, 101, 1000, 4097):
        out.append(rng.integers(-32768, 32768, T).astype(np.int16))                     # full range
        out.append((300 + rng.normal(0, 40, T)).astype(np.int16))                        # signal-like
        out.append(rng.integers(0, 65536, T).astype(np.uint16))                          # uint16
        out.append(np.full(T, rng.integers(-32768, 32768), np.int16))                    # constant
        out.append(np.where(rng.random(T) < 0.5, -32768, 32767).astype(np.int16))        # two values, far apart
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_median_mad_is_numpy(seed):
    for x in reads(seed):
        v = x.astype(np.float64)
        c, w = R.stats(x, R.BONITO)
        med = np.median(v)
        assert c == med, (len(x), c, med)
        assert w == np.median(np.abs(v - med)), len(x)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_quantiles_are_numpy(seed):
    for x in reads(seed):
        v = x.astype(np.float64)
        for q in (0.0, 0.2, 0.5, 0.9, 1.0, 0.1, 1.0 / 3.0, 0.999):
            qf = np.float64(np.float32(q))
            assert R.quantile(np.sort(v), q) == np.quantile(v, qf), (len(x), q)
        for norm in R.PARAMS[1:]:
            qa, qb = np.quantile(v, np.float64(np.float32(norm[1]))), np.quantile(v, np.float64(np.float32(norm[2])))
            assert R.stats(x, norm) == (qa + qb, qb - qa)


def test_empty_and_tiny_reads():
    for norm in R.PARAMS:
        assert R.stats(np.zeros(0, np.int16), norm) == (0.0, 0.0)
    assert R.stats(np.array([-7], np.int16), R.BONITO) == (-7.0, 0.0)
    assert R.stats(np.array([-7, 4], np.int16), R.BONITO) == (-1.5, 5.5)
    assert R.stats(np.array([65535, 0], np.uint16), R.BONITO) == (32767.5, 32767.5)


def test_constants():
    # Bonito: (x - med) / (1.4826 MAD); a constant read: scale_min
    shift, scale, off, inv = R.constants(-1.5, 5.5, R.BONITO)
    assert shift == np.float32(-1.5) and scale == np.float32(np.float32(1.4826).astype(np.float64) * 5.5)
    assert off == np.float32(1.5) and inv == np.float32(1.0 / np.float64(scale))
    shift, scale, _, inv = R.constants(0.0, 0.0, R.BONITO)
    assert scale == np.float32(R.FLT_MIN) and np.isfinite(inv)
    # Dorado: shift at least 10, scale at least 1
    shift, scale, _, _ = R.constants(4.0, 0.5, R.DORADO)
    assert shift == np.float32(10.0) and scale == np.float32(1.0)
