"""CPU tests of windows_ref: on the PAD grid the windows are the chunks of signal_ref, and a window outside the signal is pad."""
import numpy as np
import pytest

import ranges_ref as G
import signal_ref as SR
import windows_ref as W

PAD = -7.0


def signal(T, seed=3):
    return np.random.default_rng(seed).integers(-3000, 3000, T).astype(np.int16)


@pytest.mark.parametrize("T", [0, 1, 8, 9, 2049])
@pytest.mark.parametrize("L,S", [(8, 8), (16, 8), (1024, 1000)])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_pad_grid_is_the_chunk_rule(T, L, S, dtype):
    x = signal(T)
    starts, want = SR.chunk_rows(x, L, S, "pad", 0, 1.5, 0.25, PAD, dtype)
    assert starts == SR.chunk_starts(T, L, S, "pad", 0)
    got = W.window_rows(x, None, None, starts, L, 1.5, 0.25, PAD, dtype)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert (got == want).all()


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_windows_over_the_ends(dtype):
    x = signal(20)
    L = 8
    bits = SR.typed_bits(x, 0.0, 1.0, dtype)
    p = SR.pad_bits(PAD, dtype)
    got = W.window_rows(x, None, None, [-8, -3, 0, 0, 15, 19, 20, 25, -100], L, 0.0, 1.0, PAD, dtype)
    assert (got[0] == p).all() and (got[6] == p).all() and (got[7] == p).all() and (got[8] == p).all()
    assert (got[1][:3] == p).all() and (got[1][3:] == bits[:5]).all()
    assert (got[2] == bits[:8]).all() and (got[3] == got[2]).all()
    assert (got[4][:5] == bits[15:]).all() and (got[4][5:] == p).all()
    assert got[5][0] == bits[19] and (got[5][1:] == p).all()


def test_range_and_empty_signal():
    x = signal(40)
    got = W.window_rows(x, 8, 24, [-2, 10], 8, 0.0, 1.0, PAD, "f16")
    bits = SR.typed_bits(x[8:24], 0.0, 1.0, "f16")
    p = SR.pad_bits(PAD, "f16")
    assert (got[0][:2] == p).all() and (got[0][2:] == bits[:6]).all()
    assert (got[1][:6] == bits[10:]).all() and (got[1][6:] == p).all()
    for xs, b, e in ((x[:0], None, None), (x, 30, 10), (x, 40, G.TO_END)):
        rows = W.window_rows(xs, b, e, [0, -3, 5], 16, 2.0, 3.0, PAD, "f32")
        assert rows.shape == (3, 16) and (rows == SR.pad_bits(PAD, "f32")).all()
    assert W.window_rows(x, None, None, [], 8, 0.0, 1.0, PAD, "bf16").shape == (0, 8)


def test_norm_rows_use_the_statistics_of_range_or_read():
    import norm_ref as R

    x = signal(500, 9)
    for stats in (G.STATS_RANGE, G.STATS_READ):
        rows, shift, scale = W.norm_window_rows(x, 100, 300, [0, 50], 64, R.BONITO, stats, PAD, "f32")
        sh, sc, o, s = G.shift_scale(x, 100, 300, R.BONITO, stats)
        assert (shift, scale) == (sh, sc)
        assert (rows == W.window_rows(x, 100, 300, [0, 50], 64, o, s, PAD, "f32")).all()
