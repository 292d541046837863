"""CPU tests of tests/events_ref.py, the numpy statement of signal events: against a brute-force loop over each event's samples (moments
equal; mean and sd within float32 rounding of np.mean / np.std on float64 data), the clamping rules, constant events, the extremes."""
import numpy as np

import events_ref as EV

TO_END = 0xFFFFFFFF


def brute(x, starts, o, s):
    T = len(x)
    out = []
    for c, st in enumerate(starts):
        a = min(int(st), T)
        z = min(int(starts[c + 1]), T) if c + 1 < len(starts) else T
        v = [int(t) for t in x[a:z]]
        out.append((z - a, sum(v), sum(t * t for t in v), np.asarray(v, np.float64)))
    return out


def check(x, starts, o=0.0, s=1.0):
    n, S1, S2 = EV.moments(x, starts)
    mean, sd = EV.records(n, S1, S2, o, s)
    rows, mom = EV.event_rows(x, None, None, starts, o, s)
    assert rows.shape == (len(starts), 4) and mom.shape == (len(starts), 2) and mom.dtype == np.int64
    for c, (cnt, s1, s2, v) in enumerate(brute(x, starts, o, s)):
        assert (int(n[c]), int(S1[c]), int(S2[c])) == (cnt, s1, s2), (c, starts[c])
        assert (int(mom[c, 0]), int(mom[c, 1].view(np.uint64))) == (s1, s2)
        assert rows[c, 2] == cnt and rows[c, 3] == 0
        if cnt == 0:
            assert rows[c, 0] == 0 and rows[c, 1] == 0, "an empty event is +0 / +0"
            continue
        want_m = (v.mean() + np.float64(np.float32(o))) * np.float64(np.float32(s))
        want_s = v.std() * abs(np.float64(np.float32(s)))
        # mean: one float32 rounding (2^-24 relative) of a float64 value with three float64 roundings behind it.  sd: the same, and the
        # cancellation in S2/n - m^2 -- its terms are below max|x|^2 and carry 2^-53 relative each, so v is off by at most 3 * 2^-53 max^2
        # and sd = sqrt(v) by that over 2 sd; a constant event has v == 0 exactly
        assert abs(np.float64(mean[c]) - want_m) <= 2.0 ** -23 * abs(want_m), (c, mean[c], want_m)
        if want_s == 0.0:
            assert sd[c] == 0.0, (c, sd[c])
        else:
            vmax = max(float(abs(v).max()), 1.0) * abs(np.float64(np.float32(s)))
            assert abs(np.float64(sd[c]) - want_s) <= 2.0 ** -23 * want_s + 2.0 ** -51 * vmax * vmax / want_s, (c, sd[c], want_s)


def test_against_brute_force():
    rng = np.random.default_rng(1)
    for T in (0, 1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 4101):
        x = rng.integers(-32768, 32768, T).astype(np.int16)
        walk = np.clip(330 + rng.normal(0, 40, T), 80, 580).astype(np.int16)
        for starts in ([], [0], list(range(T)), sorted(rng.integers(0, T + 3, 40).tolist()), [5, 5, 9, T, T + 1, TO_END],
                       np.cumsum(rng.integers(1, 31, T // 15 + 1)).tolist()):
            check(x, starts, -3.5, 0.25)
            check(walk, starts, 12.0, -1.5)
            check(x.view(np.uint16), starts)


def test_clamping_rules():
    x = np.arange(10, dtype=np.int16)
    n, S1, S2 = EV.moments(x, [3, 3, 6, 10, 11, TO_END])
    assert n.tolist() == [0, 3, 4, 0, 0, 0]   # equal starts: an empty event; at or behind T: empty; samples 0 .. 2 belong to none
    assert S1.tolist() == [0, 3 + 4 + 5, 6 + 7 + 8 + 9, 0, 0, 0]
    n, S1, S2 = EV.moments(x, [4])
    assert n.tolist() == [6] and S1.tolist() == [sum(range(4, 10))]   # the last event runs to the end
    assert EV.moments(x, [])[0].tolist() == []
    rows, mom = EV.event_rows(x, 2, 8, [0, 4, 100], 0.0, 1.0)   # positions are the range's: samples 2 .. 7
    assert rows[:, 2].tolist() == [4, 2, 0] and mom[:, 0].tolist() == [2 + 3 + 4 + 5, 6 + 7, 0]


def test_constant_events_have_sd_zero_exactly():
    for val in (-32768, -1, 0, 1, 333, 32767):
        x = np.full(100, val, np.int16)
        n, S1, S2 = EV.moments(x, [0, 1, 8, 50])
        mean, sd = EV.records(n, S1, S2, 0.0, 1.0)
        assert (sd.view(np.uint32) == 0).all(), val
        assert (mean == np.float32(val)).all()
    x = np.full(100, 65535, np.uint16)
    n, S1, S2 = EV.moments(x, [0, 33])
    mean, sd = EV.records(n, S1, S2, 0.0, 1.0)
    assert (sd.view(np.uint32) == 0).all() and (mean == np.float32(65535)).all()


def test_extremes_do_not_wrap():
    x = np.full(70_000, -32768, np.int16)
    n, S1, S2 = EV.moments(x, [0])
    assert (int(n[0]), int(S1[0]), int(S2[0])) == (70_000, -32768 * 70_000, 32768 * 32768 * 70_000)
    u = np.full(70_000, 65535, np.uint16)
    n, S1, S2 = EV.moments(u, [0, 69_999])
    assert (int(S1[0]), int(S2[0])) == (65535 * 69_999, 65535 * 65535 * 69_999) and (int(S1[1]), int(S2[1])) == (65535, 65535 * 65535)
    mean, sd = EV.records(n, S1, S2, 0.0, 1.0)
    assert mean.tolist() == [65535.0, 65535.0] and sd.tolist() == [0.0, 0.0]
