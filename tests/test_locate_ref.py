"""CPU tests of the numpy statement of the signal-locate rule (tests/locate_ref.py; include/vbz_gpu.h: vbz_gpu_locate): against the defining
triple loop on random small pairs with -128 in the targets, the swap identity against match_ref.hits, the planted answers of the
catalogue, and a count of the catalogue's pairs by rows per lane."""
import collections

import numpy as np

import locate_ref as LR
import match_ref as M


def test_statement_against_the_triple_loop():
    rng = np.random.default_rng(77)
    for _ in range(300):
        n, L = int(rng.integers(1, 24)), int(rng.integers(1, 40))
        levels = rng.integers(-127, 128, n)
        target = rng.integers(-128, 128, L)
        target[rng.integers(0, L)] = -128
        # rows the query, columns the target: dtw_brute's `ref` is the sequence aligned whole
        assert LR.locate(levels, target) == M.dtw_brute(levels, target), (levels.tolist(), target.tolist())
    assert LR.locate([], [1, 2]) == LR.EMPTY and LR.locate([1], []) == LR.EMPTY


def test_swap_identity_against_match_hits():
    """hits(query, valid, target, target_len)[i][g] == match_ref.hits(target as the query, target_len, levels as references, n)[g][i] for
    targets without -128 (the match rule clamps its query to +-127)"""
    rng = np.random.default_rng(78)
    N, stride = 48, 96
    query = (rng.integers(-127, 128, (9, N)) / 32.0).astype(np.float32)
    query[3, 5] = np.nan
    valid = np.array([48, 1, 17, 48, 0, 33, 500, 0xFFFFFFFF, 2], np.uint64)
    target = rng.integers(-127, 128, (7, stride)).astype(np.int8)
    target_len = np.array([96, 1, 40, 0, 97, 0xFFFFFFFF, 64], np.uint64)
    got = LR.hits(query, valid, 32.0, target, target_len)
    levels = M.quantize(query, 32.0)
    n = np.minimum(valid, N)
    tvalid = np.where((target_len != 0) & (target_len <= stride), target_len, 0)
    want = M.hits(target.astype(np.float32) / np.float32(32.0), tvalid, 32.0, levels, n)
    assert (got == want.transpose(1, 0, 2)).all()
    assert (got[4] == np.array(LR.EMPTY, np.uint32)).all() and (got[:, 3] == np.array(LR.EMPTY, np.uint32)).all()
    assert (got[:, 4] == np.array(LR.EMPTY, np.uint32)).all() and (got[:, 5] == np.array(LR.EMPTY, np.uint32)).all()
    assert got[0][0].tolist() != list(LR.EMPTY)


def test_planted_answers():
    seen = 0
    for index, call in enumerate(LR.catalogue()):
        if not call.planted:
            continue
        query, valid, target, target_len = call.arrays()
        for (read, tg), hit in call.planted.items():
            got = LR.hits(query[read : read + 1], valid[read : read + 1], call.quant, target[tg : tg + 1], target_len[tg : tg + 1])[0][0]
            assert tuple(int(v) for v in got) == hit, (call.name, read, tg, got.tolist(), hit)
            seen += 1
    assert seen == 15 + 3 + 1
    long = LR.catalogue()[-1]
    assert long.name == "long" and long.target_len == [LR.LONG_L] and LR.LONG_L > 65536 and list(long.planted.values()) == [(0, LR.LONG_END)]
    assert LR.LONG_END > 65536 and (long.arrays()[2][0, LR.LONG_L :] != 0).all()


def test_catalogue_reaches_every_instantiation():
    by_c = collections.Counter()
    ns, Ls = set(), set()
    for call in LR.catalogue():
        assert call.N % 8 == 0 and 8 <= call.N <= 2048 and call.stride % 16 == 0
        for n, L in call.pairs():
            by_c[LR.rows_per_lane(n)] += 1
            ns.add(n)
            Ls.add(L)
    assert sorted(by_c) == list(LR.ROWS) and all(by_c[c] >= 20 for c in LR.ROWS), by_c
    assert set(LR.LENGTHS_N) - {0} <= ns and set(LR.LENGTHS_L) <= Ls
    a = LR.catalogue()[0]
    assert 0 in a.valid and 5000 in a.valid and 0xFFFFFFFF in a.valid
    assert {0, a.stride + 1, 0xFFFFFFFF} <= set(a.target_len)
    assert any((t[:L] == -128).any() for t, L in zip(a.targets, a.target_len) if 0 < L <= a.stride)
    # pairs shorter than the pipeline: L below the lane of the query's last row
    assert any(L < (n - 1) // LR.rows_per_lane(n) for n, L in a.pairs())
