"""CPU tests of the numpy statements in eventalign_ref (the rules of vbz_gpu_events_query_batch and vbz_gpu_locate_levels_batch): held to
plain Python loops over a few thousand random small cases, to paths of locate_path_ref as well as planted ones, to the agreement of
direct sums and prefix differences under wrap-around; and the catalogues the tests on the MI355X run are counted."""
import numpy as np

import eventalign_ref as E
import locate_path_ref as LP


def query_loops(first, event_rows, mean, n, N, min_n, result):
    out = []
    for i in range(len(first) - 1):
        q, ix, kept = [0] * N, [0] * N, 0
        c0, c1 = int(first[i]), int(first[i + 1])
        good = c0 <= c1 and c1 <= event_rows and c1 - c0 <= E.MAX_ROWS and not (result is not None and int(result[i]) >= E.E_FIRST)
        if good:
            for c in range(c0, c1):
                if kept == N:
                    break
                if int(n[c]) >= min_n:
                    q[kept], ix[kept] = int(mean[c]), c - c0
                    kept += 1
        out.append((q, kept, ix))
    return out


def test_events_query_against_loops():
    rng = np.random.default_rng(11)
    refused = kept_all = cut = 0
    for case in range(1500):
        reads = int(rng.integers(1, 6))
        rows = rng.integers(0, 40, reads)
        first = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint64)
        total = int(first[-1])
        event_rows = total
        if case % 7 == 0:   # a bad table
            i = int(rng.integers(1, reads + 1))
            kind = int(rng.integers(0, 4))
            first[i] = [0, total + 1, int(first[i - 1]) + (1 << 31), 1 << 40][kind]
            event_rows = 1 << 41 if kind == 2 and i == reads else total   # (declared rows beyond the arrays: only behind a read of 2^31 rows)
        mean, n = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32), rng.integers(0, 5, total).astype(np.uint32)
        N, min_n = int(rng.choice([8, 16, 24])), int(rng.integers(0, 5))
        result = None if case % 3 else rng.choice([0, 64, E.E_FIRST - 1, E.E_FIRST, 0xFFFFFFFF], reads).astype(np.uint32)
        # (no row of a refused read is touched: the arrays end at `total` whatever the table says)
        query, valid, index = E.events_query(first, event_rows, mean, n, N, min_n, result)
        for i, (q, kept, ix) in enumerate(query_loops(first, event_rows, mean, n, N, min_n, result)):
            assert query[i].tolist() == q and int(valid[i]) == kept and index[i].tolist() == ix, (case, i)
            own = E.read_rows(first, event_rows, i)
            refused += own is None
            if own is not None and own[1]:
                kept_all += kept == own[1]
                cut += kept == N
    assert refused > 100 and kept_all > 300 and cut > 300, (refused, kept_all, cut)


def levels_loops(c):
    """the rule, entry by entry: every entry adds itself to each of its levels"""
    pairs, hit, rows, index, first, event_rows, start, n, moments, n_reads = c.arrays()
    out = []
    for p in range(len(pairs)):
        ev = E.pair_events(pairs[p], hit[p], rows[p], index, first, event_rows, n_reads, c.N, c.W)
        if ev is None:
            out.append(None)
            continue
        s, e = int(hit[p][2]), int(hit[p][1])
        rec = [None] * (e - s)
        for k, cc in enumerate(ev.tolist()):
            for j in range(int(rows[p][k][0]), int(rows[p][k][1])):
                st, nn, s1, s2 = int(start[cc]), int(n[cc]), int(moments[cc][0]), int(moments[cc][1])
                if rec[j - s] is None:
                    rec[j - s] = [st, 0, 0, 0, 0, 0]
                r = rec[j - s]
                r[1], r[2], r[3], r[4], r[5] = (st + nn) % (1 << 32), (r[2] + nn) % (1 << 32), r[3] + 1, (r[4] + s1) % (1 << 64), (r[5] + s2) % (1 << 64)
        out.append(rec)
    return out


def held_to_loops(c):
    n_levels, lv = c.expected()
    direct = c.expected(direct=True)
    assert (direct[0] == n_levels).all() and (direct[1] == lv).all(), c.name
    for p, rec in enumerate(levels_loops(c)):
        if rec is None:
            assert n_levels[p] == 0 and not lv[p].any(), (c.name, p)
            continue
        assert n_levels[p] == len(rec) and not lv[p, len(rec):].any(), (c.name, p)
        got = lv[p, :len(rec)].astype(np.uint64)
        words = np.stack([got[:, 0], got[:, 1], got[:, 2], got[:, 3], got[:, 4] | got[:, 5] << np.uint64(32), got[:, 6] | got[:, 7] << np.uint64(32)], 1)
        assert words.tolist() == rec, (c.name, p)


def test_levels_against_loops_on_planted_paths():
    rng = np.random.default_rng(12)
    stalls = skips = 0
    for case in range(400):
        c = E.LevelsCall("random %u" % case, 24, 40)
        for _ in range(int(rng.integers(1, 6))):
            n = int(rng.integers(1, 25))
            path = E.random_path(rng, n, int(rng.integers(1, 41)), int(rng.integers(0, 9)))
            assert E.path_ok(path, n, int(path[0, 0]), int(path[-1, 1]))
            a, b = E.shape_counts(path)
            stalls, skips = stalls + (a > 0), skips + (b > 0)
            c.plant(rng, path, gaps=bool(rng.integers(0, 2)), moments=str(rng.choice(["small", "2^46", "wrap"])), dwell=int(rng.choice([3, 30, 1 << 31])))
        c.use_index = bool(case % 4)
        held_to_loops(c)
    assert stalls > 500 and skips > 500, (stalls, skips)


def test_levels_on_paths_of_the_locate_rule():
    """the paths locate_path_ref traces, as vbz_gpu_locate_path_batch would leave them"""
    rng = np.random.default_rng(13)
    N, G, L = 24, 2, 80
    covered = 0
    for case in range(40):
        query = rng.normal(0, 1.5, (5, N)).astype(np.float32)
        target = rng.integers(-90, 91, (G, L)).astype(np.int8)
        valid = rng.integers(0, N + 1, 5)
        pairs = [(int(rng.integers(0, 5)), int(rng.integers(0, G)), int(a), int(a + rng.integers(1, 48))) for a in rng.integers(0, 32, 6)] + [(0, LP.NONE, 0, 0)]
        hit, rows = LP.paths(query, valid, 32.0, target, [L, L - 7], pairs, 48)
        c = E.LevelsCall("locate %u" % case, N, 48)
        for r in range(5):
            c.add_read(rng, N + 3, N, gaps=True, moments="wrap")
        c.pairs, c.hit, c.rows = [tuple(p) for p in pairs], [tuple(h) for h in hit.tolist()], list(rows)
        n_levels, lv = c.expected()
        for p in range(len(pairs)):
            empty = hit[p].tolist() == list(E.EMPTY_HIT)
            assert (n_levels[p] == 0) == empty and (empty or n_levels[p] == hit[p][1] - hit[p][2]), (case, p)
            if not empty:
                assert lv[p, :n_levels[p], 3].sum() >= max(int(hit[p][3]), int(n_levels[p])) and (lv[p, :n_levels[p], 3] >= 1).all()
                covered += 1
        held_to_loops(c)
    assert covered > 100, covered


def test_direct_sums_and_prefix_differences_agree_under_wrap():
    for c in E.levels_tables():
        a, b = c.expected(), c.expected(direct=True)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), c.name
    wrapped = 0
    c = [c for c in E.levels_tables() if c.name == "running totals pass 2^64"][0]
    pairs, hit, rows, index, first, event_rows, start, n, moments, n_reads = c.arrays()
    for p in range(len(pairs)):
        ev = E.pair_events(pairs[p], hit[p], rows[p], index, first, event_rows, n_reads, c.N, c.W)
        wrapped += sum(int(v) for v in moments[ev, 1]) >= 1 << 64
    assert wrapped >= 5, wrapped
    big = [c for c in E.levels_tables() if c.name == "n sums pass 2^32"][0]
    assert sum(big.ev_n) >= 1 << 32


def test_the_catalogues():
    stalls = skips = pairs = longest_stall = longest_skip = 0
    sizes = set()
    for c in E.levels_catalogue():
        held = c.expected()
        assert (held[0] > 0).all(), c.name
        assert c.N % 8 == 0 and c.W % 8 == 0
        for p, h in enumerate(c.hit):
            path = c.rows[p][:h[3]].astype(np.int64)
            a, b = E.shape_counts(path)
            stalls, skips, pairs = stalls + (a > 0), skips + (b > 0), pairs + 1
            sizes.add(h[3])
            longest_skip = max(longest_skip, int((path[:, 1] - path[:, 0]).max()))
            longest_stall = max(longest_stall, int(held[1][p, :, 3].max()))
    assert set(range(1, 137)) | {255, 256, 257, 2047, 2048} <= sizes
    assert pairs > 300 and stalls > 200 and skips > 150 and longest_stall == 2048 and longest_skip >= 300, (pairs, stalls, skips, longest_stall, longest_skip)
    for c in E.levels_shapes()[-1:]:   # the stall begins at every residue of a 64-entry turn
        begins = {int(np.flatnonzero(c.rows[p][1:c.hit[p][3], 0] == c.rows[p][:c.hit[p][3] - 1, 1] - 1)[0]) % 64 for p in range(len(c.pairs))}
        assert begins == set(range(64))
    for name in E.BROKEN:   # a refused table: the one broken pair, wherever it stands
        for at in (0, 2, 4):
            c, p = E.levels_broken(name, at)
            n_levels, lv = c.expected()
            assert n_levels[p] == 0 and not lv[p].any() and (np.delete(n_levels, p) > 0).all(), (name, at, n_levels)
    assert len(E.BROKEN) == 26
    dropped = refused = full = 0
    for c in E.query_catalogue():
        query, valid, index = c.expected()
        for i in range(len(valid)):
            own = E.read_rows(c.first, c.event_rows, i)
            refused += own is None
            dropped += own is not None and valid[i] < min(own[1], c.N)
            full += valid[i] == c.N
            assert not query[i, valid[i]:].any() and not index[i, valid[i]:].any()
    assert dropped > 60 and refused == 5 and full > 60, (dropped, refused, full)
