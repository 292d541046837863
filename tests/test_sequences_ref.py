"""tests/sequences_ref.py held to a brute-force loop: runs_ref and period_ref over every byte string of a small alphabet, against a
statement that knows nothing of masks or openings -- a position is matched when some window of r consecutive positions that contains it
consists of positions equal to the byte d in front of them -- and a few cases written out by hand, RMIN - 1 and RMIN among them."""
import itertools

import numpy as np

import sequences_ref as S


def brute(x, d, r, begin=0, end=None, first_stays=True):
    """pairs and literals by definition.  Position p of x[begin : end] is marked when p - d >= 0 (p - d >= begin does not matter: the source
    may lie in front of the chunk) and x[p] == x[p - d]; it is matched when r consecutive marked positions inside [begin, end) contain it."""
    end = len(x) if end is None else end
    marked = [p - d >= 0 and x[p] == x[p - d] for p in range(len(x))]
    matched = []
    for p in range(begin, end):
        hit = False
        for w in range(p - r + 1, p + 1):   # the window [w, w + r)
            if w >= begin and w + r <= end and all(marked[w : w + r]):
                hit = True
        matched.append(hit)
    pairs, lits, ll, ml = [], [], 0, 0
    for p in range(begin, end):
        if matched[p - begin]:
            ml += 1
        else:
            if ml:
                pairs.append((ll, ml))
                ll = ml = 0
            ll += 1
            lits.append(x[p])
    if ml:
        pairs.append((ll, ml))
    return pairs, lits


def same(got, want):
    return got[0] == want[0] and got[1].tolist() == list(want[1])


def test_runs_ref_against_brute_force_small_minimum():
    # every string over {0, 1, 2} up to length 8 with a minimum run of 3 and 4: every arrangement of runs, gaps and back-to-back runs
    for rmin in (3, 4):
        for n in range(0, 9):
            for t in itertools.product(range(3), repeat=n):
                x = np.array(t, np.uint8)
                assert same(S.runs_ref(x, rmin), brute(list(t), 1, rmin - 1)), (rmin, t)


def test_runs_ref_against_brute_force_at_rmin():
    # the real minimum: every string over {0, 1} of RMIN - 1 ... RMIN + 1 bytes (a run needs RMIN of them)
    for n in range(S.RMIN - 1, S.RMIN + 2):
        for t in itertools.product(range(2), repeat=n):
            assert same(S.runs_ref(np.array(t, np.uint8)), brute(list(t), 1, S.RMIN - 1)), t


def test_period_ref_against_brute_force():
    # distances 1 ... 3, a minimum of 2 and 3, chunks [begin, end) that begin at every other position of every string over {0, 1} up to length 8
    for rper in (2, 3):
        for n in range(0, 9):
            for t in itertools.product(range(2), repeat=n):
                x = np.array(t, np.uint8)
                for D in (1, 2, 3):
                    for begin in range(0, n + 1, 2):
                        for end in (n, max(begin, n - 3)):
                            assert same(S.period_ref(x, begin, end, D, rper), brute(list(t), D, rper, begin, end)), (rper, t, D, begin, end)


def test_runs_ref_by_hand():
    R = S.RMIN
    z = lambda n, v=0: [v] * n
    cases = [
        ([], [], []),
        (z(R - 1), [], z(R - 1)),                                  # one short of a run: all literals
        (z(R), [(1, R - 1)], [0]),                                 # the shortest run: its first byte stays
        (z(R + 1), [(1, R)], [0]),
        ([9] + z(R), [(2, R - 1)], [9, 0]),
        ([9] + z(R - 1) + [9], [], [9] + z(R - 1) + [9]),
        (z(R) + [7], [(1, R - 1)], [0, 7]),                        # a tail literal
        (z(R, 5) + z(R, 6), [(1, R - 1), (1, R - 1)], [5, 6]),     # back to back, different values: two sequences, no gap
        (z(R, 0x55) + [1, 2] + z(40, 0xFF), [(1, R - 1), (3, 39)], [0x55, 1, 2, 0xFF]),
        (z(R - 1, 3) + z(R, 4), [(R, R - 1)], z(R - 1, 3) + [4]),  # a short run in front of a run: literals
        (z(300), [(1, 299)], [0]),
    ]
    for x, pairs, lits in cases:
        got = S.runs_ref(np.array(x, np.uint8))
        assert got[0] == pairs and got[1].tolist() == lits, (x, got)
    # the literal lengths are at least 1 whatever the bytes: a run's first byte has nothing equal in front of it
    rng = np.random.default_rng(1)
    for _ in range(200):
        x = np.repeat(rng.integers(0, 3, 40, dtype=np.uint8), rng.integers(1, 30, 40))
        pairs, lits = S.runs_ref(x)
        assert all(ll >= 1 and ml >= R - 1 for ll, ml in pairs)
        assert sum(ll + ml for ll, ml in pairs) + len(lits) - sum(ll for ll, _ in pairs) == len(x)


def test_period_ref_by_hand():
    P = S.RPER
    t = list(range(1, 41))                 # a template of 40 different bytes
    x = np.array(t * 3, np.uint8)
    assert S.period_ref(x, 0, 120, 40)[0] == [(40, 80)]
    assert S.period_ref(x, 0, 120, 40)[1].tolist() == t
    # a chunk that begins inside the repeat: nothing stands in front of it, its first position is matched from before the chunk
    assert S.period_ref(x, 48, 120, 40)[0] == [(0, 72)]
    assert S.period_ref(x, 0, 48, 40)[0] == []              # 8 marked positions: below RPER
    assert S.period_ref(x, 0, 40 + P, 40)[0] == [(40, P)]   # exactly RPER
    assert S.period_ref(x, 0, 40 + P - 1, 40)[0] == []
    y = x.copy()
    y[60] = 200                             # one changed byte: it and its copy 40 further on break the marks twice
    assert S.period_ref(y, 0, 120, 40)[0] == [(40, 20), (1, 39), (1, 19)]
    y[60 + P] = 201                         # a stretch of RPER - 1 marks between two changes stays literal
    pairs, lits = S.period_ref(y, 0, 120, 40)   # (and so do the 15 and 3 marks behind the copies of the two changes: a tail of 20)
    assert pairs == [(40, 20), (1 + P, 39 - P)] and len(lits) == 40 + 1 + P + 20


def test_checkpoints_ref_spacing_and_words():
    assert S.CP_MIN_SPACING == 32
    for nseq, spacing, count in ((1, 32, 0), (32, 32, 0), (33, 32, 1), (2048, 32, 63), (2049, 64, 32), (4096, 64, 63), (4097, 128, 32)):
        seqs = np.zeros(nseq, [("unread", "<i8"), ("ll_state", "<u2"), ("ml_state", "<u2")])
        seqs["unread"] = 100000 - 7 * np.arange(nseq)
        seqs["ll_state"] = np.arange(nseq) % 64
        seqs["ml_state"] = (np.arange(nseq) * 5) % 64
        sp, words = S.checkpoints_ref(seqs)
        assert (sp, len(words)) == (spacing, count), (nseq, sp, len(words))
        for j, w in enumerate(words):
            k = (j + 1) * spacing
            assert w == (100000 - 7 * k) | (k % 64) << 20 | ((5 * k) % 64) << 26


def test_key_spans_tile_the_region():
    for K in (1, 255, 256, S.KEYSPAN, S.KEYSPAN + 1, 20000, S.BLOCK_MAX):
        for shared in (False, True):
            spans = S.key_spans(K, shared)
            limit = S.KEYSPAN_SHARED if shared else S.KEYSPAN
            assert len(spans) == (K + limit - 1) // limit and spans[0][0] == 0 and spans[-1][1] == K
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and all(0 < e - b <= limit for b, e in spans)
