"""CPU test of tests/match_sweep.py: the restated dispatch of csrc/match.hip against the headers' own examples, the census of the loops
the catalogues reach -- the existing ones alone and together with the sweep (pytest -s prints both tables; DESIGN.md 4.22 holds them) --
and the sweep's calls checked against themselves: garbage behind the ends moves no answer, the planted answers are match_span_ref's and
match_path_ref's."""
import numpy as np

import match_path_ref as P
import match_sweep as W


# ---- the restated rule ------------------------------------------------------------------------------------------------------------------------
def test_rows_per_lane_and_the_packed_rule_are_the_headers():
    assert [W.rows_per_lane(m) for m in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32]
    assert [W.start_bits(n) for n in (1, 2, 3, 136, 256, 257, 4096, 4097, 65536)] == [0, 1, 2, 8, 8, 9, 12, 13, 16]
    # match_select.h and DESIGN.md 4.22: stride 2 048 is packed up to N = 4 096, 400 up to 16 384, 128 up to 65 536; the next N or stride up is wide
    for N, stride in ((4096, 2048), (16384, 400), (65536, 128)):
        assert W.packed(N, stride) and W.packed(N - 8, stride) and not W.packed(N + 8, stride), (N, stride)
    assert not W.packed(4096, 2064) and not W.packed(65536, 144) and W.packed(16384, 512) and not W.packed(16384, 528) and W.packed(8, 2048)
    assert W.instantiation("cost", 4096, 2048, 300) == (W.COST, 8, None)
    assert W.instantiation("span", 4096, 2048, 300) == (W.SPAN, 8, 3) and W.instantiation("span", 8192, 2048, 300) == (W.SPAN_WIDE, 8, 7)
    assert W.instantiation("path", 4096, 2048, 2048) == (W.PATH, 32, None) and W.instantiation("path", 32776, 144, 1) == (W.PATH_WIDE, 1, None)


def test_the_sweeps_shapes_run_the_kernels_they_are_meant_for():
    assert W.packed(W.DENSE_N, W.DENSE_STRIDE) and W.start_bits(W.DENSE_N) == 8 and not W.packed(W.DENSE_WIDE_N, W.DENSE_STRIDE)
    assert W.packed(W.EVERY_N, W.EVERY_STRIDE) and not W.packed(W.EVERY_WIDE_N, W.EVERY_STRIDE)
    assert W.packed(W.PATHS_WIDTH, W.DENSE_STRIDE) and not W.packed(W.PATHS_WIDE, W.DENSE_STRIDE) and W.packed(W.PATHS_WIDE - 8, W.DENSE_STRIDE)
    assert W.packed(W.CLASS_N, W.CLASS_STRIDE) and not W.packed(W.CLASS_WIDE_N, W.CLASS_STRIDE)
    assert W.packed(W.STRETCH_N, W.STRETCH_STRIDE) and not W.packed(W.STRETCH_WIDE_N, W.STRETCH_STRIDE)
    for sb, (N, stride) in zip((12, 13, 14, 15, 16), W.BOUND):   # each the largest packed stride of its sb
        assert W.start_bits(N) == sb and W.packed(N, stride) and not W.packed(N, stride + 16), (N, stride)
        wN, ws = W.bound_wide(N, stride)
        assert not W.packed(wN, ws) and wN % 8 == 0 and ws % 16 == 0 and ws <= 2048 and wN <= 65536, (N, stride)


# ---- the census -------------------------------------------------------------------------------------------------------------------------------
def _table(cen, runs):
    """the rows of the printed table: what is reached of every family of loops"""
    rows = [("match_kernel: C", sorted(c for k, c, _ in cen if k == W.COST), 6)]
    for c in W.CS:
        rows.append(("packed span: SEL of C = %d" % c, sorted(s for k, cc, s in cen if k == W.SPAN and cc == c), c))
    rows.append(("packed span: (C, SEL)", sorted((c, s) for k, c, s in cen if k == W.SPAN), 63))
    for name, k in (("wide span: C", W.SPAN_WIDE), ("packed path: C", W.PATH), ("wide path: C", W.PATH_WIDE)):
        rows.append((name, sorted(c for kk, c, _ in cen if kk == k), 6))
    for name, k in (("packed path: C with a refetch inside a lane", W.PATH), ("wide path: C with a refetch inside a lane", W.PATH_WIDE)):
        rows.append((name, sorted(c for (kk, c), run in runs.items() if kk == k and run * c > 1024 + 16), 6))
    return rows


def _existing_runs():
    runs = {}
    for i, pc in enumerate(P.catalogue()):
        for key, run in W.long_runs(pc, P.expected(i)[1]).items():
            runs[key] = max(runs.get(key, 0), run)
    return runs


def _merge(a, b):
    out = {k: set(v) for k, v in a.items()}
    for k, v in b.items():
        out.setdefault(k, set()).update(v)
    return out


def test_census_of_the_existing_catalogues_beside_the_union():
    """Prints (pytest -s) what the catalogues reached before the sweep and what they reach with it, and asserts the union: every C of
    match_kernel, all 63 (C, SEL) of the packed span kernel, every C of the wide span kernel and of both path forward kernels, and for
    every C and both keys a path that stays on one reference row for more than (1 024 + 16) / C columns"""
    old, old_runs = W.census(W.existing_shapes()), _existing_runs()
    new_runs = W.sweep_long_runs()
    both = _merge(old, W.census(W.sweep_shapes()))
    both_runs = {k: max(old_runs.get(k, 0), new_runs.get(k, 0)) for k in set(old_runs) | set(new_runs)}
    before, after = _table(old, old_runs), _table(both, both_runs)
    print("\n%-46s %-22s %s" % ("loops of match.hip reached", "existing catalogues", "with the sweep"))
    for (name, a, of), (_, b, _) in zip(before, after):
        short = lambda v: "%d / %d" % (len(v), of) + ("  " + str(v) if 0 < len(v) < of and of <= 32 and len(v) <= 8 else "")
        print("%-46s %-22s %s" % (name, short(a), short(b)))
    for name, reached, of in after:
        assert len(reached) == of, (name, reached)
    # what the gap was: the stage-entry catalogues and the fused calls together
    gap = dict((name, len(reached)) for name, reached, _ in before)
    assert gap["packed span: (C, SEL)"] < 63 and gap["wide span: C"] < 6 and gap["wide path: C"] < 6, gap


def test_the_sweep_alone_reaches_what_it_was_built_for():
    cen = W.census(W.sweep_shapes())
    assert sorted((c, s) for k, c, s in cen if k == W.SPAN) == [(c, s) for c in W.CS for s in range(c)]
    for k in (W.COST, W.SPAN_WIDE, W.PATH, W.PATH_WIDE):
        assert sorted(c for kk, c, _ in cen if kk == k) == list(W.CS), k
    # the wide span kernel tracks the lane's last row, which is a true row for M = 0 mod C alone (behind the reference's end the rows are
    # free and every one of them holds the answer): each C needs such an M, and one that is not
    wide = [(W.rows_per_lane(m), m) for s in W.sweep_shapes() if s.kind == "span" and not W.packed(s.N, s.stride) for _, m in s.pairs]
    for c in W.CS:
        assert any(cc == c and m % c == 0 for cc, m in wide) and (c == 1 or any(cc == c and m % c != 0 for cc, m in wide)), c
    runs = W.sweep_long_runs()
    for k in (W.PATH, W.PATH_WIDE):
        for c in W.CS:
            assert runs[(k, c)] == W.stretch_length(c) and runs[(k, c)] * c > 1024 + 16, (k, c, runs.get((k, c)))


def _steps(cen, kernel, c):
    out = set()
    for (k, cc, _), steps in cen.items():
        if k == kernel and cc == c:
            out |= steps
    return out


def test_step_residues_of_the_dense_calls():
    """steps = n + la decides the systolic loop's tails (the odd last step, the last block of fewer than 64) and the path pass's open
    word (steps mod 16 / C).  C = 1, 2, 4: the dense calls meet every residue.  C = 8, 16, 32: both parities and both sides of a block"""
    dense = W.census(W.dense_shapes())
    for c in (1, 2, 4):
        for k in (W.COST, W.SPAN, W.SPAN_WIDE):
            assert {s % 64 for s in _steps(dense, k, c)} == set(range(64)), (k, c)
        for k in (W.PATH, W.PATH_WIDE):
            assert {s % (16 // c) for s in _steps(dense, k, c)} == set(range(16 // c)), (k, c)
            assert {s % 2 for s in _steps(dense, k, c)} == {0, 1}, (k, c)
    every = W.census(W.sweep_shapes())
    for c in (8, 16, 32):
        for k in (W.COST, W.SPAN, W.SPAN_WIDE, W.PATH, W.PATH_WIDE):
            steps = _steps(every, k, c)
            assert {s % 2 for s in steps} == {0, 1} and {0, 1} <= {s % 64 for s in steps}, (k, c)
    # ... and of every one of the packed span kernel's 63 loops: both parities
    for (k, c, sel), steps in every.items():
        if k == W.SPAN:
            assert {s % 2 for s in steps} == {0, 1}, (c, sel)


# ---- the calls ----------------------------------------------------------------------------------------------------------------------------------
def test_the_existing_catalogues_hold_none_of_the_sweeps_lengths():
    lengths = W.every_lengths()
    assert len(lengths) == 63 and len(set(lengths)) == 63 and not set(lengths) & W.existing_lengths()
    assert sorted((W.rows_per_lane(m), (m - 1) % W.rows_per_lane(m)) for m in lengths) == [(c, s) for c in W.CS for s in range(c)]
    for m in lengths:   # the upper half of the class
        c = W.rows_per_lane(m)
        assert (m - 1) // c >= (32 if c == 1 else 48), m
    b = W.every()
    assert [min(int(v), b.N) for v in b.valid] == list(W.EVERY_READS) and (b.N, b.quant, b.stride) == (256, 32.0, 2048)


def test_garbage_behind_the_ends_moves_no_answer():
    """A with NaN, infinities, +-1e30 and levels behind every read's end and random int8 (-128 among them) behind every reference's end
    against A padded with zeros: the same spans, and the hits are the spans' first two words"""
    g, z = W.dense(), W.dense(False)
    gq, gv, gr, gl = g.arrays()
    zq, zv, zr, zl = z.arrays()
    assert (gv == zv).all() and (gl == zl).all() and gv.tolist() == list(range(1, 137)) and gl.tolist() == list(range(1, 137))
    for i, n in enumerate(gv.tolist()):
        assert (gq[i, :n] == zq[i, :n]).all() and not zq[i, n:].any(), i
        assert (gr[i, : gl[i]] == zr[i, : gl[i]]).all() and not zr[i, gl[i] :].any() and (gr[i, gl[i] :] == -128).any(), i
    tail = np.concatenate([gq[i, n:] for i, n in enumerate(gv.tolist())])
    assert np.isnan(tail).any() and np.isposinf(tail).any() and np.isneginf(tail).any() and (np.abs(tail) == np.float32(1e30)).any() and (tail == 3.0).any()
    assert (W.dense_spans() == W.dense_spans(False)).all()
    assert (W.dense_hits() == W.dense_spans()[:, :, :2]).all()
    assert (W.dense_spans()[:, :, 0] != 0xFFFFFFFF).all()
    # alphabets: odd n and M draw from three levels, even ones from signal
    assert set(np.unique(zq[134, :135]).tolist()) <= {-1.0, 0.0, 1.0} and len(np.unique(zq[135])) > 8 and set(np.unique(zr[134, :135]).tolist()) <= {-1, 0, 1}


def test_dense_paths_cover_every_length_and_width():
    pc = W.dense_paths()
    assert len(pc.pairs) == 136 * 34 and pc.max_width == 40 and (pc.call.N, pc.call.stride) == (136, 144)
    assert {(int(pc.call.ref_len[rf]), b - a) for _, rf, a, b in pc.pairs} == {(m, w) for m in range(1, 137) for w in range(1, 35)}
    assert len(W.path_pairs(pc)) == len(pc.pairs) and {rd for rd, *_ in pc.pairs} == {0, 1} and pc.call.valid == [136, 135]
    assert len({a % 8 for _, _, a, _ in pc.pairs}) == 8
    wide = W.dense_paths_wide()
    pick = W.dense_paths_wide_pick()
    assert len(wide.pairs) == len(pick) <= 256 and {int(wide.call.ref_len[rf]) for _, rf, _, _ in wide.pairs} == set(range(1, 137))
    assert (wide.call.N, wide.max_width, wide.call.stride) == (32776, 32776, 144) and len(W.path_pairs(wide)) == len(pick)
    assert W.match_path_pair_bytes(wide.max_width, wide.call.stride) * len(pick) < 1 << 30
    q, v, r, l = wide.call.arrays()
    pq, pv, pr, pl = pc.call.arrays()
    assert (v == pv).all() and (l == pl).all() and all((q[i, :n] == pq[i, :n]).all() for i, n in enumerate(v.tolist()))


def test_paths_per_class():
    for wide in (False, True):
        pc = W.class_paths(wide)
        lens = [int(m) for m in pc.call.ref_len]
        assert [W.rows_per_lane(m) for m in lens] == [2, 2, 4, 4, 8, 8, 16, 16, 32, 32] and lens[0::2] == [128, 256, 512, 1024, 2048]
        assert not set(lens[1::2]) & (W.existing_lengths() | set(W.every_lengths()) | set(lens[0::2]))
        assert len(pc.pairs) == 80 == len(W.path_pairs(pc)) and {b - a for _, _, a, b in pc.pairs} == set(W.CLASS_WIDTHS)
        assert pc.max_width == pc.call.N == (8192 if wide else 256) and pc.call.stride == 2048
    assert W.class_paths(True).pairs == W.class_paths().pairs
    assert (W.class_paths_expected()[0][:, 0] != P.EMPTY[0]).all()


def test_stretched_copies_hold_one_row_for_the_stretch():
    """cost 0, row i0 holds L = 1 024 / C + 24 columns, every other row one: match_path_ref's answer is the planted one"""
    pc, what = W.stretched()
    hit, rows = W.stretched_expected()
    assert len(pc.pairs) == 13 == len(what) and pc.max_width == pc.call.N == 1728 and pc.call.stride == 2048
    assert sorted({L for _, L in what}) == [56, 88, 152, 280, 536, 1048]
    firsts, lasts = 0, 0
    for p, ((rd, rf, a, b), (i0, L)) in enumerate(zip(pc.pairs, what)):
        m = int(pc.call.ref_len[rf])
        c = W.rows_per_lane(m)
        assert L == W.stretch_length(c) and a == 0 and b == W.STRETCH_BG + m + L - 1
        assert hit[p].tolist() == [0, b, W.STRETCH_BG, m], (p, hit[p].tolist())
        width = (rows[p, :m, 1].astype(np.int64) - rows[p, :m, 0]).tolist()
        assert width == [L if i == i0 else 1 for i in range(m)], (p, m, i0)
        firsts += i0 % c == 0
        lasts += i0 % c == c - 1
    assert firsts >= 7 and lasts >= 7
    assert [int(pc.call.ref_len[rf]) for _, rf, _, _ in pc.pairs][-2:] == [1, 64] and what[-2][0] == 0 and what[-1][0] == 63
    wide, wwhat = W.stretched(True)
    assert wwhat == what and wide.pairs == pc.pairs and wide.max_width == wide.call.N == 8192


def test_the_bound_is_met_with_both_fields_full():
    for i, (N, stride) in enumerate(W.BOUND):
        f = W.bound(i)
        spans = W.bound_spans(i)
        assert spans.shape == (1, 1, 4) and spans[0][0].tolist() == [254 * stride, N, N - 1, 0] == list(f.planted[(0, 0)]) + [0]
        sb = W.start_bits(N)
        assert (254 * stride) >> (31 - sb - 1) == 1 and N - 1 == (1 << sb) - 1   # the cost field's top bit is set, the start field is all ones
        pc, (hit, rows) = W.bound_paths(i)
        assert hit.tolist() == [[254 * stride, N, N - 1, stride]] and (rows[0] == np.array([N - 1, N], np.uint32)).all()


def test_every_span_of_the_dense_call_is_a_window():
    pc, want = W.dense_windows()
    assert len(pc.pairs) == 136 * 136 == len(W.path_pairs(pc)) and pc.max_width == 136
    assert all(a < b for _, _, a, b in pc.pairs)
    # on the host, a thinned sample: the path over (start, end) of a span gives the span's cost and start
    query, valid, ref, ref_len = pc.call.arrays()
    some = list(range(0, len(pc.pairs), 97))
    hit, _ = P.paths(query, valid, pc.call.quant, ref, ref_len, [pc.pairs[p] for p in some], pc.max_width)
    assert (hit == want[some]).all()
