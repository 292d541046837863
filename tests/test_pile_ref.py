"""CPU tests of tests/pile_ref.py, the numpy statements of the four pile-up rules: each against plain Python loops, Python integers and Python
floats (a Python float is an IEEE double and every operation on it rounds once, to nearest even: the rule's own arithmetic), the count
word's two halves, u = +-2^24 kept and the next representable w beyond it skipped, pile_kmers of a position pile against a direct per-k-mer
pile of the levels, and the catalogues counted."""
import math
import struct

import numpy as np

import pile_ref as P
import squiggle_ref as R

M64 = (1 << 64) - 1


def f32(bits):
    return struct.unpack("<f", struct.pack("<I", int(bits)))[0]


def to_f32_bits(x):
    try:
        return struct.unpack("<I", struct.pack("<f", x))[0]
    except OverflowError:
        return 0x7F800000 if x > 0 else 0xFF800000


def plain_levels_pile(call):
    pairs, hit, n_levels, levels, n_reads, fit = call.arrays()
    T, G = call.T, len(call.target_len)
    pile = [[0] * (G * T) for _ in range(4)] if call.before is None or call.flags & P.CLEAR else [[int(v) for v in plane] for plane in call.before]
    for p in range(len(pairs)):
        read, ref, end, start, W = int(pairs[p][0]), int(pairs[p][1]), int(hit[p][1]), int(hit[p][2]), int(n_levels[p])
        if read >= n_reads or ref >= G or W == 0 or W > call.W or end - start != W or end < start:
            continue
        Lg = int(call.target_len[ref])
        if Lg == 0 or Lg > T or end > Lg:
            continue
        o, s = 0.0, 1.0
        if fit is not None:
            if call.flags & P.REQUIRE_OK and int(fit[p][3]) == 0:
                continue
            o, s = f32(fit[p][0]), f32(fit[p][1])
        for t in range(W):
            rec = [int(v) for v in levels[p, t]]
            ns, ne, total = rec[2], rec[3], rec[4] | rec[5] << 32
            total -= (1 << 64) if total >> 63 else 0
            c = ref * T + start + t
            skip = ns < max(call.min_samples, 1) or (call.max_entries != 0 and ne > call.max_entries)
            if not skip:
                w = ((float(total) / float(ns) + o) * s) * f32(to_f32_bits(call.fix))
                skip = not (abs(w) <= 2.0 ** 24)
            if skip:
                pile[0][c] = (pile[0][c] + (1 << 32)) & M64
                continue
            u = int(round(w))   # (Python's round: to nearest, ties to even)
            pile[0][c] = (pile[0][c] + 1) & M64
            pile[1][c] = (pile[1][c] + ns) & M64
            pile[2][c] = (pile[2][c] + u) & M64
            pile[3][c] = (pile[3][c] + u * u) & M64
    return np.array(pile, np.uint64)


def test_levels_pile_against_plain_python():
    cases = P.pile_cases() + [c for _, c in P.invalid_pair_calls()] + P.split_call()
    for call in cases:
        got, want = call.expected(), plain_levels_pile(call)
        assert (got == want).all(), (call.name, np.argwhere(got != want)[:5].tolist())
    names = [c.name for c in P.pile_cases()]
    assert len(names) == len(set(names)) == 19 and len(P.invalid_pair_calls()) == 12
    assert sum(len(c.pairs) for c in P.pile_cases()) == 514


def test_the_count_words_two_halves():
    for call in [c for c in P.pile_cases() if c.name.startswith("skip")]:
        w = call.expected()[0]
        kept, skipped = w & np.uint64(0xFFFFFFFF), w >> np.uint64(32)
        assert ((kept + skipped)[11:141] == 3).all() and int(skipped.sum()) >= 12 and int(kept.sum()) + int(skipped.sum()) == 390, call.name
    # the low half carries into the high half: ONE 64-bit number
    call = [c for c in P.pile_cases() if c.name == "added to a dirty arena"][0]
    before, after = call.before[0], call.expected()[0]
    carried = (before & np.uint64(0xFFFFFFFF)) == np.uint64(0xFFFFFFFF)
    grew = after != before
    assert (carried & grew).any()
    for b, a in zip(before[carried & grew], after[carried & grew]):
        assert int(a) & 0xFFFFFFFF < 0xFFFFFFFF and int(a) >> 32 > int(b) >> 32
    # an invalid pair and a pair without a good fit under REQUIRE_OK add to neither half
    for _, call in P.invalid_pair_calls():
        w = call.expected()[0]
        assert int((w & np.uint64(0xFFFFFFFF)).sum() + (w >> np.uint64(32)).sum()) == 80, call.name


def test_u_at_the_bound_and_the_next_w_beyond_it():
    edge = 2.0 ** 24
    keep, u = P.fixed([edge, -edge, math.nextafter(edge, math.inf), math.nextafter(-edge, -math.inf), math.nextafter(edge, 0.0), float("nan"), float("inf"),
                       0.5, 1.5, 2.5, -0.5, -2.5])
    assert keep.tolist() == [True, True, False, False, True, False, False, True, True, True, True, True]
    assert u.tolist() == [1 << 24, -(1 << 24), 0, 0, 1 << 24, 0, 0, 0, 2, 2, 0, -2]
    got = [c for c in P.pile_cases() if c.name == "u at the bound"][0].expected()
    assert int(got[0, 3]) == 2 and int(got[0, 4]) == 2 and int(got[0, 5]) == 2                       # 2^24, 2^24 and -2^24 kept beside the small ones
    assert int(got[0, 6]) == 1 + (1 << 32) and int(got[0, 7]) == 1 + (1 << 32)                       # one quarter beyond: skipped
    assert int(got[3, 3]) == 1 << 48 and int(got[2, 3]) == 1 << 24 and int(got[2, 5]) == (-(1 << 24) + 2) & M64   # (+ rint(1.5) of the second pair)


def test_squiggle_kmers_is_the_squiggle_without_the_gather():
    cases = P.kmers_cases()
    assert len(cases) == len(R.squiggle_cases()) + 32
    assert {(c.k, c.flags) for c in cases} == {(k, f) for k in range(1, 10) for f in range(4)}
    for call in cases:
        if call.seq.shape[1] > 9000:
            continue   # (the 70 000-base case: the device tests run it)
        kmer, kmer_len = P.squiggle_kmers(call.seq, call.seq_len, call.k, call.target_stride, call.flags)
        target, target_len, masked, level = call.expected()
        live = kmer != P.MARK
        m = np.where(live, call.model[np.where(live, kmer, 0)], np.uint32(0))
        assert (kmer_len == target_len).all() and (m == level).all() and (np.where(live, R.quantise(m, call.quant), 0) == target).all(), call.name
        inside = np.arange(call.target_stride)[None, :] < target_len[:, None]
        assert ((~live & inside).sum(axis=1) == masked).all() and not (live & ~inside).any(), call.name
        assert (kmer[live] < 4 ** call.k).all()


def plain_pile_kmers(call):
    cells = 4 ** call.k
    rows, T = call.kmer.shape
    out = [[0] * cells for _ in range(4)] if call.before is None or call.flags & P.CLEAR else [[int(v) for v in plane] for plane in call.before]
    for g in range(rows):
        L = int(call.target_len[g])
        if L > T:
            continue
        for j in range(L):
            idx = int(call.kmer[g, j])
            if idx < cells:
                for q in range(4):
                    out[q][idx] = (out[q][idx] + int(call.pile[q, g * T + j])) & M64
    return np.array(out, np.uint64)


def test_pile_kmers_against_plain_python():
    cases = P.pile_kmers_cases()
    assert len(cases) == 9 * 4 + 4 * 6
    assert {c.k for c in cases} == set(range(1, 10)) and {c.k for c in cases if c.flags & P.DIRECT} == set(range(1, 10))   # both forms at every k
    for call in cases:
        if call.kmer.shape[0] * call.kmer.shape[1] > 10000 and call.k not in (1, 6):
            continue   # (the plain loop is slow: the large tables at two k, the small ones at every k)
        got, want = call.expected(), plain_pile_kmers(call)
        assert (got == want).all(), (call.name, np.argwhere(got != want)[:5].tolist())


def test_positions_then_kmers_equal_a_direct_pile_of_the_levels():
    rng = np.random.default_rng(2811)
    call = [t for t in P.pile_cases() if t.name == "staggered overlaps"][0]
    pile = call.expected()
    pairs, hit, n_levels, levels, n_reads, fit = call.arrays()
    for k in (2, 6):
        kmer = rng.integers(0, 4 ** k, (2, call.T)).astype(np.uint32)
        direct = [[0] * 4 ** k for _ in range(4)]
        for p in range(len(pairs)):
            keep, u, ns = P.level_values(levels[p, :n_levels[p]], 0.0, 1.0, call.fix, 0, 0)
            for t in range(int(n_levels[p])):
                idx = int(kmer[pairs[p][1], hit[p][2] + t])
                adds = (1, int(ns[t]), int(u[t]), int(u[t]) ** 2) if keep[t] else (1 << 32, 0, 0, 0)
                for q in range(4):
                    direct[q][idx] = (direct[q][idx] + adds[q]) & M64
        assert (P.pile_kmers(pile, kmer, call.target_len, k) == np.array(direct, np.uint64)).all(), k


def plain_model_update(call):
    cells = 4 ** call.k
    fix = f32(to_f32_bits(call.fix))
    model, sd = [], []
    for i in range(cells):
        n = int(call.kmer_pile[0, i]) & 0xFFFFFFFF
        if n < max(call.min_obs, 1):
            model.append(int(call.prior[i]))
            sd.append(0)
            continue
        total = int(call.kmer_pile[2, i])
        total -= (1 << 64) if total >> 63 else 0
        mean = float(total) / float(n)
        var = float(int(call.kmer_pile[3, i])) / float(n) - mean * mean
        model.append(to_f32_bits(mean / fix))
        sd.append(to_f32_bits(math.sqrt(max(var, 0.0)) / fix))
    return np.array(model, np.uint32), np.array(sd, np.uint32)


def test_model_update_against_plain_python():
    cases = P.update_cases()
    assert len(cases) == 10 and {c.k for c in cases} >= {1, 2, 3, 4, 6, 9}
    below = 0
    for call in cases:
        if call.k == 9:
            continue   # (262 144 k-mers: the device tests run it)
        got, want = call.expected(), plain_model_update(call)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), call.name
        if call.name.startswith("equal observations"):
            kp = call.kmer_pile
            n = (kp[0] & np.uint64(0xFFFFFFFF)).astype(np.float64)
            mean = kp[2].view(np.int64).astype(np.float64) / n
            below = int((kp[3].astype(np.float64) / n - mean * mean < 0).sum())
            assert (got[1][kp[3].astype(np.float64) / n - mean * mean < 0] == 0).all()
    assert below > 0   # var does round below zero in the catalogue
    # the prior's 32 bits are kept: a NaN payload, -0
    call = cases[2]
    model, sd = call.expected()
    kept = (call.kmer_pile[0] & np.uint64(0xFFFFFFFF)).astype(np.int64) < 8
    assert (model[kept] == call.prior[kept]).all() and (sd[kept] == 0).all() and 0x7FC12345 in model[kept].tolist() + call.prior[~kept].tolist()


def test_the_model_chains_conditions_hold_on_the_numpy_statements():
    import model_chain as MC

    d = MC.numpy_chain()
    MC.assert_conditions(d)
    q = MC.margins(d)
    assert q["observations"] > 3500 and q["smallest_count"] >= 30 and q["worst_start_offset"]["one"] <= 4 and q["worst_start_offset"]["two"] <= 4, q
    # the update moved exactly what it had observations for, and every k-mer had them
    assert (d["model"] != MC.planted()[2].view(np.uint32)).sum() > MC.MOVED and (d["sd"].view(np.float32) > 0).all()
