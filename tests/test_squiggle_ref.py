"""tests/squiggle_ref.py held to plain Python: the squiggle statement to a loop over k-mers on random small cases, the fit's integer sums
to Python big integers and its float64 formula to Python floats, the stated bounds reached by the extreme catalogue case without leaving
int64, the catalogues counted, and the refit chain's conditions met by the numpy statements alone (tests/refit_chain.py), so that the test
on the MI355X cannot pass vacuously."""
import math
import struct

import numpy as np

import refit_chain as RC
import squiggle_ref as R

LETTER = {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3, "U": 3, "u": 3}


def f32(x):
    return struct.unpack("<f", struct.pack("<I", int(x)))[0]


def plain_quantise(bits, quant):
    v = float(np.float32(f32(bits)) * np.float32(quant))   # one float32 multiply
    if math.isnan(v):
        return 0
    if math.isinf(v):
        return 127 if v > 0 else -127
    r = round(v)   # Python rounds halves to even
    return max(-127, min(127, r))


def plain_squiggle(seq, seq_len, model, k, target_stride, quant, flags):
    S, stride = seq.shape
    rows = 2 * S if flags & R.BOTH else S
    out = []
    for r in range(rows):
        s, rc = (r >> 1, r & 1) if flags & R.BOTH else (r, 0)
        n = int(seq_len[s])
        q, m, masked = [0] * target_stride, [0] * target_stride, 0
        L = n - k + 1 if k <= n <= stride else 0
        if L > target_stride:
            L = 0
        if L:
            b = [LETTER.get(chr(x)) for x in seq[s, :n]]
            if rc:
                b = [None if x is None else 3 - x for x in reversed(b)]
            for j in range(L):
                kmer = b[j:j + k]
                at = L - 1 - j if flags & R.REVERSED else j
                if None in kmer:
                    masked += 1
                    continue
                index = sum(x * 4 ** (k - 1 - i) for i, x in enumerate(kmer))
                m[at], q[at] = int(model[index]), plain_quantise(model[index], quant)
        out.append((q, m, L, masked))
    return out


def test_squiggle_statement_against_a_plain_loop():
    rng = np.random.default_rng(77)
    alphabet = np.frombuffer(b"ACGTacgtUuNn-\x00\xff", np.uint8)
    for trial in range(60):
        k = int(rng.integers(1, 10))
        S = int(rng.integers(1, 4))
        stride = 16 * int(rng.integers(1, 5))
        target_stride = 16 * int(rng.integers(1, 5))
        seq = rng.choice(alphabet, (S, stride), p=[0.2] * 4 + [0.03] * 4 + [0.02] * 2 + [0.008] * 5)
        seq_len = rng.integers(0, stride + 3, S).astype(np.uint32)
        model = rng.normal(0, 3, 4 ** k).astype(np.float32)
        model[rng.integers(0, 4 ** k, 3)] = [np.nan, np.inf, 1.5 / 32]
        flags = int(rng.integers(0, 4))
        got = R.squiggle(seq, seq_len, model.view(np.uint32), k, target_stride, 32.0, flags)
        want = plain_squiggle(seq, seq_len, model.view(np.uint32), k, target_stride, 32.0, flags)
        for r, (q, m, L, masked) in enumerate(want):
            assert got[0][r].tolist() == q and got[3][r].tolist() == m and got[1][r] == L and got[2][r] == masked, (trial, r, k, flags)


def test_quantiser_is_the_match_calls():
    from vbz_compression_amd.batch import quantize_levels
    v = np.concatenate([R.special_model(), np.random.default_rng(3).normal(0, 5, 4000).astype(np.float32)])
    for quant in (32.0, 1.5, 1e-3):
        assert (R.quantise(v.view(np.uint32), quant) == quantize_levels(v, quant)).all()
    assert R.quantise(R.special_model().view(np.uint32), 32.0).tolist()[:14] == [0, 127, -127, 0, 0, 2, 2, 0, -2, 126, 127, -127, 127, -127]


def plain_fit(call):
    """the fit of every pair of a call in Python integers and floats -> [(offset bits, scale bits, used, ok, sums)]"""
    pairs, hit, n_levels, levels, n_reads, prior = call.arrays()
    out = []
    for p in range(len(pairs)):
        W = int(n_levels[p])
        K, Sg, Sgg, Sq, Sgq, fit = 0, 0, 0, 0, 0, None
        if R.pair_valid(pairs[p], hit[p], W, call.target_len, call.target.shape[1], n_reads, call.W):
            start, ref = int(hit[p][2]), int(pairs[p][1])
            for t in range(W):
                ns, ne = int(levels[p, t, 2]), int(levels[p, t, 3])
                total = int(levels[p, t, 4]) | int(levels[p, t, 5]) << 32
                total -= (total >> 63) << 64
                if ns < max(call.min_samples, 1) or (call.max_entries and ne > call.max_entries):
                    continue
                m = float(total) / float(ns)
                if not abs(m) <= 32768:
                    continue
                q, g = round(m * 64.0), int(call.target[ref, start + t])
                K, Sg, Sgg, Sq, Sgq = K + 1, Sg + g, Sgg + g * g, Sq + q, Sgq + g * q
            num, den = K * Sgq - Sg * Sq, K * Sgg - Sg * Sg
            assert abs(num) < 1 << 62 and 0 <= den < 1 << 47 and all(abs(v) < 1 << 63 for v in (Sg, Sgg, Sq, Sgq))
            if K >= 2 and den > 0 and num > 0:
                A = float(num) / float(den)
                B = (float(Sq) - A * float(Sg)) / float(K)
                a, b = A / 64.0, B / 64.0
                with np.errstate(over="ignore"):
                    scale, offset = np.float32(1.0 / (a * float(np.float32(call.quant)))), np.float32(-b)
                if np.isfinite(scale) and np.isfinite(offset) and scale > 0:
                    fit = (offset, scale)
        if fit is None:
            fit = R.prior_constants(prior, int(pairs[p][0]), n_reads)
            ok = 0
        else:
            ok = 1
        bits = np.array(fit, np.float32).view(np.uint32)
        out.append((int(bits[0]), int(bits[1]), K, ok, (Sg, Sgg, Sq, Sgq)))
    return out


def test_fit_statement_against_python_integers_and_floats():
    calls = [c for c in R.fit_cases() if c.name != "the extreme case"] + [c for _, c, _ in R.invalid_pair_calls()]
    for call in calls:
        out, sums = call.expected()
        for p, (o, s, K, ok, sm) in enumerate(plain_fit(call)):
            assert out[p].tolist() == [o, s, K, ok] and [int(v) for v in sums[p]] == list(sm), (call.name, p)


def test_the_extreme_case_reaches_the_bounds_inside_int64():
    call = R.extreme_call()
    pairs, hit, n_levels, levels, n_reads, prior = call.arrays()
    out, sums = call.expected()
    g = call.target[0].astype(object)
    assert len(g) == 65536 and min(g) == -128 and max(g) == 127
    for p, sign in ((0, 1), (1, -1)):
        q = [sign * (-32768 if t % 2 == 0 else 32768) * 64 for t in range(65536)]
        assert max(abs(v) for v in q) == 1 << 21
        K, Sg, Sgg, Sq, Sgq = 65536, sum(g), sum(x * x for x in g), sum(q), sum(x * y for x, y in zip(g, q))
        assert [int(v) for v in sums[p]] == [Sg, Sgg, Sq, Sgq] and out[p][2] == K
        num, den = K * Sgq - Sg * Sq, K * Sgg - Sg * Sg
        assert 1 << 59 < abs(num) < 1 << 62 and 1 << 45 < den < 1 << 47, (num.bit_length(), den.bit_length())
        assert out[p][3] == (1 if sign > 0 else 0) and (num > 0) == (sign > 0)
    assert plain_fit(call)[0][:4] == tuple(out[0].tolist())


def test_exact_recovery_is_exact():
    call = R.exact_call()
    out, _ = call.expected()
    offset, scale = R.fitted_tables(out)
    for p, (a, b) in enumerate(call.planted):
        assert out[p][3] == 1 and offset[p] == np.float32(-b) and scale[p] == np.float32(1.0 / (a * 32.0)), (p, a, b, offset[p], scale[p])


def test_invalid_pairs_keep_the_prior_and_spare_their_neighbours():
    for name, call, bad in R.invalid_pair_calls():
        out, sums = call.expected()
        pairs, hit, n_levels, levels, n_reads, prior = call.arrays()
        assert out[bad][2:].tolist() == [0, 0] and not sums[bad].any(), name
        want = R.prior_constants(prior, int(pairs[bad][0]), n_reads)
        assert out[bad][:2].tolist() == np.array(want, np.float32).view(np.uint32).tolist(), name
        if int(pairs[bad][0]) >= n_reads:
            assert out[bad][:2].tolist() == [0, 0x3F800000], name
        assert out[0][2:].tolist() == [40, 1] and out[2][2:].tolist() == [40, 1], name


def test_the_catalogues_hold_what_they_promise():
    cases = R.squiggle_cases()
    assert {c.k for c in cases} == {1, 2, 5, 6, 9} and {c.flags for c in cases} == {0, 1, 2, 3}
    assert any(not c.use_level for c in cases) and any(c.quant != 32.0 for c in cases)
    Ls, masked_rows, refused = set(), 0, 0
    for c in cases:
        target, target_len, masked, level = c.expected()
        Ls |= {int(v) for v in target_len}
        masked_rows += int((masked > 0).sum())
        refused += int(((target_len == 0) & (np.repeat(c.seq_len, 2 if c.flags & R.BOTH else 1) >= c.k)).sum())
        if c.name.startswith("a palindrome"):
            assert (target[0] == target[1]).all() and (level[0] == level[1]).all() and target_len[0] == target_len[1] == 1396
        if c.name.startswith("lower case"):
            assert (target[0] == target[2]).all() and (target[0] == target[4]).all() and not masked.any()
        if c.name.startswith("all 256"):
            assert masked.min() > 700
        if c.name.startswith("special"):
            assert {0, 127, -127, 2, -2, 126} <= set(target[0].tolist()) and 0x7FC12345 in level[0] and 0x80000000 in level[0]
        if c.name.startswith("70 000"):
            assert target_len.tolist() == [69992, 69992] and 100 < masked[0] == masked[1]
    for seam in (R.LANE, R.WAVE, R.BLOCK):
        assert {seam - 1, seam, seam + 1} <= Ls, seam
    assert {0, 1, 2} <= Ls and masked_rows > 300 and refused >= 8
    fits = R.fit_cases()
    widths = {int(w) for c in fits for w in c.n_levels}
    assert {1, 2, 63, 64, 65, 128, 65536} <= widths
    starts = {int(h[2]) % 4 for c in fits for h in c.hit}
    assert starts == {0, 1, 2, 3}
    assert any(int(h[1]) == int(c.target_len[int(p[1])]) for c in fits for p, h in zip(c.pairs, c.hit))
    used, oks = set(), set()
    for c in fits:
        out, sums = c.expected()
        used |= {int(v) for v in out[:, 2]}
        oks |= {int(v) for v in out[:, 3]}
    assert {0, 1, 2, 65536} <= used and oks == {0, 1}
    assert any(c.prior is None for c in fits) and any(c.prior is not None for c in fits) and any(not c.use_sums for c in fits)
    assert len(R.invalid_pair_calls()) == 12


def test_the_chain_conditions_hold_for_the_numpy_statements():
    d = RC.numpy_chain()
    RC.assert_conditions(d)
