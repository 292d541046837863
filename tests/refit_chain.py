"""The refit chain's planted workload and its numpy statement, shared by test_squiggle_ref (which asserts the chain's conditions on the
numpy statements alone) and test_gpu_refit_chain (which holds every table of the device's chain to them bit for bit).

A random sequence of 2 400 bases and a random 5-mer model whose levels are whole numbers of 1 / 32; reads synthesised from stretches of both
strands' squiggles under a planted per-read line  counts = a level + b  with noise, a within 12 % of 8 and |b| up to 60 counts.  Round one runs
under constants that are deliberately off -- offset 0, scale 1 / 256 for every read, as if a were 8 and b were 0 -- and round two under the
tables vbz_gpu_levels_fit_batch makes of round one's levels."""
import functools

import numpy as np

import eventalign_ref as E
import events_ref as EV
import locate_path_ref as LP
import locate_span_ref as LS
import match_path_ref as MP
import segment_ref as S
import squiggle_ref as R

K, BASES, STRIDE_SEQ, STRIDE = 5, 2400, 2416, 2400
N, W, QUANT, MIN_N, READS = 128, 256, 32.0, 5, 8
SCALE0, OFFSET0 = 1.0 / 256.0, 0.0
L = BASES - K + 1


@functools.lru_cache(maxsize=None)
def planted():
    """(seq uint8 [1, STRIDE_SEQ], model float32 [4 ** K], the reads' int16 signals, (strand, first level, levels, a, b) per read)"""
    rng = np.random.default_rng(2510)
    seq = np.full((1, STRIDE_SEQ), 0x4E, np.uint8)
    seq[0, :BASES] = np.frombuffer(R.random_seq(rng, BASES), np.uint8)
    model = (rng.integers(-100, 101, 4 ** K) / 32.0).astype(np.float32)
    target = R.squiggle(seq, [BASES], model.view(np.uint32), K, STRIDE, QUANT, R.BOTH)[0]
    reads, plan = [], []
    for i in range(READS):
        g, m = i % 2, int(rng.integers(150, 190))
        first = int(rng.integers(0, L - m))
        a, b = 8.0 * (1.0 + rng.uniform(-0.12, 0.12)), float(rng.uniform(-60, 60))
        dwell = rng.integers(6, 15, m)
        x = np.repeat(a * target[g, first:first + m].astype(np.float64) + b, dwell) + rng.normal(0, 4, int(dwell.sum()))
        reads.append(np.clip(np.rint(x), -32768, 32767).astype(np.int16))
        plan.append((g, first, m, a, b))
    return seq, model, reads, plan


def round_of(signals, starts, first, cap, offset, scale, target, target_len):
    """events under (offset, scale) -> events_query -> locate_span -> match_best, as numpy tables"""
    want = [EV.event_rows(x, None, None, starts[i].tolist(), offset[i], scale[i]) for i, x in enumerate(signals)]
    rec = np.zeros((cap, 4), np.uint32)
    mom = np.zeros((cap, 2), np.uint64)
    total = int(first[-1])
    rec[:total], mom[:total] = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want]).view(np.uint64)
    query, valid, index = E.events_query(first.astype(np.uint64), cap, rec[:, 0], rec[:, 2], N, MIN_N, None)
    spans = LS.spans(query.view(np.float32), valid, QUANT, target, target_len)
    return {"rec": rec, "mom": mom, "query": query, "valid": valid, "index": index, "spans": spans, "pairs": MP.best(spans)}


@functools.lru_cache(maxsize=None)
def numpy_chain():
    seq, model, signals, plan = planted()
    target, target_len, masked, level = R.squiggle(seq, [BASES], model.view(np.uint32), K, STRIDE, QUANT, R.BOTH)
    starts = [S.starts(x) for x in signals]
    first = np.concatenate([[0], np.cumsum([len(v) for v in starts])]).astype(np.int64)
    cap = sum(S.max_rows(len(x), 2) for x in signals)
    start = np.zeros(cap, np.uint32)
    start[:int(first[-1])] = np.concatenate(starts)
    d = {"target": target, "target_len": target_len, "masked": masked, "first": first, "start": start, "cap": cap}
    one = round_of(signals, starts, first, cap, [OFFSET0] * READS, [SCALE0] * READS, target, target_len)
    hit, rows = LP.paths(one["query"].view(np.float32), one["valid"], QUANT, target, target_len, one["pairs"], W)
    n_levels, levels = E.levels(one["pairs"], hit, rows, one["index"], first.astype(np.uint64), cap, start, one["rec"][:, 2], one["mom"], READS, N, W)
    out, sums = R.levels_fit(one["pairs"], hit, n_levels, levels, target, target_len, READS, W, MIN_N, 0, QUANT, None)
    offset, scale = R.fitted_tables(out)
    two = round_of(signals, starts, first, cap, offset, scale, target, target_len)
    d.update({"one": one, "hit": hit, "rows": rows, "n_levels": n_levels, "levels": levels, "fit": out, "sums": sums, "two": two})
    return d


def assert_conditions(d):
    """the planted strand and stretch are found in both rounds, each read's second-round cost is not above its first, and the fit moved
    the constants towards the planted line"""
    seq, model, signals, plan = planted()
    assert d["masked"].tolist() == [0, 0] and d["target_len"].tolist() == [L, L]
    offset, scale = R.fitted_tables(d["fit"])
    for i, (g, first, m, a, b) in enumerate(plan):
        for name in ("one", "two"):
            read, ref, begin, end = (int(v) for v in d[name]["pairs"][i])
            cost, e, s, _ = (int(v) for v in d[name]["spans"][i, ref])
            assert read == i and ref == g and first - 3 <= s <= first + 3 and e - s > 0.6 * min(m, N), (name, i, plan[i], d[name]["spans"][i].tolist())
        c1, c2 = int(d["one"]["spans"][i, g, 0]), int(d["two"]["spans"][i, g, 0])
        assert c2 <= c1, (i, c1, c2)
        assert d["fit"][i][3] == 1 and d["fit"][i][2] >= 20, (i, d["fit"][i].tolist())
        # under the planted line the constants are offset = -b and scale = 1 / (a quant); round one is off by up to 12 % and 60 counts, and
        # a fit that is worth its name at least halves both
        assert abs(float(scale[i]) * a * QUANT - 1.0) < 0.06 and abs(float(offset[i]) + b) < 30.0, (i, float(offset[i]), float(scale[i]), a, b)
    total1 = sum(int(d["one"]["spans"][i, p[0], 0]) for i, p in enumerate(plan))
    total2 = sum(int(d["two"]["spans"][i, p[0], 0]) for i, p in enumerate(plan))
    assert total2 < 0.7 * total1, (total1, total2)
