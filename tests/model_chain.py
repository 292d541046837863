"""The model chain's planted workload and its numpy statement, shared by test_pile_ref (which asserts the chain's conditions on the numpy
statements alone) and test_gpu_model_chain (which holds every table of the device's chain to them bit for bit).

A random sequence of 1 200 bases and a true 3-mer model whose levels are whole numbers of 1 / 32 in +-100 / 32; 32 reads synthesised from
stretches of both strands' true squiggles, 150 - 190 levels each, dwell 6 - 14 samples, 8 counts a level, noise sd 4.  The prior model is the
true one with 16 k-mers moved by +-16 ... 32 / 32.  Round one runs under the prior; its levels are fitted, piled per position, added per k-mer
and turned into a new model (fix 256, min_obs 8); round two runs under the new model's squiggle and the fitted constants."""
import functools

import numpy as np

import eventalign_ref as E
import locate_path_ref as LP
import pile_ref as P
import refit_chain as RC
import segment_ref as S
import squiggle_ref as R

K, BASES, STRIDE_SEQ, STRIDE = 3, 1200, 1216, 1200
N, W, QUANT, MIN_N, READS = RC.N, RC.W, RC.QUANT, RC.MIN_N, 32   # (128, 256, 32.0, 5: refit_chain's round_of runs under them)
FIX, MIN_OBS, MOVED = 256.0, 8, 16
SCALE0, OFFSET0 = 1.0 / 256.0, 0.0
L = BASES - K + 1
SEED = 2820


@functools.lru_cache(maxsize=None)
def planted():
    """(seq uint8 [1, STRIDE_SEQ], true model, prior model float32 [4 ** K], the moved k-mers, the reads' int16 signals, (strand, first level,
    levels) per read)"""
    rng = np.random.default_rng(SEED)
    seq = np.full((1, STRIDE_SEQ), 0x4E, np.uint8)
    seq[0, :BASES] = np.frombuffer(R.random_seq(rng, BASES), np.uint8)
    true = (rng.integers(-100, 101, 4 ** K) / 32.0).astype(np.float32)
    moved = np.sort(rng.choice(4 ** K, MOVED, replace=False))
    prior = true.copy()
    prior[moved] += (rng.integers(16, 33, MOVED) * rng.choice([-1, 1], MOVED) / 32.0).astype(np.float32)
    target = R.squiggle(seq, [BASES], true.view(np.uint32), K, STRIDE, QUANT, R.BOTH)[0]
    reads, plan = [], []
    for i in range(READS):
        g, m = i % 2, int(rng.integers(150, 190))
        first = int(rng.integers(0, L - m))
        dwell = rng.integers(6, 15, m)
        x = np.repeat(8.0 * target[g, first:first + m].astype(np.float64), dwell) + rng.normal(0, 4, int(dwell.sum()))
        reads.append(np.clip(np.rint(x), -32768, 32767).astype(np.int16))
        plan.append((g, first, m))
    return seq, true, prior, moved, reads, plan


@functools.lru_cache(maxsize=None)
def numpy_chain():
    seq, true, prior, moved, signals, plan = planted()
    squiggle = lambda model: R.squiggle(seq, [BASES], np.asarray(model).view(np.uint32), K, STRIDE, QUANT, R.BOTH)   # noqa: E731
    target, target_len, masked, _ = squiggle(prior)
    kmer, kmer_len = P.squiggle_kmers(seq, [BASES], K, STRIDE, R.BOTH)
    starts = [S.starts(x) for x in signals]
    first = np.concatenate([[0], np.cumsum([len(v) for v in starts])]).astype(np.int64)
    cap = sum(S.max_rows(len(x), 2) for x in signals)
    start = np.zeros(cap, np.uint32)
    start[:int(first[-1])] = np.concatenate(starts)
    d = {"target": target, "target_len": target_len, "masked": masked, "kmer": kmer, "kmer_len": kmer_len, "first": first, "start": start, "cap": cap}
    one = RC.round_of(signals, starts, first, cap, [OFFSET0] * READS, [SCALE0] * READS, target, target_len)
    hit, rows = LP.paths(one["query"].view(np.float32), one["valid"], QUANT, target, target_len, one["pairs"], W)
    n_levels, levels = E.levels(one["pairs"], hit, rows, one["index"], first.astype(np.uint64), cap, start, one["rec"][:, 2], one["mom"], READS, N, W)
    fit, sums = R.levels_fit(one["pairs"], hit, n_levels, levels, target, target_len, READS, W, MIN_N, 0, QUANT, None)
    pile = P.levels_pile(one["pairs"], hit, n_levels, levels, target_len, STRIDE, READS, W, MIN_N, 0, FIX, fit, P.REQUIRE_OK)
    kmer_pile = P.pile_kmers(pile, kmer, kmer_len, K)
    model, sd = P.model_update(kmer_pile, prior.view(np.uint32), K, MIN_OBS, FIX)
    target2 = squiggle(model)[0]
    offset, scale = R.fitted_tables(fit)
    two = RC.round_of(signals, starts, first, cap, offset, scale, target2, target_len)
    d.update({"one": one, "hit": hit, "rows": rows, "n_levels": n_levels, "levels": levels, "fit": fit, "pile": pile, "kmer_pile": kmer_pile, "model": model,
              "sd": sd, "target2": target2, "two": two})
    return d


def margins(d):
    """the chain's quantities: what assert_conditions holds, and what the issue's table lists"""
    seq, true, prior, moved, signals, plan = planted()
    model = d["model"].view(np.float32)
    count = (d["kmer_pile"][0] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    err, err0 = np.abs(model.astype(np.float64) - true), np.abs(prior.astype(np.float64) - true)
    still = np.setdiff1d(np.arange(4 ** K), moved)
    cost = lambda name: np.array([int(d[name]["spans"][i, p[0], 0]) for i, p in enumerate(plan)], np.int64)   # noqa: E731
    start_off = {name: max(abs(int(d[name]["spans"][i, p[0], 2]) - p[1]) for i, p in enumerate(plan)) for name in ("one", "two")}
    return {"observations": int(count.sum()), "smallest_count": int(count.min()), "worst_moved_ratio": float((err[moved] / err0[moved]).max()),
            "worst_unmoved_error": float(err[still].max()), "cost_one": int(cost("one").sum()), "cost_two": int(cost("two").sum()),
            "reads_whose_cost_rises": int((cost("two") > cost("one")).sum()), "worst_start_offset": start_off}


def assert_conditions(d):
    """every read's strand is found and its start is within 8 levels in both rounds; each moved k-mer's error against the true model is at
    most half its prior error; no other k-mer is more than 0.25 from it; round two's summed cost is below half of round one's; no read's
    cost rises"""
    seq, true, prior, moved, signals, plan = planted()
    assert d["masked"].tolist() == [0, 0] and d["target_len"].tolist() == [L, L]
    for i, (g, first, m) in enumerate(plan):
        for name in ("one", "two"):
            read, ref, begin, end = (int(v) for v in d[name]["pairs"][i])
            s = int(d[name]["spans"][i, ref, 2])
            assert read == i and ref == g and abs(s - first) <= 8, (name, i, plan[i], d[name]["spans"][i].tolist())
    q = margins(d)
    assert q["smallest_count"] >= MIN_OBS, q
    assert q["worst_moved_ratio"] <= 0.5 and q["worst_unmoved_error"] <= 0.25, q
    assert 2 * q["cost_two"] < q["cost_one"] and q["reads_whose_cost_rises"] == 0, q
