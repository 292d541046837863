#!/usr/bin/env python3
"""Cost of the four pile-up calls (include/vbz_gpu_pile.h) against the unfused torch route for each -- float64 arithmetic and index_add_ on
int64 -- the legs alternating in one process (median of --reps calls, HIP events on the codec's stream, untimed warm-up calls first).

  levels_pile     on tools/time_refit.py's workload (--reads pairs, N = 2 048, G = 2 targets of --levels levels: a coverage depth of some
                  250), over the levels arena and the fit table the chain leaves, beside levels_fit, which reads the same arena without
                  adds; and the same pairs dealt over G = 64 targets (depth about 8), to show what contention costs
  squiggle_kmers  G sequences of --levels + k - 1 bases: k = 1, 5, 6 and 9 at G = 2, k = 5 and 6 at G = 64
  pile_kmers      the position pile of each levels_pile leg into k-mer piles at the same k: as the library chooses (the table in LDS up to
                  csrc/vbz_kernels.h's PILE_KMERS_LDS_KMAX) and with global adds (DIRECT), so both sides of the threshold
  model_update    at the same k
Every arena is checked bit for bit against the torch route.  Bytes of adds are what the rule adds: 32 a kept level, 8 a skipped one.

    python tools/time_pile.py [--reads 8192] [--reps 20] [--levels 30000] [--out profiles/pile_time.json]"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import squiggle_ref as R  # noqa: E402
from time_eventalign import G, N, QUANT, SCALE, Tables, compressed  # noqa: E402
from time_segment import timed  # noqa: E402
from vbz_compression_amd import batch  # noqa: E402

FIX = 256.0
LDS_KMAX = int(re.search(r"PILE_KMERS_LDS_KMAX = (\d+);", open(os.path.join(ROOT, "vbz_compression_amd", "csrc", "vbz_kernels.h")).read()).group(1))
u = lambda t: t.to(torch.int64) & 0xFFFFFFFF   # noqa: E731


def unfused_pile(pairs, hit, n_levels, lv, fit, t_len, Gn, stride, fix, min_samples, max_entries, require_ok):
    """-> pile int64 [4, Gn * stride]"""
    dev, W = lv.device, int(lv.shape[1])
    ref, end, start, nl = u(pairs[:, 1]), u(hit[:, 1]), u(hit[:, 2]), u(n_levels)
    refc = ref.clamp(max=Gn - 1)
    Lg = u(t_len)[refc]
    valid = (ref < Gn) & (nl > 0) & (nl <= W) & (end > start) & (end - start == nl) & (Lg > 0) & (Lg <= stride) & (end <= Lg)
    if require_ok:
        valid &= fit[:, 3] != 0
    t = torch.arange(W, device=dev)[None, :]
    live = (t < nl[:, None]) & valid[:, None]
    ns, ne, total = u(lv[..., 2]), u(lv[..., 3]), lv.view(torch.int64)[..., 2]
    keep = ns >= max(min_samples, 1)
    if max_entries:
        keep &= ne <= max_entries
    f = torch.float64
    o, s = fit[:, 0].view(torch.float32).to(f)[:, None], fit[:, 1].view(torch.float32).to(f)[:, None]
    w = ((total.to(f) / ns.clamp(min=1).to(f) + o) * s) * float(np.float32(fix))
    keep &= w.abs() <= 16777216.0
    val = torch.where(keep, torch.round(w), 0.0).to(torch.int64)
    cell = (refc[:, None] * stride + start[:, None] + t)[live]
    keep, val, ns = keep[live], val[live], ns[live]
    pile = torch.zeros((4, Gn * stride), dtype=torch.int64, device=dev)
    pile[0].index_add_(0, cell, torch.where(keep, 1, 1 << 32))
    pile[1].index_add_(0, cell, torch.where(keep, ns, 0))
    pile[2].index_add_(0, cell, val)
    pile[3].index_add_(0, cell, val * val)
    return pile


def unfused_kmers(seq, lens, lut, k, T):
    """the given strand of every sequence -> kmer int32 [S, T]; lens on the host"""
    dev, S = seq.device, int(seq.shape[0])
    kmer = torch.full((S, T), -1, dtype=torch.int32, device=dev)
    for s in range(S):
        c = lut[seq[s, :lens[s]].to(torch.int64)]
        L = lens[s] - k + 1
        index, bad = torch.zeros(L, dtype=torch.int64, device=dev), torch.zeros(L, dtype=torch.bool, device=dev)
        for i in range(k):
            part = c[i:i + L]
            bad |= part == 4
            index = index * 4 + part.clamp(max=3)
        kmer[s, :L] = torch.where(bad, -1, index).to(torch.int32)
    return kmer


def unfused_pile_kmers(pile, kmer, t_len, k):
    dev, (Gn, T) = pile.device, kmer.shape
    key = u(kmer)
    live = (torch.arange(T, device=dev)[None, :] < u(t_len).clamp(max=T)[:, None]) & (u(t_len) <= T)[:, None] & (key < 4 ** k)
    out = torch.zeros((4, 4 ** k), dtype=torch.int64, device=dev)
    idx = key[live]
    for q in range(4):
        out[q].index_add_(0, idx, pile[q].reshape(Gn, T)[live])
    return out


def unfused_update(kp, prior, fix, min_obs):
    f = torch.float64
    n = kp[0] & 0xFFFFFFFF
    have = n >= max(min_obs, 1)
    nn = n.clamp(min=1).to(f)
    mean = kp[2].to(f) / nn
    sq = torch.where(kp[3] < 0, kp[3].to(f) + 18446744073709551616.0, kp[3].to(f))   # (a uint64 above 2^63)
    var = sq / nn - mean * mean
    fx = float(np.float32(fix))
    model, sd = (mean / fx).to(torch.float32), (torch.sqrt(var.clamp(min=0.0)) / fx).to(torch.float32)
    return torch.where(have, model, prior), torch.where(have, sd, 0.0)


def workload(c, n, L, min_n, seed=5):
    """time_refit.py's chain up to levels_fit -> (pairs, hit, n_levels, levels, fit, target, target_len, W, locate)"""
    dev = c.device
    lens = (c.synth_lengths(seed, 0, n) // 32 * 32).to(torch.int32)
    opts, comp, coff, csize, off, size32 = compressed(c, lens, seed)
    sg = batch.Segmentation(3, 6, 4.0, 9.0, 2)
    cap = int((lens.to(torch.int64) // (sg.radius + 1) + 2).sum())
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    scale0, offset0 = torch.full((n,), SCALE, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
    gen = torch.Generator(device="cpu").manual_seed(seed + 1)
    stride = (L + 15) // 16 * 16
    target = torch.clamp(torch.randint(-75, 113, (G, stride // 3 + 1), generator=gen).repeat_interleave(3, dim=1)[:, :stride]
                         + torch.randint(-3, 4, (G, stride), generator=gen), -127, 127).to(torch.int8).to(dev)
    t_len = torch.full((G,), L, dtype=torch.int32, device=dev)
    lc = batch.Locate(N, QUANT)
    A = Tables(dev, n, cap)
    with torch.cuda.stream(c.stream):
        c.signal_segment(comp, coff, csize, off, size32, res, opts, sg, event_first=A.first, start=A.start)
        c.signal_events(comp, coff, csize, off, size32, res, opts, A.first, A.start, scale=scale0, offset=offset0, moments=A.mom, arena=A.rec)
        c.events_query(A.first, A.rec, N, min_n=min_n, result=res, index=A.index, query=A.query, valid=A.valid)
        c.locate_span(A.query, A.valid, target, t_len, lc, out=A.spans)
        c.match_best(A.spans, out=A.pairs)
    torch.cuda.synchronize()
    tb = A.pairs.cpu().numpy().view(np.uint32)
    widths = (tb[:, 3] - tb[:, 2])[tb[:, 1] != 0xFFFFFFFF]
    W = max(8, (int(widths.max()) + 7) // 8 * 8)
    A.levels(dev, n, W)
    with torch.cuda.stream(c.stream):
        c.locate_path(A.query, A.valid, target, t_len, A.pairs, W, lc, hit=A.hit, rows=A.rows)
        c.locate_levels(A.pairs, A.hit, A.rows, A.first, A.start, A.rec, A.mom, W, index=A.index, n_levels=A.n_levels, levels=A.lv)
        fit = c.levels_fit(A.pairs, A.hit, A.n_levels, A.lv, target, t_len, n, lc, min_samples=min_n)[0]
    torch.cuda.synchronize()
    return A.pairs, A.hit, A.n_levels, A.lv, fit, target, t_len, W, lc


def pile_case(c, tables, n, reps, min_n, Gn):
    """levels_pile over Gn targets: the workload's own (Gn = G) or the same pairs dealt over Gn rows"""
    pairs, hit, n_levels, lv, fit, target, t_len, W, lc = tables
    dev, stride, L = c.device, int(target.shape[1]), int(t_len[0])
    if Gn != G:
        pairs = pairs.clone()
        won = pairs[:, 1] != -1
        pairs[:, 1] = torch.where(won, torch.arange(n, device=dev, dtype=torch.int32) % Gn, pairs[:, 1])
        target, t_len = torch.zeros((Gn, stride), dtype=torch.int8, device=dev), torch.full((Gn,), L, dtype=torch.int32, device=dev)
    pile = torch.empty((4, Gn, stride), dtype=torch.int64, device=dev)
    out = [torch.empty((n, 4), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)]
    un = {}

    def fused():
        c.levels_pile(pairs, hit, n_levels, lv, target, t_len, n, fix=FIX, fit=fit, require_ok=True, clear=True, locate=lc, min_samples=min_n, pile=pile)

    def fit_alone():
        c.levels_fit(pairs, hit, n_levels, lv, target, t_len, n, lc, min_samples=min_n, out=out[0], offset=out[1], scale=out[2])

    def unfused():
        un["pile"] = unfused_pile(pairs, hit, n_levels, lv, fit, t_len, Gn, stride, FIX, min_n, 0, True)

    legs = {"levels_pile": fused, "unfused_pile": unfused, "clear_alone": lambda: c.levels_pile(pairs[:0], hit[:0], n_levels[:0], lv[:0], target, t_len, n, fix=FIX,
                                                                                               clear=True, locate=lc, pile=pile)}
    if Gn == G:
        legs["levels_fit"] = fit_alone
    ms = timed(c, legs, reps)
    with torch.cuda.stream(c.stream):
        fused()
    torch.cuda.synchronize()
    assert torch.equal(pile.reshape(4, -1), un["pile"]), "levels_pile != the unfused route"
    word = pile[0].reshape(-1)
    kept, skipped = int((word & 0xFFFFFFFF).sum()), int((word >> 32).sum())
    added = 32 * kept + 8 * skipped
    adds_ms = max(ms["levels_pile"] - ms["clear_alone"], 1e-6)
    return {"pairs": n, "targets": Gn, "levels": L, "max_width": W, "kept": kept, "skipped": skipped, "depth_mean": round(kept / max(int((word != 0).sum()), 1), 1),
            "ms": ms, "bytes_added": added, "added_GB_per_s": round(added / ms["levels_pile"] / 1e6, 1),
            "added_GB_per_s_without_the_clear": round(added / adds_ms / 1e6, 1), "float_adds_GB_per_s_of_the_guide": 1300.0,
            "records_GB_per_s": round((kept + skipped) * 32 / ms["levels_pile"] / 1e6, 1), "unfused_over_fused": round(ms["unfused_pile"] / ms["levels_pile"], 2),
            "checked_bit_for_bit": True}, pile


def kmers_case(c, Gn, L, k, reps, seed=11):
    dev = c.device
    rng = np.random.default_rng(seed + k)
    bases, T = L + k - 1, (L + 15) // 16 * 16
    stride = (bases + 16) // 16 * 16
    seq_h = np.full((Gn, stride), 0x4E, np.uint8)
    seq_h[:, :bases] = rng.choice(np.frombuffer(b"ACGT", np.uint8), (Gn, bases))
    seq_h[:, rng.integers(0, bases, 20)] = 0x4E   # a few Ns
    seq, seq_len = torch.from_numpy(seq_h).to(dev), torch.full((Gn,), bases, dtype=torch.int32, device=dev)
    lut = torch.from_numpy(R.CODE.astype(np.int64)).to(dev)
    kmer, kmer_len = torch.empty((Gn, T), dtype=torch.int32, device=dev), torch.empty(Gn, dtype=torch.int32, device=dev)
    un = {}

    def unfused():
        un["kmer"] = unfused_kmers(seq, [bases] * Gn, lut, k, T)

    ms = timed(c, {"squiggle_kmers": lambda: c.squiggle_kmers(seq, seq_len, k, T, kmer=kmer, target_len=kmer_len), "unfused_kmers": unfused}, reps)
    torch.cuda.synchronize()
    assert torch.equal(kmer, un["kmer"]) and kmer_len.tolist() == [L] * Gn, "squiggle_kmers != the unfused route"
    return {"rows": Gn, "levels": L, "k": k, "ms": ms, "unfused_over_fused": round(ms["unfused_kmers"] / ms["squiggle_kmers"], 2), "checked_bit_for_bit": True}, kmer, kmer_len


def pile_kmers_case(c, pile, kmer, kmer_len, k, reps, min_obs=8):
    dev = c.device
    kp, kd = torch.empty((4, 4 ** k), dtype=torch.int64, device=dev), torch.empty((4, 4 ** k), dtype=torch.int64, device=dev)
    prior = torch.randn(4 ** k, device=dev)
    model, sd = torch.empty(4 ** k, dtype=torch.float32, device=dev), torch.empty(4 ** k, dtype=torch.float32, device=dev)
    un = {}

    def unfused():
        un["kp"] = unfused_pile_kmers(pile, kmer, kmer_len, k)

    def unfused_up():
        un["model"] = unfused_update(kp, prior, FIX, min_obs)

    with torch.cuda.stream(c.stream):
        c.pile_kmers(pile, kmer, kmer_len, k, clear=True, kmer_pile=kp)
    legs = {"pile_kmers": lambda: c.pile_kmers(pile, kmer, kmer_len, k, clear=True, kmer_pile=kp),
            "pile_kmers_direct": lambda: c.pile_kmers(pile, kmer, kmer_len, k, clear=True, direct=True, kmer_pile=kd), "unfused_pile_kmers": unfused,
            "model_update": lambda: c.model_update(kp, prior, k, fix=FIX, min_obs=min_obs, sd=sd, model=model), "unfused_update": unfused_up}
    ms = timed(c, legs, reps)
    torch.cuda.synchronize()
    assert torch.equal(kp, un["kp"]) and torch.equal(kd, un["kp"]), "pile_kmers != the unfused route"
    assert torch.equal(model.view(torch.int32), un["model"][0].view(torch.int32)) and torch.equal(sd.view(torch.int32), un["model"][1].view(torch.int32)), "model_update"
    return {"k": k, "rows": int(kmer.shape[0]), "table_in_LDS": k <= LDS_KMAX, "kmers_observed": int(((kp[0] & 0xFFFFFFFF) >= min_obs).sum()), "ms": ms,
            "unfused_over_fused": round(ms["unfused_pile_kmers"] / ms["pile_kmers"], 2), "update_unfused_over_fused": round(ms["unfused_update"] / ms["model_update"], 2),
            "checked_bit_for_bit": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--levels", type=int, default=30000)
    ap.add_argument("--min-n", type=int, default=4)
    ap.add_argument("--spread", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    tables = workload(c, args.reads, args.levels, args.min_n)
    out = {"levels_pile": [], "squiggle_kmers": [], "pile_kmers": []}
    piles = {}
    for Gn in (G, args.spread):
        r, piles[Gn] = pile_case(c, tables, args.reads, args.reps, args.min_n, Gn)
        out["levels_pile"].append(r)
    for Gn, ks in ((G, (1, 5, 6, 9)), (args.spread, (5, 6))):
        for k in ks:
            r, kmer, kmer_len = kmers_case(c, Gn, args.levels, k, args.reps)
            out["squiggle_kmers"].append(r)
            out["pile_kmers"].append(pile_kmers_case(c, piles[Gn], kmer, kmer_len, k, args.reps))
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
