#!/usr/bin/env python3
"""Cost of the two pore-model calls (vbz_gpu_squiggle_batch, vbz_gpu_levels_fit_batch) against the unfused torch route for each, and of
the chain with a second round under the fitted constants, the legs alternating in one process (median of --reps calls, HIP events on the
codec's stream, untimed warm-up calls first).

  squiggle       S = 2 sequences with BOTH (4 rows), 30 000 and 1 048 576 bases, k = 6 and 9, with the level arena
  unfused_squiggle   torch: a code table lookup, the rolling index by k shifted slices, one gather, the quantisation, per row
  levels_fit     on tools/time_eventalign.py's workload (--reads reads, N = 2 048, G = 2 targets of --levels levels), over the levels arena
                 the chain leaves
  unfused_fit    torch: a gather of the target levels, the masks, int64 sums and the float64 formula
  locate_levels, locate_span, locate_path      the calls the fit stands beside, alone
  round_two      events under the fitted offset / scale tables -> events_query -> locate_span
  chain_two_rounds   segment -> events -> events_query -> locate_span -> match_best -> locate_path -> locate_levels -> levels_fit -> round_two
Every table is checked bit for bit against the unfused route (round two against the same calls under the unfused route's tables), the
squiggle's against tests/squiggle_ref.py too.  Bytes moved are what the rule needs, from the shapes: the rate is bytes over the call's time.

    python tools/time_refit.py [--reads 8192] [--reps 20] [--levels 30000] [--out profiles/refit_time.json]"""
import argparse
import json
import os
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


def unfused_squiggle(seq, lens, lut, model, k, T, quant):
    """both strands of every sequence -> (target int8 [2 S, T], level float32 [2 S, T]); lens on the host"""
    dev, S = seq.device, int(seq.shape[0])
    target, level = torch.zeros((2 * S, T), dtype=torch.int8, device=dev), torch.zeros((2 * S, T), dtype=torch.float32, device=dev)
    for s in range(S):
        n = lens[s]
        fwd = lut[seq[s, :n].to(torch.int64)]
        for rc, c in ((0, fwd), (1, torch.where(fwd == 4, fwd, 3 - fwd).flip(0))):
            L = n - k + 1
            index, bad = torch.zeros(L, dtype=torch.int64, device=dev), torch.zeros(L, dtype=torch.bool, device=dev)
            for i in range(k):
                part = c[i:i + L]
                bad |= part == 4
                index = index * 4 + part.clamp(max=3)
            m = torch.where(bad, 0.0, model[index])
            v = m * quant
            q = torch.where(torch.isnan(v), 0.0, torch.clamp(torch.round(v), -127.0, 127.0))
            target[2 * s + rc, :L], level[2 * s + rc, :L] = torch.where(bad, 0.0, q).to(torch.int8), m
    return target, level


def squiggle_case(c, bases, k, reps, seed=7):
    dev, S = c.device, 2
    rng = np.random.default_rng(seed)
    stride = (bases + 16) // 16 * 16
    seq_h = np.full((S, stride), 0x4E, np.uint8)
    seq_h[:, :bases] = rng.choice(np.frombuffer(b"ACGT", np.uint8), (S, bases))
    seq_h[:, rng.integers(0, bases, 20)] = 0x4E   # a few Ns
    model_h = rng.normal(0, 1.5, 4 ** k).astype(np.float32)
    seq, seq_len, model = torch.from_numpy(seq_h).to(dev), torch.full((S,), bases, dtype=torch.int32, device=dev), torch.from_numpy(model_h).to(dev)
    lut = torch.from_numpy(R.CODE.astype(np.int64)).to(dev)
    out = [torch.empty((2 * S, stride), dtype=torch.int8, device=dev), torch.empty(2 * S, dtype=torch.int32, device=dev),
           torch.empty(2 * S, dtype=torch.int32, device=dev), torch.empty((2 * S, stride), dtype=torch.float32, device=dev)]
    u = {}

    def fused():
        c.squiggle(seq, seq_len, model, k, stride, quant=QUANT, both=True, level=out[3], target=out[0], target_len=out[1], masked=out[2])

    def unfused():
        u["t"] = unfused_squiggle(seq, [bases] * S, lut, model, k, stride, QUANT)

    ms = timed(c, {"squiggle": fused, "unfused_squiggle": unfused}, reps)
    torch.cuda.synchronize()
    assert torch.equal(out[0], u["t"][0]) and torch.equal(out[3].view(torch.int32), u["t"][1].view(torch.int32)), "squiggle != the unfused route"
    want = R.squiggle(seq_h, [bases] * S, model_h.view(np.uint32), k, stride, QUANT, R.BOTH)
    got = (out[0].cpu().numpy(), out[1].cpu().numpy().view(np.uint32), out[2].cpu().numpy().view(np.uint32), out[3].cpu().numpy().view(np.uint32))
    assert all((g == w).all() for g, w in zip(got, want)), "squiggle != tests/squiggle_ref.py"
    moved = 2 * S * bases + 2 * S * stride * 5 + 4 * 4 ** k   # each strand's bases read once, both arenas written whole, the model once
    return {"sequences": S, "bases": bases, "k": k, "rows": 2 * S, "masked": got[2].tolist(), "ms": ms, "bytes_moved": moved,
            "GB_per_s": round(moved / ms["squiggle"] / 1e6, 1), "unfused_over_fused": round(ms["unfused_squiggle"] / ms["squiggle"], 2),
            "checked_bit_for_bit": True}


def unfused_fit(pairs, hit, n_levels, lv, target, t_len, quant, min_samples, max_entries):
    dev, P, W = lv.device, int(lv.shape[0]), int(lv.shape[1])
    u = lambda t: t.to(torch.int64) & 0xFFFFFFFF   # noqa: E731
    ref, end, start, nl = u(pairs[:, 1]), u(hit[:, 1]), u(hit[:, 2]), u(n_levels)
    Gn, stride = int(target.shape[0]), int(target.shape[1])
    refc = ref.clamp(max=Gn - 1)
    Lg = u(t_len)[refc]
    valid = (ref < Gn) & (nl > 0) & (nl <= W) & (end > start) & (end - start == nl) & (Lg > 0) & (Lg <= stride) & (end <= Lg)
    t = torch.arange(W, device=dev)[None, :]
    live = (t < nl[:, None]) & valid[:, None]
    g = target[refc[:, None], (start[:, None] + t).clamp(max=stride - 1)].to(torch.int64)
    ns, ne, total = u(lv[..., 2]), u(lv[..., 3]), lv.view(torch.int64)[..., 2]
    keep = live & (ns >= max(min_samples, 1))
    if max_entries:
        keep &= ne <= max_entries
    m = total.to(torch.float64) / ns.clamp(min=1).to(torch.float64)
    keep &= m.abs() <= 32768.0
    q = torch.where(keep, torch.round(m * 64.0), 0.0).to(torch.int64)
    g = torch.where(keep, g, 0)
    K, Sg, Sgg, Sq, Sgq = keep.sum(1), g.sum(1), (g * g).sum(1), q.sum(1), (g * q).sum(1)
    num, den = K * Sgq - Sg * Sq, K * Sgg - Sg * Sg
    good = (K >= 2) & (den > 0) & (num > 0)
    f = torch.float64
    A = num.to(f) / torch.where(good, den, 1).to(f)
    B = (Sq.to(f) - A * Sg.to(f)) / K.clamp(min=1).to(f)
    a, b = A / 64.0, B / 64.0
    scale, offset = (1.0 / (a * float(np.float32(quant)))).to(torch.float32), (-b).to(torch.float32)
    ok = good & torch.isfinite(scale) & torch.isfinite(offset) & (scale > 0)
    offset, scale = torch.where(ok, offset, 0.0), torch.where(ok, scale, 1.0)
    out = torch.stack([offset.view(torch.int32), scale.view(torch.int32), K.to(torch.int32), ok.to(torch.int32)], 1)
    return out, offset, scale, torch.stack([Sg, Sgg, Sq, Sgq], 1)


def refit_case(c, n, reps, L, min_n, seed=5):
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
    A, B, C = Tables(dev, n, cap), Tables(dev, n, cap), Tables(dev, n, cap)   # round one, round two, round two under the unfused route's tables

    def round_one(t):
        c.signal_segment(comp, coff, csize, off, size32, res, opts, sg, event_first=t.first, start=t.start)
        c.signal_events(comp, coff, csize, off, size32, res, opts, t.first, t.start, scale=scale0, offset=offset0, moments=t.mom, arena=t.rec)
        c.events_query(t.first, t.rec, N, min_n=min_n, result=res, index=t.index, query=t.query, valid=t.valid)
        c.locate_span(t.query, t.valid, target, t_len, lc, out=t.spans)
        c.match_best(t.spans, out=t.pairs)

    with torch.cuda.stream(c.stream):
        round_one(A)
    torch.cuda.synchronize()
    tb = A.pairs.cpu().numpy().view(np.uint32)
    won = tb[:, 1] != 0xFFFFFFFF
    widths = (tb[:, 3] - tb[:, 2])[won]
    W = max(8, (int(widths.max()) + 7) // 8 * 8)
    A.levels(dev, n, W)
    fit = [torch.empty((n, 4), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
           torch.empty((n, 4), dtype=torch.int64, device=dev)]
    u = {}

    def levels():
        c.locate_path(A.query, A.valid, target, t_len, A.pairs, W, lc, hit=A.hit, rows=A.rows)
        c.locate_levels(A.pairs, A.hit, A.rows, A.first, A.start, A.rec, A.mom, W, index=A.index, n_levels=A.n_levels, levels=A.lv)

    def fit_alone():
        c.levels_fit(A.pairs, A.hit, A.n_levels, A.lv, target, t_len, n, lc, min_samples=min_n, sums=fit[3], out=fit[0], offset=fit[1], scale=fit[2])

    def fit_unfused():
        u["fit"] = unfused_fit(A.pairs, A.hit, A.n_levels, A.lv, target, t_len, QUANT, min_n, 0)

    def round_two(t, offset, scale):
        c.signal_events(comp, coff, csize, off, size32, res, opts, A.first, A.start, scale=scale, offset=offset, moments=t.mom, arena=t.rec)
        c.events_query(A.first, t.rec, N, min_n=min_n, result=res, index=t.index, query=t.query, valid=t.valid)
        c.locate_span(t.query, t.valid, target, t_len, lc, out=t.spans)

    def chain():
        round_one(A)
        levels()
        fit_alone()
        round_two(B, fit[1], fit[2])

    with torch.cuda.stream(c.stream):
        chain()   # (the stage legs read the chain's tables)
    torch.cuda.synchronize()
    legs = {"chain_two_rounds": chain, "round_one": lambda: round_one(A), "round_two": lambda: round_two(B, fit[1], fit[2]),
            "locate_span": lambda: c.locate_span(A.query, A.valid, target, t_len, lc, out=C.spans),
            "locate_path": lambda: c.locate_path(A.query, A.valid, target, t_len, A.pairs, W, lc, hit=A.hit, rows=A.rows),
            "locate_levels": lambda: c.locate_levels(A.pairs, A.hit, A.rows, A.first, A.start, A.rec, A.mom, W, index=A.index, n_levels=A.n_levels, levels=A.lv),
            "levels_fit": fit_alone, "unfused_fit": fit_unfused}
    ms = timed(c, legs, reps)
    torch.cuda.synchronize()
    uo, uoff, usc, usum = u["fit"]
    assert torch.equal(uo, fit[0]) and torch.equal(usum, fit[3]), "levels_fit != the unfused route"
    assert torch.equal(uoff.view(torch.int32), fit[1].view(torch.int32)) and torch.equal(usc.view(torch.int32), fit[2].view(torch.int32)), "offset / scale"
    with torch.cuda.stream(c.stream):
        round_two(C, uoff, usc)
    torch.cuda.synchronize()
    total = int(A.first[-1])
    for name in ("query", "valid", "index", "spans"):
        assert torch.equal(getattr(B, name).view(torch.int32), getattr(C, name).view(torch.int32)), ("round two under the unfused route's tables", name)
    assert torch.equal(B.rec[:total], C.rec[:total])
    fit_h, nl_h = fit[0].cpu().numpy().view(np.uint32), A.n_levels.cpu().numpy().view(np.uint32)
    one, two = A.spans.cpu().numpy().view(np.uint32), B.spans.cpu().numpy().view(np.uint32)
    best1, best2 = one[..., 0].min(1).astype(np.int64), two[..., 0].min(1).astype(np.int64)
    moved = int(nl_h.astype(np.int64).sum()) * 33 + n * (16 + 16 + 4 + 16 + 8 + 32)   # a record and a target level per level, the pair's tables
    return {"reads": n, "event_rows": total, "query_len": N, "min_n": min_n, "targets": G, "levels": L, "max_width": W, "winners": int(won.sum()),
            "levels_in_all": int(nl_h.astype(np.int64).sum()), "fits_ok": int(fit_h[:, 3].sum()), "used_median": float(np.median(fit_h[:, 2])),
            "cost_median_round_one_two": [float(np.median(best1)), float(np.median(best2))], "ms": ms, "levels_fit_bytes_moved": moved,
            "levels_fit_GB_per_s": round(moved / ms["levels_fit"] / 1e6, 1), "unfused_over_fused": round(ms["unfused_fit"] / ms["levels_fit"], 2),
            "checked_bit_for_bit": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--levels", type=int, default=30000)
    ap.add_argument("--min-n", type=int, default=4)
    ap.add_argument("--bases", type=int, nargs="*", default=[30000, 1048576])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    out = {"squiggle": [squiggle_case(c, b, k, args.reps) for b in args.bases for k in (6, 9)],
           "refit": refit_case(c, args.reads, args.reps, args.levels, args.min_n)}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
