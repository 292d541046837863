#!/usr/bin/env python3
"""Cost of the two event-space alignment calls (vbz_gpu_events_query_batch, vbz_gpu_locate_levels_batch) inside the chain they complete and
against the unfused route for each, the legs alternating in one process.

Workload: tools/time_segment.py's -- --reads step-signal reads of ~100 k int16 samples, plateaus of random dwell 3 ... 30 under noise,
compressed once -- segmented with (3, 6, 4, 9, 2); the event means, calibrated by 1 / 256, are the query: N = 2 048 events a read, events
of fewer than --min-n samples dropped; G = 2 targets of --levels int8 levels.  Each leg behind untimed warm-up calls and timed with HIP
events on the codec's stream (median of --reps calls):
  seg_events     segment -> events: the chain stopped before the first new call
  to_path        ... -> events_query -> locate_span -> match_best -> locate_path: the chain stopped before the second new call
  chain          ... -> locate_levels: eventalign, no host copy between the calls
  locate_span, locate_path      the locate legs the new calls stand beside, alone
  events_query   the first new call alone          unfused_query   torch: read numbers by repeat_interleave, ranks among the kept by cumsum,
                                                                   one scatter into the padded [n, N] arenas (boolean masks: a nonzero)
  locate_levels  the second new call alone         unfused_levels  torch: cumsum of n, S1, S2 over every pair's entries, two batched
                                                                   searchsorted over begin and end for k0 and k1, gathers (it trusts the path)
Every table the chain writes is checked bit for bit against the stopped chains' and the stage calls', both new calls against their unfused
routes, and --sample reads against tests/eventalign_ref.py on the host.

    python tools/time_eventalign.py [--reads 8192] [--reps 20] [--levels 30000] [--out profiles/eventalign_time.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import eventalign_ref as E  # noqa: E402
from time_segment import step_signal, timed  # noqa: E402
from vbz_compression_amd import batch  # noqa: E402

N, G, QUANT, SCALE = 2048, 2, 32.0, 1.0 / 256.0


def compressed(c, lens, seed):
    dev, n = c.device, int(lens.numel())
    opts = c.options(True, 2, 1, 1)
    lens64 = lens.to(torch.int64)
    with torch.cuda.stream(c.stream):
        raw16 = step_signal(dev, int(lens64.sum()), seed)
        sizes = lens64 * 2
        off = torch.cumsum(sizes, 0) - sizes
        caps = torch.tensor([c.L.vbz_max_compressed_size(int(s), ctypes.byref(opts)) for s in sizes.cpu().tolist()], dtype=torch.int64)
        coff, ctotal = batch.layout(caps, 64)
        comp = torch.empty(ctotal, dtype=torch.uint8, device=dev)
        coff = coff.to(dev)
        csize = torch.zeros(n, dtype=torch.int32, device=dev)
        c.compress(raw16.view(torch.uint8), off, sizes.to(torch.int32), comp, coff, caps.to(torch.int32).to(dev), csize, opts)
    torch.cuda.synchronize()
    return opts, comp, coff, csize, off, sizes.to(torch.int32)


class Tables:
    """one set of every table the chain writes"""

    def __init__(self, dev, n, cap):
        self.first = torch.empty(n + 1, dtype=torch.int64, device=dev)
        self.start = torch.empty(cap, dtype=torch.int32, device=dev)
        self.rec = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        self.mom = torch.zeros((cap, 2), dtype=torch.int64, device=dev)
        self.query = torch.empty((n, N), dtype=torch.float32, device=dev)
        self.valid = torch.empty(n, dtype=torch.int32, device=dev)
        self.index = torch.empty((n, N), dtype=torch.int32, device=dev)
        self.spans = torch.empty((n, G, 4), dtype=torch.int32, device=dev)
        self.pairs = torch.empty((n, 4), dtype=torch.int32, device=dev)
        self.hit = torch.empty((n, 4), dtype=torch.int32, device=dev)
        self.rows = torch.empty((n, N, 2), dtype=torch.int32, device=dev)

    def levels(self, dev, n, W):
        self.n_levels = torch.empty(n, dtype=torch.int32, device=dev)
        self.lv = torch.empty((n, W, 8), dtype=torch.int32, device=dev)


def unfused_query(first, total, rec, min_n, n):
    dev = rec.device
    rows = first[1:] - first[:-1]
    read = torch.repeat_interleave(torch.arange(n, device=dev), rows, output_size=total)
    keep = rec[:total, 2] >= min_n
    excl = torch.cumsum(keep, 0) - keep.to(torch.int64)            # kept rows in front of each row, over the whole table
    rank = excl - excl[first[:-1].clamp(max=total - 1)][read]     # ... in front of it within its read
    sel = keep & (rank < N)
    query = torch.zeros((n, N), dtype=torch.int32, device=dev)
    index = torch.zeros((n, N), dtype=torch.int32, device=dev)
    at = read[sel] * N + rank[sel]
    query.view(-1)[at] = rec[:total, 0][sel]
    index.view(-1)[at] = (torch.arange(total, device=dev) - first[:-1][read])[sel].to(torch.int32)
    ck = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(keep, 0)])
    valid = (ck[first[1:]] - ck[first[:-1]]).clamp(max=N).to(torch.int32)
    return query.view(torch.float32), valid, index


def unfused_levels(pairs, hit, rows, index, first, total, start, rec, mom, W):
    dev, P = rows.device, int(rows.shape[0])
    u = lambda t: t.to(torch.int64) & 0xFFFFFFFF   # noqa: E731
    read, end, begin, n = u(pairs[:, 0]), u(hit[:, 1]), u(hit[:, 2]), u(hit[:, 3])
    live = torch.arange(N, device=dev)[None, :] < n[:, None]
    far = 1 << 40
    b, e = torch.where(live, u(rows[..., 0]), far), torch.where(live, u(rows[..., 1]), far)
    j = begin[:, None] + torch.arange(W, device=dev)[None, :]
    k0, k1 = torch.searchsorted(e, j, right=True), torch.searchsorted(b, j, right=True)
    c = (first[read][:, None] + u(index[read])).clamp(max=total - 1)
    ev_n, st = torch.where(live, u(rec[:total, 2])[c], 0), u(start[:total])[c]
    z = torch.zeros((P, 1), dtype=torch.int64, device=dev)
    pn = torch.cat([z, torch.cumsum(ev_n, 1)], 1)
    p1 = torch.cat([z, torch.cumsum(torch.where(live, mom[:total, 0][c], 0), 1)], 1)
    p2 = torch.cat([z, torch.cumsum(torch.where(live, mom[:total, 1][c], 0), 1)], 1)
    ok = (torch.arange(W, device=dev)[None, :] < (end - begin)[:, None]) & (n > 0)[:, None]
    k0c, k1c = k0.clamp(max=N - 1), k1.clamp(min=1, max=N)
    out = torch.zeros((P, W, 4), dtype=torch.int64, device=dev)
    out[..., 0] = torch.gather(st, 1, k0c) | ((torch.gather(st + ev_n, 1, k1c - 1) & 0xFFFFFFFF) << 32)
    out[..., 1] = ((torch.gather(pn, 1, k1c) - torch.gather(pn, 1, k0c)) & 0xFFFFFFFF) | ((k1c - k0c) << 32)
    out[..., 2] = torch.gather(p1, 1, k1c) - torch.gather(p1, 1, k0c)
    out[..., 3] = torch.gather(p2, 1, k1c) - torch.gather(p2, 1, k0c)
    out = torch.where(ok[..., None], out, 0)
    return torch.where(n > 0, end - begin, 0).to(torch.int32), out.view(torch.int32).reshape(P, W, 8)


def case(c, n, reps, L, min_n, sample, seed=5):
    dev = c.device
    lens = (c.synth_lengths(seed, 0, n) // 32 * 32).to(torch.int32)
    opts, comp, coff, csize, off, size32 = compressed(c, lens, seed)
    sg = batch.Segmentation(3, 6, 4.0, 9.0, 2)
    cap = int((lens.to(torch.int64) // (sg.radius + 1) + 2).sum())
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    scale, offset = torch.full((n,), SCALE, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
    gen = torch.Generator(device="cpu").manual_seed(seed + 1)
    stride = (L + 15) // 16 * 16
    target = torch.clamp(torch.randint(-75, 113, (G, stride // 3 + 1), generator=gen).repeat_interleave(3, dim=1)[:, :stride]
                         + torch.randint(-3, 4, (G, stride), generator=gen), -127, 127).to(torch.int8).to(dev)
    t_len = torch.full((G,), L, dtype=torch.int32, device=dev)
    lc = batch.Locate(N, QUANT)
    A, B, C = Tables(dev, n, cap), Tables(dev, n, cap), Tables(dev, n, cap)   # chain, to_path, seg_events and the stage calls

    def seg_events(t):
        c.signal_segment(comp, coff, csize, off, size32, res, opts, sg, event_first=t.first, start=t.start)
        c.signal_events(comp, coff, csize, off, size32, res, opts, t.first, t.start, scale=scale, offset=offset, moments=t.mom, arena=t.rec)

    def to_path(t, W):
        seg_events(t)
        c.events_query(t.first, t.rec, N, min_n=min_n, result=res, index=t.index, query=t.query, valid=t.valid)
        c.locate_span(t.query, t.valid, target, t_len, lc, out=t.spans)
        c.match_best(t.spans, out=t.pairs)
        c.locate_path(t.query, t.valid, target, t_len, t.pairs, W, lc, hit=t.hit, rows=t.rows)

    # one untimed run: the rows in all, the widest winner
    with torch.cuda.stream(c.stream):
        seg_events(A)
        c.events_query(A.first, A.rec, N, min_n=min_n, result=res, index=A.index, query=A.query, valid=A.valid)
        c.locate_span(A.query, A.valid, target, t_len, lc, out=A.spans)
        c.match_best(A.spans, out=A.pairs)
    torch.cuda.synchronize()
    total = int(A.first[-1])
    tb = A.pairs.cpu().numpy().view(np.uint32)
    won = tb[:, 1] != 0xFFFFFFFF
    widths = (tb[:, 3] - tb[:, 2])[won]
    W = max(8, (int(widths.max()) + 7) // 8 * 8)
    for t in (A, B, C):
        t.levels(dev, n, W)
    u = {}

    def chain():
        to_path(A, W)
        c.locate_levels(A.pairs, A.hit, A.rows, A.first, A.start, A.rec, A.mom, W, index=A.index, n_levels=A.n_levels, levels=A.lv)

    def q_alone():
        c.events_query(A.first, A.rec, N, min_n=min_n, result=res, index=C.index, query=C.query, valid=C.valid)

    def q_unfused():
        u["query"] = unfused_query(A.first, total, A.rec, min_n, n)

    def lv_alone():
        c.locate_levels(A.pairs, A.hit, A.rows, A.first, A.start, A.rec, A.mom, W, index=A.index, n_levels=C.n_levels, levels=C.lv)

    def lv_unfused():
        u["levels"] = unfused_levels(A.pairs, A.hit, A.rows, A.index, A.first, total, A.start, A.rec, A.mom, W)

    def span_alone():
        c.locate_span(A.query, A.valid, target, t_len, lc, out=C.spans)

    def path_alone():
        c.locate_path(A.query, A.valid, target, t_len, A.pairs, W, lc, hit=C.hit, rows=C.rows)

    with torch.cuda.stream(c.stream):
        chain()   # (the stage legs read the chain's tables)
    torch.cuda.synchronize()
    legs = {"seg_events": lambda: seg_events(C), "to_path": lambda: to_path(B, W), "chain": chain, "locate_span": span_alone, "locate_path": path_alone,
            "events_query": q_alone, "unfused_query": q_unfused, "locate_levels": lv_alone, "unfused_levels": lv_unfused}
    ms = timed(c, legs, reps)
    torch.cuda.synchronize()
    # bit for bit: the chain against the stopped chains, the stage calls and the unfused routes
    assert torch.equal(res.to(torch.int64), lens.to(torch.int64) * 2), "verdicts"
    for name in ("first", "query", "valid", "index", "spans", "pairs", "hit", "rows"):
        assert torch.equal(getattr(A, name), getattr(B, name)), ("the chain stopped before locate_levels", name)
    assert torch.equal(A.first, C.first) and torch.equal(A.start[:total], C.start[:total]) and torch.equal(A.rec[:total], C.rec[:total])
    assert torch.equal(A.mom[:total], C.mom[:total]), "the chain stopped before events_query"
    for name in ("query", "valid", "index", "spans", "hit", "rows", "n_levels", "lv"):
        assert torch.equal(getattr(A, name).view(torch.int32), getattr(C, name).view(torch.int32)), ("the stage call", name)
    uq, uv, ui = u["query"]
    assert torch.equal(uq.view(torch.int32), A.query.view(torch.int32)) and torch.equal(uv, A.valid) and torch.equal(ui, A.index), "events_query != the unfused route"
    un, ul = u["levels"]
    assert torch.equal(un, A.n_levels) and torch.equal(ul, A.lv), "locate_levels != the unfused route"
    # a sample against the numpy statements
    first_h = A.first.cpu().numpy().astype(np.uint64)
    nl_h = A.n_levels.cpu().numpy().view(np.uint32)
    picks = np.linspace(0, n - 1, min(sample, n)).astype(int).tolist()
    for i in picks:
        lo, hi = int(first_h[i]), int(first_h[i + 1])
        rec_h = A.rec[lo:hi].cpu().numpy().view(np.uint32)
        fi = np.array([0, hi - lo], np.uint64)
        q, v, ix = E.events_query(fi, hi - lo, rec_h[:, 0], rec_h[:, 2], N, min_n)
        assert (A.query[i].cpu().numpy().view(np.uint32) == q[0]).all() and int(A.valid[i]) == int(v[0]) and (A.index[i].cpu().numpy().view(np.uint32) == ix[0]).all(), i
        pr = A.pairs[i].cpu().numpy().view(np.uint32).copy()
        pr[0] = 0
        wn, wl = E.levels(pr[None], A.hit[i].cpu().numpy().view(np.uint32)[None], A.rows[i].cpu().numpy().view(np.uint32)[None], ix, fi, hi - lo,
                          A.start[lo:hi].cpu().numpy().view(np.uint32), rec_h[:, 2], A.mom[lo:hi].cpu().numpy().view(np.uint64), 1, N, W)
        assert nl_h[i] == wn[0] and (A.lv[i].cpu().numpy().view(np.uint32) == wl[0]).all(), i
    lv_h = A.lv[picks].cpu().numpy().view(np.uint32)
    ent = np.concatenate([lv_h[k, :nl_h[i], 3] for k, i in enumerate(picks)])
    valid_h = A.valid.cpu().numpy()
    return {"reads": n, "event_rows": total, "query_len": N, "min_n": min_n, "kept_median": float(np.median(valid_h)), "reads_cut_at_N": int((valid_h == N).sum()),
            "targets": G, "levels": L, "max_width": W, "winners": int(won.sum()), "winner_width_median_max": [float(np.median(widths)), int(widths.max())],
            "entries_per_level_mean_max_in_sample": [round(float(ent.mean()), 2), int(ent.max())], "ms": ms,
            "new_calls_in_chain_ms": {"events_query": round(ms["to_path"] - ms["seg_events"] - ms["locate_span"] - ms["locate_path"], 3),
                                      "locate_levels": round(ms["chain"] - ms["to_path"], 3)},
            "unfused_over_fused": {"events_query": round(ms["unfused_query"] / ms["events_query"], 2),
                                   "locate_levels": round(ms["unfused_levels"] / ms["locate_levels"], 2)},
            "checked_bit_for_bit": True, "reads_checked_against_eventalign_ref": len(picks)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--levels", type=int, default=30000)
    ap.add_argument("--min-n", type=int, default=4)
    ap.add_argument("--sample", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    out = {"segmentation": [3, 6, 4.0, 9.0, 2], "headline": case(c, args.reads, args.reps, args.levels, args.min_n, args.sample)}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
