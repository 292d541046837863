#!/usr/bin/env python3
"""Cost of the fused segmentation (vbz_gpu_signal_segment_batch) against its floor and the unfused route, alternating in one process.

Workload: --reads reads of ~100 k int16 samples (the lengths of SURVEY.md 8d, rounded down to 32), each a step signal: plateaus of random
dwell 3 ... 30 at levels in [-600, 900] under Gaussian noise of 6 counts, synthesised on the device and compressed once.  Each behind
untimed warm-up calls and timed with HIP events on the codec's stream (median of --reps calls):
  i16        the int16 decode alone: the floor -- no sample need be stored, but every sample must be decoded
  segment    the fused call: event_first and start
  seg+events the fused call followed by the event call on its tables (records and moments)
  unfused    the int16 decode, then torch: int64 cumulative sums of x and x^2 over the arena, both detectors' N and D as differences,
             float64 scores, max_pool1d over the r scores on either side, nonzero, and the sort that puts row 0 in front of every
             read's boundaries -- in blocks of whole reads below 2^26 samples
Every event_first and start of the fused call is checked bit for bit against the unfused route in the same run, and --sample reads
against tests/segment_ref.py on the host.  Then one 20 M-sample read, the same (one workgroup walks it: DESIGN.md 4.20).

    python tools/time_segment.py [--reads 8192] [--reps 20] [--sample 24] [--profile]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import segment_ref as S  # noqa: E402
from vbz_compression_amd import batch  # noqa: E402

BLOCK = 1 << 26
GAP = 64   # samples between two reads' slots: no neighbourhood of the unfused route reaches from one read into the next (r <= 32)


def timed(c, fns, reps, warm=2):
    """median milliseconds of every fn, the fns alternating call by call"""
    ms = {k: [] for k in fns}
    with torch.cuda.stream(c.stream):
        for _ in range(warm):
            for f in fns.values():
                f()
        for _ in range(reps):
            for k, f in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}


def step_signal(dev, total, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    d = torch.randint(3, 31, (total // 3 + 1,), generator=g, device=dev, dtype=torch.int64)
    level = torch.rand(d.numel(), generator=g, device=dev) * 1500 - 600
    x = torch.repeat_interleave(level, d)[:total] + torch.randn(total, generator=g, device=dev) * 6.0
    return x.round().clamp(-32768, 32767).to(torch.int16)


def case(c, lens, reps, seed, sg, sample, profile=False):
    dev = c.device
    n = int(lens.numel())
    opts = c.options(True, 2, 1, 1)
    lens64 = lens.to(torch.int64)
    total = int(lens64.sum())
    with torch.cuda.stream(c.stream):
        raw16 = step_signal(dev, total, seed)   # (contiguous: every length is a multiple of 32 samples)
        sizes = lens64 * 2
        off = torch.cumsum(sizes, 0) - sizes
        caps = torch.tensor([c.L.vbz_max_compressed_size(int(s), ctypes.byref(opts)) for s in sizes.cpu().tolist()], dtype=torch.int64)
        coff, ctotal = batch.layout(caps, 64)
        comp = torch.empty(ctotal, dtype=torch.uint8, device=dev)
        coff = coff.to(dev)
        csize = torch.zeros(n, dtype=torch.int32, device=dev)
        c.compress(raw16.view(torch.uint8), off, sizes.to(torch.int32), comp, coff, caps.to(torch.int32).to(dev), csize, opts)
    torch.cuda.synchronize()
    host_reads = {i: raw16[int(off[i]) // 2 : int(off[i]) // 2 + int(lens[i])].cpu().numpy() for i in np.linspace(0, n - 1, min(sample, n)).astype(int).tolist()}
    del raw16
    size32 = sizes.to(torch.int32)
    stride = lens64 + GAP
    base = torch.cumsum(stride, 0) - stride          # the slots' first samples in the int16 arena
    doff = base * 2
    atotal = int(stride.sum())
    arena16 = torch.zeros(atotal, dtype=torch.int16, device=dev)
    dst = arena16.view(torch.uint8)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    cap = int((lens64 // (sg.radius + 1) + 2).sum())
    first = torch.empty(n + 1, dtype=torch.int64, device=dev)
    start = torch.empty(cap, dtype=torch.int32, device=dev)
    rec = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    mom = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    base_h, lens_h = base.cpu().tolist(), lens64.cpu().tolist()
    blocks, a = [], 0
    while a < n:
        b = a + 1
        while b < n and base_h[b] + lens_h[b] + GAP - base_h[a] < BLOCK:
            b += 1
        blocks.append((a, b, base_h[a], base_h[b - 1] + lens_h[b - 1] + GAP))
        a = b
    r = sg.radius
    dets = [(sg.short_window, sg.short_threshold)] + ([(sg.long_window, sg.long_threshold)] if sg.long_window else [])
    u = {}

    def i16():
        c.decompress(comp, coff, csize, dst, doff, size32, res, opts)

    def fused():
        c.signal_segment(comp, coff, csize, doff, size32, res, opts, sg, event_first=first, start=start)

    def fused_events():
        fused()
        c.signal_events(comp, coff, csize, doff, size32, res, opts, first, start, moments=mom, arena=rec)

    def unfused():
        i16()
        keys = [torch.arange(n, device=dev, dtype=torch.int64)[lens64 > 0] << 32]   # row 0 of every read that has samples
        for ra, rb, lo, hi in blocks:
            x = arena16[lo:hi].to(torch.int64)
            L = hi - lo
            z1 = torch.zeros(1, dtype=torch.int64, device=dev)
            c1 = torch.cat([z1, torch.cumsum(x, 0)])
            c2 = torch.cat([z1, torch.cumsum(x * x, 0)])
            del x
            p = torch.arange(L, device=dev, dtype=torch.int64)
            rd = torch.searchsorted(base[ra:rb] - lo, p, right=True) - 1
            q = p - (base[ra:rb] - lo)[rd]
            Tq = lens64[ra:rb][rd]
            s = torch.zeros(L, dtype=torch.float64, device=dev)
            for w, t in dets:
                ok = (q >= w) & (q + w <= Tq)
                pl, ph = (p - w).clamp(min=0), (p + w).clamp(max=L)
                A, B = c1[p] - c1[pl], c1[ph] - c1[p]
                A2, B2 = c2[p] - c2[pl], c2[ph] - c2[p]
                N = w * (A - B) ** 2
                D = (w * (A2 + B2) - A * A - B * B).clamp(min=1)
                tt = float(np.float64(np.float32(t)) * np.float64(np.float32(t)))
                s = torch.maximum(s, torch.where(ok, (N.to(torch.float64) / D.to(torch.float64)) / tt, 0.0))
                del A, B, A2, B2, N, D, ok
            m = F.max_pool1d(F.pad(s, (r, r), value=-1.0)[None, None, :], r, 1)[0, 0]   # m[j] = max s[j - r ... j - 1]
            hit = torch.nonzero((s >= 1.0) & (s > m[:L]) & (s >= m[r + 1 : r + 1 + L]))[:, 0]
            keys.append(((rd[hit] + ra) << 32) + q[hit])
            del s, m, p, q, rd, Tq, c1, c2
        key = torch.sort(torch.cat(keys))[0]
        u["first"] = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(key >> 32, minlength=n), 0)])
        u["start"] = (key & 0xFFFFFFFF).to(torch.int32)

    fns = {"i16": i16, "segment": fused, "seg+events": fused_events, "unfused": unfused}
    ms = timed(c, fns, reps)
    torch.cuda.synchronize()
    rows = int(first[-1])
    assert torch.equal(res.to(torch.int64), lens64 * 2), "verdicts"
    assert torch.equal(first, u["first"]), "event_first != the unfused route"
    assert torch.equal(start[:rows], u["start"]), "start != the unfused route, bit for bit"
    first_h, start_h = first.cpu().numpy(), start[:rows].cpu().numpy().view(np.uint32)
    P = (sg.short_window, sg.long_window, sg.short_threshold, sg.long_threshold, sg.radius)
    for i, x in host_reads.items():
        assert start_h[first_h[i] : first_h[i + 1]].tolist() == S.starts(x, None, None, P).tolist(), ("segment_ref, read", i)
    phases = None
    if profile:   # the fused call's launches by the library's own labels
        c.profile(True)
        c.profile_reset()
        with torch.cuda.stream(c.stream):
            for _ in range(5):
                fused()
        torch.cuda.synchronize()
        phases = {k: round(v[1] / 5, 4) for k, v in c.profile_read().items()}
        c.profile(False)
    return {"reads": n, "samples": total, "rows": rows, "mean_dwell": round(total / max(rows, 1), 2), "ms": ms, "phases_ms": phases,
            "unfused_over_segment": round(ms["unfused"] / ms["segment"], 3), "segment_over_i16": round(ms["segment"] / ms["i16"], 3),
            "checked_against_unfused": True, "reads_checked_against_segment_ref": len(host_reads)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sample", type=int, default=24)
    ap.add_argument("--long", type=int, default=20_000_000, help="samples of the one long read (0: none)")
    ap.add_argument("--profile", action="store_true", help="also the fused call's launches by the library's labels")
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    sg = batch.Segmentation(3, 6, 4.0, 9.0, 2)
    lens = (c.synth_lengths(5, 0, args.reads) // 32 * 32).to(torch.int32)
    out = {"segmentation": [3, 6, 4.0, 9.0, 2], "headline": case(c, lens, args.reps, 5, sg, args.sample, args.profile)}
    print(json.dumps(out), flush=True)
    if args.long:
        torch.cuda.empty_cache()
        out["one_long_read"] = case(c, torch.tensor([args.long // 32 * 32], dtype=torch.int32, device=c.device), args.reps, 7, sg, 1, args.profile)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
