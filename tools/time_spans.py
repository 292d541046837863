#!/usr/bin/env python3
"""Cost of the fused span call (vbz_gpu_signal_spans_batch) against its floors, the trim call and the unfused route, alternating in one
process.

Workload: --reads reads of ~100 k int16 samples (the lengths of SURVEY.md 8d, rounded down to 32) of the synthetic signal, with three
open-pore plateaus (+900 counts, 20 ... 419 samples: above the threshold of ~ +700) and two single-sample spikes (+1 200: in, but dropped
by m) planted per read, synthesised on the device and
compressed once.  Settings: ABOVE, MED_MAD, f = 6, D = 50, m = 5.  Each behind untimed warm-up calls and timed with HIP events on the
codec's stream (median of --reps calls):
  i16          the int16 decode alone: a floor -- every sample must be decoded
  stats        the statistics-alone call (MED_MAD): the floor of the call with a normalisation
  trim         the trim call (the statistics, then the prefix pass)
  spans        the fused call with the normalisation: edge_first, edge and shift_scale
  spans_given  the fused call with given constants (the shift_scale of `stats` as level): no counting pass
  spans+events the fused call with given constants followed by the event call on its tables
  unfused      the statistics call and the int16 decode, then torch: float64 compare against the per-read threshold, nonzero, diff, the
               merge and the length filter, bincount and cumsum -- in blocks of whole reads below 2^26 samples
Every edge_first and edge of both fused calls is checked bit for bit against the unfused route in the same run, and --sample reads against
tests/spans_ref.py on the host.  Then one 20 M-sample read, the same (the span pass runs on its segments: DESIGN.md 4.21).

    python tools/time_spans.py [--reads 65536] [--reps 20] [--sample 24] [--profile]"""
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

import spans_ref as S  # noqa: E402
from vbz_compression_amd import batch  # noqa: E402

BLOCK = 1 << 26
PLANT = 4096


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


def plant(raw16, off16, lens):
    """per read i: plateaus of +900 over 20 + 37 i % 400 samples at 1/5, 1/2 and 4/5 of the read, and spikes of +1 200 at 1/3 and 2/3"""
    n, dev = int(lens.numel()), raw16.device
    ar = torch.arange(420, dtype=torch.int64, device=dev)[None, :]
    T = lens.to(torch.int64)
    for a in range(0, n, PLANT):
        b = min(n, a + PLANT)
        i = torch.arange(a, b, dtype=torch.int64, device=dev)
        width = torch.minimum(20 + (i * 37) % 400, T[a:b] // 8)[:, None]
        for num, den in ((1, 5), (1, 2), (4, 5)):
            at = off16[a:b] + T[a:b] * num // den
            raw16[(at[:, None] + ar)[ar < width]] += 900
        for num, den in ((1, 3), (2, 3)):
            at = (off16[a:b] + T[a:b] * num // den)[T[a:b] > 8]
            raw16[at] += 1200


def case(c, lens, reps, seed, sp, norm, sample, profile=False):
    dev = c.device
    n = int(lens.numel())
    opts = c.options(True, 2, 1, 1)
    lens64 = lens.to(torch.int64)
    total = int(lens64.sum())
    sizes = lens64 * 2
    off = torch.cumsum(sizes, 0) - sizes   # (contiguous: every length is a multiple of 32 samples)
    off16 = off // 2
    with torch.cuda.stream(c.stream):
        raw = torch.empty(total * 2, dtype=torch.uint8, device=dev)
        c.synth_signal(seed, 0, raw, off, lens)
        plant(raw.view(torch.int16), off16, lens)
        caps = torch.tensor([c.L.vbz_max_compressed_size(int(s), ctypes.byref(opts)) for s in sizes.cpu().tolist()], dtype=torch.int64)
        coff, ctotal = batch.layout(caps, 64)
        comp = torch.empty(ctotal, dtype=torch.uint8, device=dev)
        coff = coff.to(dev)
        csize = torch.zeros(n, dtype=torch.int32, device=dev)
        c.compress(raw, off, sizes.to(torch.int32), comp, coff, caps.to(torch.int32).to(dev), csize, opts)
    torch.cuda.synchronize()
    pick = np.linspace(0, n - 1, min(sample, n)).astype(int).tolist()
    host_reads = {i: raw.view(torch.int16)[int(off16[i]) : int(off16[i]) + int(lens[i])].cpu().numpy() for i in pick}
    del raw
    size32 = sizes.to(torch.int32)
    arena16 = torch.zeros(total, dtype=torch.int16, device=dev)
    dst = arena16.view(torch.uint8)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    cap = int(sum(sp.max_edges(t) for t in lens64.cpu().tolist()))
    tabs = {k: (torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)) for k in ("norm", "given")}
    ss = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    ss0 = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    begin = torch.zeros(n, dtype=torch.int32, device=dev)
    rec = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    mom = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    base_h, lens_h = off16.cpu().tolist(), lens64.cpu().tolist()
    blocks, a = [], 0
    while a < n:
        b = a + 1
        while b < n and base_h[b] + lens_h[b] - base_h[a] < BLOCK:
            b += 1
        blocks.append((a, b, base_h[a], base_h[b - 1] + lens_h[b - 1]))
        a = b
    D, m, f64 = sp.merge_gap, sp.min_length, float(np.float64(np.float32(sp.threshold_factor)))
    u = {}

    def i16():
        c.decompress(comp, coff, csize, dst, off, size32, res, opts)

    def stats():
        c.signal_norm(comp, coff, csize, off, size32, res, opts, norm, shift_scale=ss0)

    def trim():
        c.signal_trim(comp, coff, csize, off, size32, res, opts, norm, out=begin)

    def fused():
        c.signal_spans(comp, coff, csize, off, size32, res, opts, sp, norm=norm, shift_scale=ss, edge_first=tabs["norm"][0], edge=tabs["norm"][1])

    def given():
        c.signal_spans(comp, coff, csize, off, size32, res, opts, sp, level=ss0, edge_first=tabs["given"][0], edge=tabs["given"][1])

    def given_events():
        given()
        c.signal_events(comp, coff, csize, off, size32, res, opts, tabs["given"][0], tabs["given"][1], moments=mom, arena=rec)

    def unfused():
        stats()
        i16()
        thr = ss0[:, 0].double() + f64 * ss0[:, 1].double()
        counts = torch.zeros(n, dtype=torch.int64, device=dev)
        pairs = []
        for ra, rb, lo, hi in blocks:
            rd = torch.repeat_interleave(torch.arange(ra, rb, device=dev, dtype=torch.int64), lens64[ra:rb])
            hit = torch.nonzero(arena16[lo:hi].double() > thr[rd])[:, 0]   # (ascending positions of the block)
            if hit.numel() == 0:
                continue
            r = rd[hit]
            cut = torch.ones(hit.numel() + 1, dtype=torch.bool, device=dev)
            cut[1:-1] = (r[1:] != r[:-1]) | (hit[1:] - hit[:-1] - 1 > D)
            first, last = hit[cut[:-1]], hit[cut[1:]]
            keep = last + 1 - first >= m
            first, last, rk = first[keep], last[keep], r[cut[:-1]][keep]
            counts += torch.bincount(rk, minlength=n)
            q0 = lo - off16[rk]
            pairs.append(torch.stack([first + q0, last + 1 + q0], 1).reshape(-1))
            del rd, hit, r, cut
        u["first"] = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(2 * counts, 0)])
        u["edge"] = (torch.cat(pairs) if pairs else torch.zeros(0, dtype=torch.int64, device=dev)).to(torch.int32)

    fns = {"i16": i16, "stats": stats, "trim": trim, "spans": fused, "spans_given": given, "spans+events": given_events, "unfused": unfused}
    ms = timed(c, fns, reps)
    torch.cuda.synchronize()
    words = int(u["first"][-1])
    assert torch.equal(res.to(torch.int64), lens64 * 2), "verdicts"
    assert words >= 2 * n, ("the workload has fewer spans than reads: the planted plateaus are not in", words // 2, n)
    assert torch.equal(ss, ss0), "shift_scale of the span call != the statistics call's"
    for k, (first, edge) in tabs.items():
        assert torch.equal(first, u["first"]), ("edge_first != the unfused route", k)
        assert torch.equal(edge[:words], u["edge"]), ("edge != the unfused route, bit for bit", k)
    first_h, edge_h, ss_h = tabs["norm"][0].cpu().numpy(), tabs["norm"][1][:words].cpu().numpy().view(np.uint32), ss.cpu().numpy()
    P = (S.ABOVE, D, m, sp.ignore_prefix, sp.threshold_factor)
    for i, x in host_reads.items():
        assert edge_h[first_h[i] : first_h[i + 1]].tolist() == S.edges(x, None, None, P, ss_h[i][0], ss_h[i][1]).tolist(), ("spans_ref, read", i)
    phases = None
    if profile:   # both fused calls' launches by the library's own labels
        phases = {}
        for k, fn in (("spans", fused), ("spans_given", given), ("stats", stats), ("i16", i16)):
            c.profile(True)
            c.profile_reset()
            with torch.cuda.stream(c.stream):
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            phases[k] = {name: round(v[1] / 5, 4) for name, v in c.profile_read().items()}
            c.profile(False)
    return {"reads": n, "samples": total, "spans": words // 2, "edge_cap": cap, "ms": ms, "phases_ms": phases,
            "span_pass_and_emit_ms": round(ms["spans"] - ms["stats"], 4), "unfused_over_spans": round(ms["unfused"] / ms["spans"], 3),
            "spans_given_over_i16": round(ms["spans_given"] / ms["i16"], 3), "spans_over_stats": round(ms["spans"] / ms["stats"], 3),
            "checked_against_unfused": True, "reads_checked_against_spans_ref": len(host_reads)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sample", type=int, default=24)
    ap.add_argument("--long", type=int, default=20_000_000, help="samples of the one long read (0: none)")
    ap.add_argument("--profile", action="store_true", help="also the calls' launches by the library's labels")
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    sp = batch.Spans("above", 50, 5, 0, 6.0)
    lens = (c.synth_lengths(5, 0, args.reads) // 32 * 32).to(torch.int32)
    out = {"spans": ["above", 50, 5, 0, 6.0], "norm": "med_mad", "headline": case(c, lens, args.reps, 5, sp, batch.MED_MAD, args.sample, args.profile)}
    print(json.dumps(out), flush=True)
    if args.long:
        torch.cuda.empty_cache()
        out["one_long_read"] = case(c, torch.tensor([args.long // 32 * 32], dtype=torch.int32, device=c.device), args.reps, 7, sp, batch.MED_MAD, 1, args.profile)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
