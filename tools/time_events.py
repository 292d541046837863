#!/usr/bin/env python3
"""Cost of the fused per-event reduction (vbz_gpu_signal_events_batch) against its floors and the unfused route, alternating in one process.

Workload: --reads synthetic reads (~100 k int16 samples each) compressed once; every read cut into events of random dwell
2 ... 30 samples (mean 16: a basecaller's move table at stride 5 ... 6 looks like that), the first event at sample 0.  Two kinds of constants:
  given     offset / scale tables per read
  med_mad   the read's own median / MAD (batch.MED_MAD), on the device in the same call
Each behind untimed warm-up calls and timed with HIP events on the codec's stream (median of --reps calls):
  i16       the int16 decode alone                           } the floors: no sample need be stored for events,
  stats     the statistics-alone call (med_mad only)         } but every sample must be decoded (and counted)
  events    the fused call, records and moments
  unfused   the int16 decode (and the statistics call), then torch: int64 cumulative sums of x and x^2 over the arena, the moments as
            differences at the events' ends, the record in float64 by the header's formulas -- in blocks of whole reads below 2^27 samples
            (three 8-byte temporaries per sample).  The events' end positions in the arena are precomputed outside the timing.
Every fused output is checked in the same run: n, both moments and the mean bit for bit against the unfused one; the sd bit for bit
against numpy's correctly rounded sqrt over the unfused moments, and the rows where torch's float64 sqrt gives other bits are counted.  Then one 20 M-sample
read (the large-read path), the same.

    python tools/time_events.py [--reads 8192] [--reps 20] [--profile]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vbz_compression_amd import batch  # noqa: E402

DWELL_LO, DWELL_HI = 2, 30
BLOCK = 1 << 27


def timed(c, fns, reps, warm=3):
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


def event_lists(c, lens, seed):
    """(event_first int64 [n + 1], start int32 [rows]) -- dwells drawn over the concatenated reads, a start at 0 of every read"""
    dev = c.device
    n = int(lens.numel())
    lens64 = lens.to(torch.int64)
    end = torch.cumsum(lens64, 0)
    total = int(end[-1])
    g = torch.Generator(device=dev).manual_seed(seed)
    d = torch.randint(DWELL_LO, DWELL_HI + 1, (total // DWELL_LO + 1,), generator=g, device=dev, dtype=torch.int64)
    pos = torch.cumsum(d, 0)
    pos = pos[pos < total]
    rd = torch.searchsorted(end, pos, right=True)
    key = torch.unique(torch.cat([rd * (1 << 32) + (pos - (end - lens64)[rd]), torch.arange(n, device=dev, dtype=torch.int64) * (1 << 32)]))
    counts = torch.bincount(key >> 32, minlength=n)
    first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    first[1:] = torch.cumsum(counts, 0)
    return first, (key & 0xFFFFFFFF).to(torch.int32).contiguous()


def case(c, lens, reps, seed, profile=False):
    dev = c.device
    n = int(lens.numel())
    opts = c.options(True, 2, 1, 1)
    with torch.cuda.stream(c.stream):
        sizes = lens.to(torch.int64) * 2
        off, total = batch.layout(sizes.cpu(), 64)
        off = off.to(dev)
        raw = torch.zeros(total, dtype=torch.uint8, device=dev)
        c.synth_signal(seed, 0, raw, off, lens)
        caps = torch.tensor([c.L.vbz_max_compressed_size(int(s), ctypes.byref(opts)) for s in sizes.cpu().tolist()], dtype=torch.int64)
        coff, ctotal = batch.layout(caps, 64)
        comp = torch.empty(ctotal, dtype=torch.uint8, device=dev)
        coff = coff.to(dev)
        csize = torch.zeros(n, dtype=torch.int32, device=dev)
        c.compress(raw, off, sizes.to(torch.int32).to(dev), comp, coff, caps.to(torch.int32).to(dev), csize, opts)
    torch.cuda.synchronize()
    del raw
    size32 = sizes.to(torch.int32).to(dev)
    first, start = event_lists(c, lens, seed)
    rows = int(first[-1])
    g = torch.Generator().manual_seed(seed)
    o_t = (torch.rand(n, generator=g) * 400 - 200).to(dev)
    s_t = (torch.rand(n, generator=g) * 0.3 + 0.05).to(dev)
    arena16 = torch.zeros(total // 2, dtype=torch.int16, device=dev)   # (zeroed once: the gaps between slots add nothing to a cumulative sum)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    # the events' ends in the arena, per row: [a, z) in int16 positions, and the blocks of whole reads
    counts = first[1:] - first[:-1]
    rd = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), counts)
    T = lens.to(torch.int64)[rd]
    st = start.to(torch.int64)
    nxt = torch.cat([st[1:], st[:1]])
    last = torch.ones(rows, dtype=torch.bool, device=dev)
    last[:-1] = rd[1:] != rd[:-1]
    base = (off // 2)[rd]
    a_abs = base + torch.minimum(st, T)
    z_abs = base + torch.where(last, T, torch.minimum(nxt, T))
    off_h, lens_h, first_h = (off // 2).cpu().tolist(), lens.cpu().tolist(), first.cpu().tolist()
    blocks, a = [], 0
    while a < n:
        b = a + 1
        while b < n and off_h[b] + lens_h[b] - off_h[a] < BLOCK:
            b += 1
        blocks.append((off_h[a], off_h[b - 1] + lens_h[b - 1], first_h[a], first_h[b]))
        a = b
    del T, st, nxt, last, base
    arena = torch.empty((rows, 4), dtype=torch.int32, device=dev)
    mom = torch.empty((rows, 2), dtype=torch.int64, device=dev)
    u_mean, u_sd = torch.empty(rows, dtype=torch.float32, device=dev), torch.empty(rows, dtype=torch.float32, device=dev)
    u_n, u_mom = torch.empty(rows, dtype=torch.int64, device=dev), torch.empty((rows, 2), dtype=torch.int64, device=dev)
    ss = torch.empty((n, 2), dtype=torch.float32, device=dev)
    ss2 = torch.empty((n, 2), dtype=torch.float32, device=dev)
    dst = arena16.view(torch.uint8)

    def i16():
        c.decompress(comp, coff, csize, dst, off, size32, res, opts)

    def stats():
        c.signal_norm(comp, coff, csize, off, size32, res, opts, batch.MED_MAD, shift_scale=ss2)

    def reduce(o, s):
        for lo, hi, r0, r1 in blocks:
            if r1 == r0:
                continue
            x = arena16[lo:hi].to(torch.int64)
            z1 = torch.zeros(1, dtype=torch.int64, device=dev)
            c1 = torch.cat([z1, torch.cumsum(x, 0)])
            c2 = torch.cat([z1, torch.cumsum(x * x, 0)])
            ia, iz = a_abs[r0:r1] - lo, z_abs[r0:r1] - lo
            cnt = iz - ia
            S1, S2 = c1[iz] - c1[ia], c2[iz] - c2[ia]
            nd = cnt.clamp(min=1).to(torch.float64)
            m = S1.to(torch.float64) / nd
            v = (S2.to(torch.float64) / nd - m * m).clamp(min=0.0)
            od, sd_ = o[rd[r0:r1]].to(torch.float64), s[rd[r0:r1]].to(torch.float64)
            live = cnt > 0
            u_mean[r0:r1] = torch.where(live, ((m + od) * sd_).to(torch.float32), 0.0)
            u_sd[r0:r1] = torch.where(live, (torch.sqrt(v) * sd_.abs()).to(torch.float32), 0.0)
            u_n[r0:r1] = cnt
            u_mom[r0:r1, 0], u_mom[r0:r1, 1] = S1, S2

    def check(what, s):
        """n, both moments and the mean bit for bit against the unfused route on the device.  The sd likewise where torch's float64 sqrt
        is correctly rounded; the rows where the two differ are counted, and every sd is then held bit for bit to numpy's sqrt (which
        is) over the unfused route's moments on the host.  -> rows whose sd differs from torch's"""
        torch.cuda.synchronize()
        assert torch.equal(res.to(torch.int64), lens.to(torch.int64) * 2), what
        assert torch.equal(arena[:, 2].to(torch.int64), u_n) and bool((arena[:, 3] == 0).all()), "%s: n" % what
        assert torch.equal(mom, u_mom), "%s: moments" % what
        assert torch.equal(arena[:, 0], u_mean.view(torch.int32)), "%s: mean != the unfused route, bit for bit" % what
        differ = int((arena[:, 1] != u_sd.view(torch.int32)).sum())
        cnt = u_n.cpu().numpy()
        nd = np.maximum(cnt, 1).astype(np.float64)
        m = u_mom[:, 0].cpu().numpy().astype(np.float64) / nd
        v = u_mom[:, 1].cpu().numpy().astype(np.float64) / nd - m * m
        sd = np.sqrt(np.where(v < 0.0, 0.0, v)) * np.abs(s[rd].cpu().numpy().astype(np.float64))
        sd = np.where(cnt > 0, sd.astype(np.float32), np.float32(0.0))
        assert (arena[:, 1].cpu().numpy().view(np.uint32) == sd.view(np.uint32)).all(), "%s: sd != numpy over the unfused moments, bit for bit" % what
        return differ

    row = {"reads": n, "samples": int(lens.to(torch.int64).sum()), "rows": rows, "mean_dwell": round(int(lens.to(torch.int64).sum()) / max(rows, 1), 2)}

    def fused_given():
        c.signal_events(comp, coff, csize, off, size32, res, opts, first, start, scale=s_t, offset=o_t, moments=mom, arena=arena)

    def unfused_given():
        i16()
        reduce(o_t, s_t)

    ms = timed(c, {"i16": i16, "events": fused_given, "unfused": unfused_given}, reps)
    differ = check("given", s_t)
    phases = None
    if profile:   # the fused call's launches by the library's own labels (HIP events around every launch: the sum exceeds the call's time)
        c.profile(True)
        c.profile_reset()
        with torch.cuda.stream(c.stream):
            for _ in range(5):
                fused_given()
        torch.cuda.synchronize()
        phases = {k: round(v[1] / 5, 4) for k, v in c.profile_read().items()}
        c.profile(False)
    row["given"] = {"ms": ms, "phases_ms": phases, "sd_rows_unlike_torch_sqrt": differ, "unfused_over_events": round(ms["unfused"] / ms["events"], 3), "events_over_i16": round(ms["events"] / ms["i16"], 3), "checked": True}

    def fused_norm():
        c.signal_events(comp, coff, csize, off, size32, res, opts, first, start, norm=batch.MED_MAD, norm_out=ss, moments=mom, arena=arena)

    def unfused_norm():
        stats()
        i16()
        reduce(-ss2[:, 0], (1.0 / ss2[:, 1].to(torch.float64)).to(torch.float32))

    ms = timed(c, {"i16": i16, "stats": stats, "events": fused_norm, "unfused": unfused_norm}, reps)
    differ = check("med_mad", (1.0 / ss2[:, 1].to(torch.float64)).to(torch.float32))
    assert torch.equal(ss.view(torch.int32), ss2.view(torch.int32)), "shift_scale != the statistics call's"
    row["med_mad"] = {"ms": ms, "sd_rows_unlike_torch_sqrt": differ, "unfused_over_events": round(ms["unfused"] / ms["events"], 3), "events_over_stats": round(ms["events"] / ms["stats"], 3),
                      "checked": True}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile", action="store_true", help="also the fused call's launches by the library's labels (given constants)")
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    out = {"headline": case(c, c.synth_lengths(5, 0, args.reads), args.reps, 5, args.profile)}
    torch.cuda.empty_cache()
    out["one_20M_read"] = case(c, torch.tensor([20_000_000], dtype=torch.int32, device=c.device), args.reps, 7, args.profile)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
