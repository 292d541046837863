#!/usr/bin/env python3
"""Cost of finding every read's trim point on the device (vbz_gpu_signal_trim_batch) against the statistics call it extends and against
the unfused route, alternating in one process.

Headline: 65 536 synthetic reads (~100 k int16 samples each) with a +300 plateau over their first 500 ... 3 499 samples,
compressed once; the default trim (W = 40, m = 3, t0 = 10, M = 8 000, f = 2.4); then, each behind untimed warm-up calls and timed with
HIP events on the codec's stream (median of --reps calls):
  stats_med_mad / stats_quantile   vbz_gpu_signal_norm_batch: the statistics alone (the code the trim call runs in front of its pass)
  trim_med_mad / trim_quantile     vbz_gpu_signal_trim_batch: the trim pass's cost is this minus the statistics call of the same run
  trim_chunks                      the trim call, then begin[] -- never copied to the host -- through vbz_gpu_range_samples_batch, the chunk
                                   layout and the ranged normalised chunk call (MED_MAD of signal[trim:], L = 10 000, S = 9 504, float16)
  unfused                          the route without the feature: the int16 decode, a torch median / MAD of every read (tools/time_norm.py), the
                                   windows' counts and the walk over them in torch, then the same layout and ranged chunk call
Then one 20 M-sample read (the large-read path), the same calls but the unfused one.  Every begin is checked against tests/trim_ref.py:
all of them over the reads' decoded first samples with the constants the call reports, and every --full-every-th read from its sorted
values alone; the torch walk of the unfused route against the device's table.

    python tools/time_trim.py [--reads 65536] [--reps 20] [--only trim_med_mad]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import norm_ref as R  # noqa: E402
import time_norm as TN  # noqa: E402
import trim_ref as T  # noqa: E402
from vbz_compression_amd import batch  # noqa: E402

L_, S_ = 10000, 9504
BLOCK = 4096
NORMS = {"med_mad": (R.BONITO, batch.MED_MAD), "quantile": (R.DORADO, batch.DORADO_QUANTILE)}


def add_plateaus(raw16, off16, lens):
    """+300 over the first 500 + 37 i % 3000 samples of read i (cut at the read's length)"""
    n = int(lens.numel())
    dev = raw16.device
    ar = torch.arange(3500, dtype=torch.int64, device=dev)[None, :]
    for a in range(0, n, BLOCK):
        b = min(n, a + BLOCK)
        width = torch.minimum(500 + (torch.arange(a, b, dtype=torch.int64, device=dev) * 37) % 3000, lens[a:b].to(torch.int64))[:, None]
        idx = (off16[a:b][:, None] + ar)[ar < width]
        raw16[idx] += 300


def torch_trim(back16, off16, lens, shift, scale, p):
    """the rule of include/vbz_gpu.h over the int16 arena in torch: begin int32 [n]"""
    W, m, t0, M, f, mf, flags = p
    dev = back16.device
    n = int(lens.numel())
    Tn = lens.to(torch.int64)
    N = torch.clamp(Tn, max=M)
    nW = torch.where(N > t0, (N - t0) // W, torch.zeros_like(N))
    maxW = int(nW.max()) if n else 0
    none = torch.clamp(Tn, max=t0)
    out = none.clone()
    if maxW == 0:
        return out.to(torch.int32)
    thr = shift.double() + float(np.float64(np.float32(f))) * scale.double()
    ar = torch.arange(maxW * W, dtype=torch.int64, device=dev)[None, :]
    kk = torch.arange(maxW, dtype=torch.int64, device=dev)[None, :]
    for a in range(0, n, BLOCK):
        b = min(n, a + BLOCK)
        inside = ar < (nW[a:b] * W)[:, None]
        x = back16[torch.where(inside, off16[a:b][:, None] + t0 + ar, 0)].double()
        high = ((x > thr[a:b][:, None]) & inside).view(b - a, maxW, W)
        seen = torch.cumsum((high.sum(2) > m).to(torch.int32), 1) > 0
        stop = seen & ~high[:, :, -1] & (kk < nW[a:b][:, None])
        k = torch.argmax(stop.to(torch.int32), 1)
        e = t0 + (k + 1) * W
        reject = ~stop.any(1) | (e.double() > float(np.float64(np.float32(mf))) * Tn[a:b].double())
        if flags & T.REJECT_AT_END:
            reject |= e >= N[a:b]
        out[a:b] = torch.where(reject, none[a:b], e)
    return out.to(torch.int32)


def case(c, lens, reps, only, seed, unfused_leg, full_every, p=T.DEFAULT):
    dev = c.device
    n = int(lens.numel())
    opts = c.options(True, 2, 1, 1)
    trim = batch.Trim(*p[:6], reject_at_end=bool(p[6]))
    with torch.cuda.stream(c.stream):
        sizes = lens.to(torch.int64) * 2
        off, total = batch.layout(sizes.cpu(), 64)
        off = off.to(dev)
        raw = torch.empty(total, dtype=torch.uint8, device=dev)
        c.synth_signal(seed, 0, raw, off, lens)
        add_plateaus(raw.view(torch.int16), off // 2, lens)
        caps = torch.tensor([c.L.vbz_max_compressed_size(int(s), ctypes.byref(opts)) for s in sizes.cpu().tolist()], dtype=torch.int64)
        coff, ctotal = batch.layout(caps, 64)
        comp = torch.empty(ctotal, dtype=torch.uint8, device=dev)
        coff = coff.to(dev)
        csize = torch.zeros(n, dtype=torch.int32, device=dev)
        c.compress(raw, off, sizes.to(torch.int32).to(dev), comp, coff, caps.to(torch.int32).to(dev), csize, opts)
    torch.cuda.synchronize()
    del raw
    size32 = sizes.to(torch.int32).to(dev)
    back = torch.empty(total, dtype=torch.uint8, device=dev)
    off16 = off // 2
    Tl = lens.to(dev)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    ss = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    begin = torch.zeros(n, dtype=torch.int32, device=dev)
    kept = {}

    def stats(name):
        c.signal_norm(comp, coff, csize, off, size32, res, opts, NORMS[name][1], shift_scale=ss)

    def trim_call(name):
        c.signal_trim(comp, coff, csize, off, size32, res, opts, NORMS[name][1], trim=trim, out=begin, shift_scale=ss)

    def trim_chunks():
        trim_call("med_mad")
        kept["fused"] = c.decompress_chunks(comp, coff, csize, Tl, res, opts, L_, S_, norm=batch.MED_MAD, begin=begin)

    def unfused():
        c.decompress(comp, coff, csize, back, off, size32, res, opts)
        med, mad = TN.torch_med_mad(back.view(torch.int16), off16, Tl, int(Tl.max()))
        k = torch.tensor(1.4826, dtype=torch.float32).double().item()
        scale = torch.clamp(k * mad, min=batch.FLT_MIN).float()
        kept["torch_begin"] = torch_trim(back.view(torch.int16), off16, Tl, med.float(), scale, p)
        kept["unfused"] = c.decompress_chunks(comp, coff, csize, Tl, res, opts, L_, S_, norm=batch.MED_MAD, begin=kept["torch_begin"])

    fns = {"stats_med_mad": lambda: stats("med_mad"), "trim_med_mad": lambda: trim_call("med_mad"), "stats_quantile": lambda: stats("quantile"),
           "trim_quantile": lambda: trim_call("quantile"), "trim_chunks": trim_chunks}
    if unfused_leg:
        fns["unfused"] = unfused
    if only:
        fns = {k: fn for k, fn in fns.items() if k in only}
    ms = TN.timed(c, fns, reps)
    torch.cuda.synchronize()
    row = {"reads": n, "samples": int(lens.to(torch.int64).sum()), "trim": list(p), "ms": ms}
    for name in NORMS:
        if "trim_" + name in ms and "stats_" + name in ms:
            row["trim_pass_ms_" + name] = round(ms["trim_" + name] - ms["stats_" + name], 4)

    # every begin against tests/trim_ref.py
    checks = {}
    W, m, t0, M, f, mf, flags = p
    with torch.cuda.stream(c.stream):
        c.decompress(comp, coff, csize, back, off, size32, res, opts)
        back16 = back.view(torch.int16)
        ar = torch.arange(M, dtype=torch.int64, device=dev)[None, :]
        Th = lens.cpu().numpy().astype(np.int64)
        for name, (ref, nm) in NORMS.items():
            if only and "trim_" + name not in only and not (name == "med_mad" and "trim_chunks" in only):
                continue
            trim_call(name)
            torch.cuda.synchronize()
            got, ssh = begin.cpu().numpy().view(np.uint32), ss.cpu().numpy()
            ok, full, moved = True, 0, int(np.sum((got != t0) & (got != 0)))
            for a in range(0, n, BLOCK):
                b = min(n, a + BLOCK)
                idx = torch.clamp(off16[a:b][:, None] + ar, max=back16.numel() - 1)
                pre = back16[idx].cpu().numpy()
                for i in range(a, b):
                    x = pre[i - a, : min(M, Th[i])]
                    ok = ok and int(got[i]) == T.trim(x, T.threshold(ssh[i][0], ssh[i][1], f), W, m, t0, M, mf, flags, T=Th[i])
                    if full_every and i % full_every == 0:   # ... and from the read's values alone
                        lo = int(off16[i])
                        whole = back16[lo : lo + int(Th[i])].cpu().numpy()
                        ok = ok and int(got[i]) == T.begin(whole, ref, p)
                        full += 1
            checks[name] = ok
            row["begins_" + name] = {"other_than_min_trim": moved, "checked_from_sorted_values": full}
        if "unfused" in fns and "trim_chunks" in fns:
            trim_chunks()
            unfused()
            torch.cuda.synchronize()
            checks["torch_walk"] = torch.equal(kept["torch_begin"], begin)
            checks["unfused_chunks"] = all(torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a, b.view(torch.int16) if b.dtype == torch.float16 else b)
                                           for a, b in zip(kept["fused"], kept["unfused"]))
    row["checked"] = checks
    assert all(checks.values()), checks
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", action="append", default=[],
                    help="time only these calls (stats_med_mad, trim_med_mad, stats_quantile, trim_quantile, trim_chunks, unfused)")
    ap.add_argument("--full-every", type=int, default=256, help="check every n-th read's begin from its sorted values alone (0: none)")
    ap.add_argument("--no-huge", action="store_true", help="skip the 20 M-sample read")
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    out = {"headline": case(c, c.synth_lengths(5, 0, args.reads), args.reps, args.only, 5, True, args.full_every)}
    torch.cuda.empty_cache()
    if not args.no_huge:
        out["one_20M_read"] = case(c, torch.tensor([20_000_000], dtype=torch.int32, device=c.device), args.reps, args.only, 7, False, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
