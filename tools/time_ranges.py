#!/usr/bin/env python3
"""Cost of per-read sample ranges in the chunk and normalising decodes (vbz_gpu_decompress_chunks_range_batch) against the un-ranged calls
and the unfused route, alternating in one process.

Headline: 65 536 synthetic reads (~100 k int16 samples each) compressed once; chunks of L = 10 000 samples every S = 9 504,
PAD, float16; then, each behind untimed warm-up calls and timed with HIP events on the codec's stream (median of --reps calls):
  chunks            (a) vbz_gpu_decompress_chunks_batch, the whole read, per-read constants given
  range_whole       (b) the range call with begin = 0, end = T: the ranged kernels on the whole read
  range_2000        (c) begin = 2 000 (a multiple of 8: whole-line stores), end to the end
  range_2003        (d) begin = 2 003 (element by element)
  norm              (e) vbz_gpu_decompress_chunks_norm_batch, MED_MAD, the whole read
  range_norm_range      begin = 2 000, end = T - 2 000, MED_MAD of the range (Bonito: trim, then normalise)
  range_norm_read       the same range, MED_MAD of the whole read (Dorado: normalise, then trim)
  unfused           (f) the route without the feature: the int16 decode, a torch median / MAD of the slices (tools/time_norm.py), the
                    float16 signal decode with the constants they give, a torch gather of the slices into chunks (tools/time_chunks.py)
Then one 20 M-sample read (the large-read path) with the range in its middle, the same calls but (f).  Every output is checked bit for
bit: (b) against (a); (c), (d) and the normalised legs against a gather of the float16 signal decode with the same constants; (f)
against range_norm_range.

    python tools/time_ranges.py [--reads 65536] [--reps 20] [--only range_2003]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import time_chunks as TC  # noqa: E402
import time_norm as TN  # noqa: E402
from vbz_compression_amd import _lib, batch  # noqa: E402

L_, S_ = 10000, 9504
PAD = 0.0


def case(c, lens, reps, only, seed, trim, odd, unfused_leg):
    """trim: samples cut at either end; odd: the begin of the element-wise leg"""
    dev = c.device
    n = int(lens.numel())
    opts = c.options(True, 2, 1, 1)
    with torch.cuda.stream(c.stream):
        sizes = lens.to(torch.int64) * 2
        off, total = batch.layout(sizes.cpu() + 2, 64)   # (one element behind every slot: the gather's pad)
        off = off.to(dev)
        raw = torch.empty(total, dtype=torch.uint8, device=dev)
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
    back = torch.empty(total, dtype=torch.uint8, device=dev)
    sig = torch.empty(total // 2, dtype=torch.float16, device=dev)
    sig_off = off // 2
    g = torch.Generator().manual_seed(seed)
    o_t = (torch.rand(n, generator=g) * 400 - 200).to(dev)
    s_t = (torch.rand(n, generator=g) * 0.3 + 0.05).to(dev)
    u_off = torch.empty(n, dtype=torch.float32, device=dev)
    u_scale = torch.empty(n, dtype=torch.float32, device=dev)
    ch = c._chunking(L_, S_, "pad", 1, PAD)
    zero = torch.zeros(n, dtype=torch.int32, device=dev)
    T = lens.to(dev)

    # the legs' ranges: (begin, end) tables (None: a NULL table), and the layout of each
    ranges = {"whole": (zero, T), "b_even": (zero + trim, None), "b_odd": (zero + odd, None), "both": (zero + trim, T - trim)}
    lay = {}
    for k, (bg, en) in [("read", (None, None))] + list(ranges.items()):
        laid = T if k == "read" else c.range_samples(T, begin=bg, end=en)
        first, info = c.chunk_layout(laid, L_, S_, mode="pad", info=True)
        lay[k] = (laid, first, info, int(first[-1]))
    max_rows = max(v[3] for v in lay.values())
    out = torch.empty((max_rows, L_), dtype=torch.float16, device=dev)
    ref = torch.empty((max_rows, L_), dtype=torch.float16, device=dev)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    ss = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    mm = batch.MED_MAD.c_struct()

    def fmt(o=None, s=None):
        f = _lib.GpuSignalFormat()
        f.out_type, f.is_signed = _lib.VBZ_GPU_SIGNAL_F16, 1
        f.offset, f.scale = (o.data_ptr() if o is not None else None), (s.data_ptr() if s is not None else None)
        return f

    f_given, f_none, f_unf = fmt(o_t, s_t), fmt(), fmt(u_off, u_scale)

    def batch_of():
        b = c._batch(comp, coff, csize, back, off, size32, res)
        b.dst, b.dst_bytes = None, total
        return b

    def call(key, f, norm=False, stats=0, dst=None):
        """key: "read" = the un-ranged entry points, else the range call with ranges[key]"""
        dst = out if dst is None else dst
        laid, first, info, rows = lay[key]
        b = batch_of()
        m = ctypes.byref(mm) if norm else None
        sp = ss.data_ptr() if norm else None
        if key == "read" and not norm:
            rc = c.L.vbz_gpu_decompress_chunks_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 0, ctypes.byref(f), ctypes.byref(ch), first.data_ptr(),
                                                     dst.data_ptr(), rows)
        elif key == "read":
            rc = c.L.vbz_gpu_decompress_chunks_norm_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 0, ctypes.byref(f), ctypes.byref(ch),
                                                          first.data_ptr(), dst.data_ptr(), rows, m, sp)
        else:
            gr = _lib.GpuSampleRanges()
            bg, en = ranges[key]
            gr.begin, gr.end, gr.stats = (bg.data_ptr() if bg is not None else None), (en.data_ptr() if en is not None else None), stats
            rc = c.L.vbz_gpu_decompress_chunks_range_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 0, ctypes.byref(f), ctypes.byref(ch),
                                                           first.data_ptr(), dst.data_ptr(), rows, m, sp, ctypes.byref(gr))
        assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)

    plans = {}

    def gather(key, f, dst):
        """the float16 signal decode with f's constants, then the range's chunk positions gathered from it"""
        laid, first, info, rows = lay[key]
        bg = ranges[key][0].to(torch.int64)
        plan = plans.get(key)
        if plan is None:   # (8 bytes per chunk position: only the timed leg's index is kept)
            plan = TC.gather_plan(c, info, laid, sig_off + bg, first, L_)
            if key == "both":
                plans[key] = plan
        sres = torch.zeros(n, dtype=torch.int32, device=dev)
        b = c._batch(comp, coff, csize, sig.view(torch.uint8), off, size32, sres)
        rc = c.L.vbz_gpu_decompress_signal_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 0, ctypes.byref(f))
        assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)
        sig[sig_off + bg + laid.to(torch.int64)] = PAD   # (the element behind the slice: outside the range, or the slot's spare one)
        flat = dst.view(-1)
        for lo, hi, r0, r1, idx in plan:
            torch.index_select(sig[lo:hi], 0, idx, out=flat[r0 * L_ : r1 * L_])

    def unfused():
        c.decompress(comp, coff, csize, back, off, size32, res, opts)
        bg = ranges["both"][0].to(torch.int64)
        laid = lay["both"][0]
        med, mad = TN.torch_med_mad(back.view(torch.int16), sig_off + bg, laid, int(laid.max()))
        k = torch.tensor(1.4826, dtype=torch.float32).double().item()
        scale = torch.clamp(k * mad, min=batch.FLT_MIN).float()
        u_off.copy_(-med.float())
        u_scale.copy_((1.0 / scale.double()).float())
        gather("both", f_unf, ref)

    fns = {"chunks": lambda: call("read", f_given), "range_whole": lambda: call("whole", f_given), "range_2000": lambda: call("b_even", f_given),
           "range_2003": lambda: call("b_odd", f_given), "norm": lambda: call("read", f_none, True),
           "range_norm_range": lambda: call("both", f_none, True, 0), "range_norm_read": lambda: call("both", f_none, True, 1)}
    if unfused_leg:
        fns["unfused"] = unfused
    if only:
        fns = {k: fn for k, fn in fns.items() if k in only}
    ms = TC.timed(c, fns, reps)
    torch.cuda.synchronize()
    row = {"reads": n, "samples": int(lens.to(torch.int64).sum()), "chunk_len": L_, "step": S_, "trim": trim, "odd_begin": odd, "ms": ms}
    if "chunks" in ms:
        for k in ms:
            if k != "chunks":
                row[k + "_over_chunks"] = round(ms[k] / ms["chunks"], 3)
    want_res = T.to(torch.int64) * 2

    def same(rows):
        return torch.equal(out[:rows].view(torch.int16), ref[:rows].view(torch.int16))

    with torch.cuda.stream(c.stream):   # (the checks' torch work in the codec's stream order)
        checks = {}
        if "range_whole" in fns:   # (b) == (a)
            call("read", f_given, dst=ref)
            call("whole", f_given)
            torch.cuda.synchronize()
            checks["range_whole"] = same(lay["read"][3]) and torch.equal(res.to(torch.int64), want_res)
        for name, key in (("range_2000", "b_even"), ("range_2003", "b_odd")):   # == a gather of the signal decode
            if name in fns:
                out.fill_(7.0)
                call(key, f_given)
                gather(key, f_given, ref)
                torch.cuda.synchronize()
                checks[name] = same(lay[key][3]) and torch.equal(res.to(torch.int64), want_res)
        for name, stats in (("range_norm_range", 0), ("range_norm_read", 1)):   # == a gather with the constants the call reports
            if name in fns:
                out.fill_(7.0)
                call("both", f_none, True, stats)
                u_off.copy_(-ss[:, 0])
                u_scale.copy_((1.0 / ss[:, 1].double()).float())
                keep = ss.clone()
                gather("both", f_unf, ref)
                torch.cuda.synchronize()
                checks[name] = same(lay["both"][3]) and torch.equal(res.to(torch.int64), want_res)
                if stats == 1 and "norm" in fns:   # the whole read's constants are the un-ranged normalising call's
                    call("read", f_none, True)
                    torch.cuda.synchronize()
                    checks["range_norm_read_constants"] = torch.equal(ss, keep)
        if "unfused" in fns and "range_norm_range" in fns:   # (f): the torch route's constants and gather give the same chunks
            call("both", f_none, True, 0)
            unfused()
            torch.cuda.synchronize()
            checks["unfused"] = same(lay["both"][3])
    row["checked"] = checks
    assert all(checks.values()), checks
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", action="append", default=[],
                    help="time only these calls (chunks, range_whole, range_2000, range_2003, norm, range_norm_range, range_norm_read, unfused)")
    ap.add_argument("--no-huge", action="store_true", help="skip the 20 M-sample read")
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    out = {"headline": case(c, c.synth_lengths(5, 0, args.reads), args.reps, args.only, 5, 2000, 2003, True)}
    torch.cuda.empty_cache()
    if not args.no_huge:
        out["one_20M_read"] = case(c, torch.tensor([20_000_000], dtype=torch.int32, device=c.device), args.reps, args.only, 7, 5_000_000, 5_000_003, False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
