#!/usr/bin/env python3
"""Cost of the calls over POD5 reads of several rows (include/vbz_gpu.h: vbz_gpu_pod5_reads) next to the row-wise calls over the same
rows, alternating in one process.

65 536 rows grouped into reads of 1 - 4 rows as pod5 cuts them: every row of a read but its last has 102 400 samples, the last one
90 000 - 110 000 (SURVEY.md 8d lengths), the signal synthesised on the device and compressed by the library.  Timed with HIP events on
the codec's stream, median of --reps calls behind untimed warm-up calls, the calls alternating; float16, L = 10 000, S = 9 504, PAD:
  chunks        the grouped chunk call with given constants against the row-wise chunk call (the same decode work)
  norm chunks   grouped normalised chunks, MED_MAD and QUANTILE, against the row-wise normalised chunks
  unfused       the exact route without these calls, on the first --unfused rows: int16 decode into pod5_read_layout, torch per-read
                median / MAD, torch gather into chunks -- against the grouped MED_MAD call on the same rows
  one read      200 rows of one read alone: the serial walk of a counting pass over its rows
Checked: every result, reads of one row against the row-wise outputs, and a sample of reads against tests/pod5_reads_ref.py.

    python tools/time_pod5_reads.py [--rows 65536] [--reps 20]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vbz_compression_amd import batch  # noqa: E402

L, S, ROW = 10_000, 9_504, 102_400
OPTS = batch.pod5_options()


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


def make_rows(c, n_rows, seed, rows_per_read=None):
    """(lens int32 [rows] on the device, first_row list) of reads of 1 - 4 rows (or rows_per_read), full rows but the last of each read"""
    rng = np.random.default_rng(seed)
    tail = c.synth_lengths(seed, 0, n_rows).cpu().numpy()
    lens, first, i = np.empty(n_rows, np.int32), [], 0
    while i < n_rows:
        k = min(rows_per_read or int(rng.integers(1, 5)), n_rows - i)
        first.append(i)
        lens[i : i + k - 1] = ROW
        lens[i + k - 1] = tail[i + k - 1]
        i += k
    return torch.from_numpy(lens).to(c.device), first


def compress_rows(c, lens, seed):
    dev = c.device
    n = int(lens.numel())
    sizes = lens.to(torch.int64).cpu() * 2
    off, total = batch.layout(sizes, 64)
    off = off.to(dev)
    size32 = sizes.to(torch.int32).to(dev)
    raw = torch.empty(total, dtype=torch.uint8, device=dev)
    c.synth_signal(seed, 0, raw, off, lens)
    caps = torch.tensor([batch.pod5_max_compressed_size(int(s) // 2) for s in sizes.tolist()], dtype=torch.int64)
    coff, ctotal = batch.layout(caps, 64)
    comp = torch.empty(ctotal, dtype=torch.uint8, device=dev)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    c.compress(raw, off, size32, comp, coff.to(dev), caps.to(torch.int32).to(dev), res, OPTS)
    torch.cuda.synchronize()
    assert int(res.min()) >= 0
    return raw, off, size32, comp, coff.to(dev), res


class Grouped:
    """the tables of one grouped chunk call, kept alive; run(norm) queues it"""

    def __init__(self, c, comp, coff, csize, lens, first, offset=None, scale=None):
        from vbz_compression_amd import _lib

        self.c, dev = c, c.device
        self.n, self.R = int(lens.numel()), len(first)
        self.comp, self.coff, self.csize = comp, coff, csize
        self.r, self.table, self.read_result = c._pod5_reads(self.n, first, None)
        self.dst_off, self.dst_cap = c._row_layout(lens)
        self.total = int(self.dst_off[-1])
        self.read_samples = torch.empty(self.R, dtype=torch.int32, device=dev)
        c._rc(c.L.vbz_gpu_pod5_read_samples_batch(c.ctx, self.n, lens.data_ptr(), _lib.ctypes.byref(self.r), self.read_samples.data_ptr()), "read_samples")
        self.ch = c._chunking(L, S, "pad", 1)
        self.chunk_first, _ = c.chunk_layout(self.read_samples, L, S, "pad", info=False)
        self.rows = int(self.chunk_first[-1])
        self.chunks = torch.empty((self.rows, L), dtype=torch.float16, device=dev)
        self.result = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.ss = torch.empty((self.R, 2), dtype=torch.float32, device=dev)
        self.offset, self.scale = offset, scale
        no_dst = torch.empty(0, dtype=torch.uint8, device=dev)
        self.b = c._batch(comp, coff, csize, no_dst, self.dst_off[: self.n], self.dst_cap, self.result)
        self.b.dst, self.b.dst_bytes = None, self.total

    def run(self, norm=None):
        import ctypes

        c = self.c
        f = c._signal_format(torch.float16, self.R, None if norm else self.scale, None if norm else self.offset, True)
        m = norm.c_struct() if norm else None
        c._rc(c.L.vbz_gpu_pod5_decompress_chunks_batch(c.ctx, ctypes.byref(self.b), ctypes.byref(OPTS), ctypes.byref(f), ctypes.byref(self.ch),
                                                       ctypes.byref(self.r), self.chunk_first.data_ptr(), self.chunks.data_ptr(), self.rows,
                                                       ctypes.byref(m) if m else None, self.ss.data_ptr() if m else None), "pod5 chunks")


def check_sample(c, g, raw, off, lens, first, norm_params, picks):
    """reads `picks` of the grouped call's last output (MED_MAD) against the numpy reference"""
    import norm_ref as R
    import pod5_reads_ref as PR

    bounds = first + [g.n]
    cf = g.chunk_first.cpu().numpy()
    host_len = lens.cpu().numpy()
    for k in picks:
        rows = []
        for i in range(bounds[k], bounds[k + 1]):
            o = int(off[i])
            rows.append(raw[o : o + 2 * int(host_len[i])].cpu().numpy().view(np.int16))
        x = np.concatenate(rows)
        shift, scale, so, sc = PR.shift_scale(x, norm_params)
        ss = g.ss[k].cpu().numpy()
        assert (ss[0].view(np.uint32), ss[1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), k
        _, want = PR.chunk_rows(x, L, S, "pad", 0, so, sc, 0.0, "f16")
        got = g.chunks[cf[k] : cf[k + 1]].view(torch.int16).cpu().numpy().view(np.uint16)
        assert (got == want).all(), k


def headline(c, n_rows, reps, seed):
    import norm_ref as R

    dev = c.device
    lens, first = make_rows(c, n_rows, seed)
    raw, off, size32, comp, coff, csize = compress_rows(c, lens, seed)
    R_ = len(first)
    gen = torch.Generator().manual_seed(seed)
    o_row = (torch.rand(n_rows, generator=gen) * 400 - 200).to(dev)
    s_row = (torch.rand(n_rows, generator=gen) * 0.3 + 0.05).to(dev)
    first_t = torch.tensor(first, device=dev)
    g = Grouped(c, comp, coff, csize, lens, first, o_row[first_t].contiguous(), s_row[first_t].contiguous())
    # the row-wise calls over the same rows
    ch = c._chunking(L, S, "pad", 1)
    row_first, _ = c.chunk_layout(lens, L, S, "pad", info=False)
    row_chunks = torch.empty((int(row_first[-1]), L), dtype=torch.float16, device=dev)
    row_res = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    row_ss = torch.empty((n_rows, 2), dtype=torch.float32, device=dev)

    def rowwise(norm=None):
        c._decode_chunks(comp, coff, csize, g.dst_off[:n_rows], g.dst_cap, g.total, row_res, OPTS, False, ch, row_first, row_chunks, torch.float16,
                         None if norm else s_row, None if norm else o_row, True, norm, row_ss if norm else None)

    ms = timed(c, {"chunks_rows": rowwise, "chunks_reads": g.run}, reps)
    torch.cuda.synchronize()
    assert torch.equal(g.result, g.dst_cap) and torch.equal(row_res, g.dst_cap)
    assert torch.equal(g.read_result, (g.read_samples.to(torch.int64) * 2).to(torch.int32))
    one = [k for k in range(R_ - 1) if first[k + 1] - first[k] == 1][:64]   # reads of one row: the row-wise call's chunks
    gcf, rcf = g.chunk_first.cpu().numpy(), row_first.cpu().numpy()
    for k in one:
        i = first[k]
        assert torch.equal(g.chunks[gcf[k] : gcf[k + 1]], row_chunks[rcf[i] : rcf[i + 1]]), k
    ms.update(timed(c, {"norm_rows_med_mad": lambda: rowwise(batch.MED_MAD), "norm_reads_quantile": lambda: g.run(batch.DORADO_QUANTILE),
                        "norm_rows_quantile": lambda: rowwise(batch.DORADO_QUANTILE), "norm_reads_med_mad": lambda: g.run(batch.MED_MAD)}, reps))
    torch.cuda.synchronize()
    assert torch.equal(g.result, g.dst_cap)
    check_sample(c, g, raw, off, lens, first, R.BONITO, [0, 1, 2, R_ // 2, R_ - 1])
    row = {"rows": n_rows, "reads": R_, "samples": int(lens.to(torch.int64).sum()), "chunk_rows": g.rows, "ms": ms}
    row["chunks_reads_over_rows"] = round(ms["chunks_reads"] / ms["chunks_rows"], 3)
    row["norm_med_mad_reads_over_rows"] = round(ms["norm_reads_med_mad"] / ms["norm_rows_med_mad"], 3)
    row["norm_quantile_reads_over_rows"] = round(ms["norm_reads_quantile"] / ms["norm_rows_quantile"], 3)
    row["norm_med_mad_over_chunks_reads"] = round(ms["norm_reads_med_mad"] / ms["chunks_reads"], 3)
    return row


def unfused(c, n_rows, reps, seed):
    """int16 decode into pod5_read_layout, torch median / MAD per read, torch gather -- against the grouped MED_MAD call"""
    dev = c.device
    lens, first = make_rows(c, n_rows, seed)
    raw, off, size32, comp, coff, csize = compress_rows(c, lens, seed)
    g = Grouped(c, comp, coff, csize, lens, first)
    lay = batch.pod5_read_layout(lens.cpu(), first, elem=2, align=16, device=dev)
    dst = torch.empty(lay.total + 64, dtype=torch.uint8, device=dev)
    res = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    cf = g.chunk_first.cpu().numpy()
    info = torch.empty((g.rows, 2), dtype=torch.int32, device=dev)
    c._chunk_layout_call(g.read_samples, g.ch, g.chunk_first, info, g.rows)
    read_of, start = info[:, 0].long(), info[:, 1].long()
    out = torch.empty((g.rows, L), dtype=torch.float16, device=dev)
    read_off, read_len = (lay.read_off // 2), lay.read_len

    def route():
        c.decompress(comp, coff, csize, dst, lay.dst_off, lay.dst_cap, res, OPTS)
        sig = dst[: lay.total].view(torch.int16)
        consts = torch.empty((g.R, 2), dtype=torch.float32, device=dev)
        for k in range(g.R):   # per-read order statistics: a sort each
            x = sig[int(read_off[k]) : int(read_off[k]) + int(read_len[k])].float()
            med = x.median()
            consts[k, 0] = med
            consts[k, 1] = 1.4826 * (x - med).abs().median()
        idx = start[:, None] + torch.arange(L, device=dev)[None, :]
        ok = idx < read_len[read_of][:, None]
        flat = (read_off[read_of][:, None] + idx).clamp_(max=sig.numel() - 1)
        y = (sig[flat].float() - consts[read_of, 0][:, None]) / consts[read_of, 1][:, None]
        out.copy_(torch.where(ok, y, torch.zeros_like(y)).half())

    read_off, read_len = read_off.to(dev), read_len.to(dev)
    ms = timed(c, {"unfused": route, "reads_med_mad": lambda: g.run(batch.MED_MAD)}, max(3, reps // 4), warm=1)
    torch.cuda.synchronize()
    assert torch.equal(res, g.dst_cap) and torch.equal(g.result, g.dst_cap)
    close = (out.float() - g.chunks.float()).abs().max().item()
    assert close < 0.05, close   # (torch's median takes the lower middle value and divides: close, not equal)
    return {"rows": n_rows, "reads": g.R, "ms": ms, "unfused_over_reads": round(ms["unfused"] / ms["reads_med_mad"], 1)}


def one_read(c, n_rows, reps, seed):
    import norm_ref as R

    lens, first = make_rows(c, n_rows, seed, rows_per_read=n_rows)
    raw, off, size32, comp, coff, csize = compress_rows(c, lens, seed)
    g = Grouped(c, comp, coff, csize, lens, first)
    ms = timed(c, {"chunks_reads": g.run, "norm_reads_quantile": lambda: g.run(batch.DORADO_QUANTILE), "norm_reads_med_mad": lambda: g.run(batch.MED_MAD)},
               reps)
    torch.cuda.synchronize()
    assert torch.equal(g.result, g.dst_cap)
    check_sample(c, g, raw, off, lens, first, R.BONITO, [0])
    return {"rows": n_rows, "reads": 1, "samples": int(lens.to(torch.int64).sum()), "ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--unfused", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    c = batch.GpuCodec(0)
    out = {"headline": headline(c, args.rows, args.reps, 5)}
    torch.cuda.empty_cache()
    out["unfused"] = unfused(c, args.unfused, args.reps, 6)
    torch.cuda.empty_cache()
    out["one_read_200_rows"] = one_read(c, 200, args.reps, 7)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
