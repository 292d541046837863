"""The verdicts of the svb decoder on the MI355X, through EVERY call that runs it (svb_kernels.hip: svb_read_open and the large-read
path's result of a read).  A catalogue of svb-level defects -- a stream a byte short or long, a source size below the control bytes, a
capacity that is off by a sample, by a byte, or zero -- is built from level-0 frames (the svb stream IS the frame, so a changed size
reaches the svb stage as it stands), at sizes around a lane's values, a wavefront's, a tile's and the paired-tile loop's; two more rows
come from a level-1 batch: a frame cut in half (the previous stage's verdict) and a source offset outside the declared arena (the
gate's).  (a) the int16 decode gives the CPU oracle's verdict and bytes for every row; (b) every other consumer of the decoder reports
(a)'s verdict for every read (a) failed; (c) for every other read it reports its own byte count, and its output is, byte for byte, that
of the same call over the good reads alone.  On the default context and on both forced paths, and with reads of three segments on the
forced large-read path; tests/test_gpu_large_reads.py runs this file again with scan launches between the segmented passes."""
import dataclasses

import numpy as np
import pytest
import torch

import oracle_lib as O
from typed_support import Frames, arena, codec, i32, sine_signal, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

E_STREAM, E_DEST, E_INPUT = 0xFFFFFFFB, 0xFFFFFFFC, 0xFFFFFFFE
SIZES = (9, 513, 2049, 4101)
BIG = 40_000   # three segments of the large-read path
# defect -> (source size, capacity) of a stream of S bytes that holds T samples in K control bytes; "appended": one more byte in the slot
DEFECTS = {
    "intact": lambda S, T, K: (S, 2 * T),
    "last byte missing": lambda S, T, K: (S - 1, 2 * T),
    "one byte appended": lambda S, T, K: (S + 1, 2 * T),
    "src_size = K - 1": lambda S, T, K: (K - 1, 2 * T),
    "src_size = 0": lambda S, T, K: (0, 2 * T),
    "dst_cap + 2": lambda S, T, K: (S, 2 * T + 2),
    "dst_cap - 2": lambda S, T, K: (S, 2 * T - 2),
    "dst_cap = 0": lambda S, T, K: (S, 0),
    "dst_cap + 1": lambda S, T, K: (S, 2 * T + 1),
}
# the oracle's verdicts, as it gave them for this catalogue at all four sizes (None: no error)
ORACLE = {"intact": None, "last byte missing": E_STREAM, "one byte appended": E_STREAM, "src_size = K - 1": E_INPUT, "src_size = 0": E_INPUT,
          "dst_cap + 2": E_STREAM, "dst_cap - 2": E_STREAM, "dst_cap = 0": None, "dst_cap + 1": E_DEST}
# (consumer, defect) pairs the consumer's Python signature cannot express: a call that takes `samples` cannot give an odd capacity
LEFT_OUT = {("decompress_chunks", "dst_cap + 1"), ("decompress_windows", "dst_cap + 1")}
MED_MAD = batch.MED_MAD
L0, L1 = (True, 2, 0, 1), (True, 2, 1, 1)


@dataclasses.dataclass
class Row:
    """one read of a batch: the bytes in its source slot, the sizes its descriptor gives, and what the oracle says of them"""
    buf: np.ndarray
    size: int
    cap: int
    defect: str
    want: object              # the oracle's bytes, or its verdict
    off: int = None           # another source offset than the slot's
    T: int = 0                # the samples of the read the row was made from

    @property
    def failed(self):
        return isinstance(self.want, int)


def level0_rows(T, rng, defects=DEFECTS):
    x = sine_signal(rng, T)
    stream = O.compress(x, O.options(*L0))
    K = (T + 3) // 4
    rows = []
    for name in defects:
        size, cap = DEFECTS[name](len(stream), T, K)
        buf = np.concatenate([stream, np.zeros(1, np.uint8)])
        rows.append(Row(buf, size, cap, name, O.decompress(buf[:size], cap, O.options(*L0)), T=T))
    return rows


_cache = {}


def catalogue():
    if "cat" not in _cache:
        rng = np.random.default_rng(23)
        rows = [r for T in SIZES for r in level0_rows(T, rng)]
        for r in rows:   # the oracle on this machine against the table above
            assert (r.want if r.failed else None) == ORACLE[r.defect], (r.defect, r.size, r.cap, r.want if r.failed else "decoded")
        _cache["cat"] = rows
    return _cache["cat"]


def big_rows(defect):
    """an intact read of three segments and one with the defect"""
    if defect not in _cache:
        _cache[defect] = level0_rows(BIG, np.random.default_rng(29), ("intact", defect))
    return _cache[defect]


def level1_rows():
    """the library's own level-1 frames: two intact, one cut in half, one whose source offset lies outside the declared arena"""
    if "l1" not in _cache:
        c = codec()
        rng = np.random.default_rng(31)
        fr = Frames(c, [sine_signal(rng, T) for T in (5000, 3000, 2500, 900)], c.options(*L1))
        host, offs, sizes = fr.src.cpu().numpy(), fr.off.cpu().tolist(), u32(fr.size).tolist()
        frames = [host[o : o + int(s)].copy() for o, s in zip(offs, sizes)]
        rows = []
        for i, (f, x) in enumerate(zip(frames, fr.reads)):
            size = len(f) // 2 if i == 1 else len(f)
            want = O.decompress(f[:size], x.nbytes, O.options(*L1))
            rows.append(Row(f, size, x.nbytes, ("intact", "frame cut in half", "src_off outside the arena", "intact")[i], want))
        assert rows[1].failed and not rows[0].failed and not rows[3].failed
        rows[2].off, rows[2].want = 1 << 40, E_INPUT   # (the descriptor check's verdict: include/vbz_gpu.h)
        _cache["l1"] = rows
    return _cache["l1"]


class Batch:
    """rows on the device: the source arena and the int16 layout that describes the reads (slots with room for a capacity too large)"""

    def __init__(self, c, rows, opts):
        self.c, self.rows, self.n, self.opts = c, rows, len(rows), c.options(*opts)
        dev = c.device
        self.src, off, _ = arena(c, [r.buf for r in rows], 64)
        off = off.cpu()
        for i, r in enumerate(rows):
            if r.off is not None:
                off[i] = r.off
        self.off, self.size = off.to(dev), i32([r.size for r in rows]).to(dev)
        self.caps = [r.cap for r in rows]
        doff, self.dst_bytes = batch.layout([cp + 32 for cp in self.caps], 64)
        self.doff_h, self.doff, self.dcap = doff.tolist(), doff.to(dev), i32(self.caps).to(dev)
        self.samples = i32([cp // 2 for cp in self.caps]).to(dev)
        self.result = torch.full((self.n,), -8, dtype=torch.int32, device=dev)
        # two windows / events per read, at samples 0 and 4
        self.first = torch.arange(0, 2 * self.n + 1, 2, dtype=torch.int64, device=dev)
        self.start = torch.tensor([0, 4] * self.n, dtype=torch.int32, device=dev)

    def args(self):
        return self.src, self.off, self.size

    def done(self, per_read):
        """(result[], every read's output bytes) of a call that has just been made"""
        torch.cuda.synchronize()
        return u32(self.result).tolist(), [bytes(p) for p in per_read()]


def _bytes(t):
    return t.reshape(-1).contiguous().view(torch.uint8).cpu().numpy().tobytes()


def _slots(B, dst):
    """the reads' slots of an arena of 2-byte samples laid out as the int16 layout"""
    def per_read():
        h = dst.view(torch.uint8).cpu().numpy()
        return [h[o : o + cp // 2 * 2].tobytes() for o, cp in zip(B.doff_h, B.caps)]
    return per_read


def _rows_of(first, *tensors):
    """read i's rows first[i] ... first[i + 1] - 1 of every tensor"""
    def per_read():
        f = first.cpu().tolist()
        return [b"".join(_bytes(t[f[i] : f[i + 1]]) for t in tensors) for i in range(len(f) - 1)]
    return per_read


def _each(*tensors):
    """entry i of every tensor"""
    return lambda: [b"".join(_bytes(t[i]) for t in tensors) for i in range(int(tensors[0].shape[0]))]


# ---- the consumers: name -> (bytes per sample in result[], the call) ---------------------------------------------------------------
def int16_decode(B):
    dst = torch.zeros(B.dst_bytes + 64, dtype=torch.uint8, device=B.c.device)
    B.c.decompress(*B.args(), dst, B.doff, B.dcap, B.result, B.opts)
    return B.done(_slots(B, dst))


def decompress_signal(B, norm=None):
    dst = torch.zeros((B.dst_bytes + 64) // 2, dtype=torch.float16, device=B.c.device)   # (float16: the typed layout is the int16 one)
    ss = torch.zeros((B.n, 2), dtype=torch.float32, device=B.c.device)
    B.c.decompress_signal(*B.args(), dst, B.doff, B.dcap, B.result, B.opts, norm=norm, norm_out=ss if norm else None)
    return B.done(lambda: [a + b for a, b in zip(_slots(B, dst)(), _each(ss)())])


def decompress_signal_norm(B):
    return decompress_signal(B, MED_MAD)


def decompress_chunks(B):
    chunks, first, _ = B.c.decompress_chunks(*B.args(), B.samples, B.result, B.opts, 64, 48)
    return B.done(_rows_of(first[: B.n + 1], chunks))


def decompress_windows(B):
    out = B.c.decompress_windows(*B.args(), B.samples, B.result, B.opts, B.first, B.start, 16)
    return B.done(_rows_of(B.first, out))


def signal_events(B):
    rec = torch.zeros((2 * B.n, 4), dtype=torch.int32, device=B.c.device)
    B.c.signal_events(*B.args(), B.doff, B.dcap, B.result, B.opts, B.first, B.start, arena=rec)
    return B.done(_rows_of(B.first, rec))


def signal_norm(B):
    ss = torch.zeros((B.n, 2), dtype=torch.float32, device=B.c.device)
    B.c.signal_norm(*B.args(), B.doff, B.dcap, B.result, B.opts, MED_MAD, shift_scale=ss)
    return B.done(_each(ss))


def signal_trim(B):
    begin, ss = B.c.signal_trim(*B.args(), B.doff, B.dcap, B.result, B.opts, MED_MAD,
                                shift_scale=torch.zeros((B.n, 2), dtype=torch.float32, device=B.c.device))
    return B.done(_each(begin, ss))


def signal_segment(B):
    first, start = B.c.signal_segment(*B.args(), B.doff, B.dcap, B.result, B.opts)
    return B.done(_rows_of(first, start))


SPANS = batch.Spans("above", 2, 2, 0, 1.0)


def signal_spans_level(B):
    """the caller's constants: no counting pass runs, the span pass writes the verdicts itself (thr = 330 + 40: the sine's crests)"""
    level = torch.tensor([[330.0, 40.0]] * B.n, dtype=torch.float32, device=B.c.device).reshape(B.n, 2)
    first, edge = B.c.signal_spans(*B.args(), B.doff, B.dcap, B.result, B.opts, SPANS, level=level)
    return B.done(_rows_of(first, edge))


def signal_spans_norm(B):
    """a normalisation: the span pass runs behind the counting passes, which have left the verdicts"""
    first, edge = B.c.signal_spans(*B.args(), B.doff, B.dcap, B.result, B.opts, SPANS, norm=MED_MAD)
    return B.done(_rows_of(first, edge))


CONSUMERS = {
    "decompress_signal": (2, decompress_signal), "decompress_chunks": (2, decompress_chunks), "decompress_windows": (2, decompress_windows),
    "signal_events": (2, signal_events), "signal_norm": (2, signal_norm), "signal_trim": (2, signal_trim), "signal_segment": (2, signal_segment),
    "decompress_signal with norm=": (2, decompress_signal_norm),
    "signal_spans with level=": (2, signal_spans_level), "signal_spans with norm=": (2, signal_spans_norm),
}


def check(c, rows, opts, min_errors, consumer_errors=5):
    """(a), (b) and (c) over `rows`; min_errors: the error verdicts (a) must find; consumer_errors: the error rows every consumer must keep"""
    # (a) the int16 decode against the oracle
    res, out = int16_decode(Batch(c, rows, opts))
    for i, r in enumerate(rows):
        print("int16 decode: %-26s size %6d cap %6d -> %s (oracle: %s)" % (r.defect, r.size, r.cap, hex(res[i]), hex(r.want) if r.failed else len(r.want)))
    for i, r in enumerate(rows):
        if r.failed:
            assert res[i] == r.want, ("int16 decode", i, r.defect, r.size, r.cap, hex(res[i]), hex(r.want))
        else:
            assert res[i] == len(r.want) and out[i][: res[i]] == r.want.tobytes(), ("int16 decode", i, r.defect, r.size, r.cap, hex(res[i]))
    failed = [_lib.is_error(v) for v in res]
    assert sum(failed) >= min_errors, (sum(failed), min_errors)
    for T in SIZES:   # seven per size: what the oracle alone gives
        n = sum(f for f, r in zip(failed, rows) if r.defect in DEFECTS and r.T == T)
        assert n >= 7 or not any(r.T == T for r in rows), (T, n)
    for name, (E, call) in CONSUMERS.items():
        keep = [i for i, r in enumerate(rows) if (name, r.defect) not in LEFT_OUT]
        sub = [rows[i] for i in keep]
        assert sum(failed[i] for i in keep) >= consumer_errors, (name, "error rows", sum(failed[i] for i in keep))
        got, out = call(Batch(c, sub, opts))
        good = [j for j, i in enumerate(keep) if not failed[i]]
        alone, out_alone = call(Batch(c, [sub[j] for j in good], opts))
        for j, i in enumerate(keep):
            r = rows[i]
            if failed[i]:   # (b) the int16 decode's verdict
                assert got[j] == res[i], (name, r.defect, r.size, r.cap, hex(got[j]), hex(res[i]))
        for g, j in enumerate(good):   # (c) its own byte count, and the bytes of the call over the good reads alone
            r = sub[j]
            assert got[j] == alone[g] == r.cap // 2 * E, (name, r.defect, r.size, r.cap, hex(got[j]), hex(alone[g]))
            assert out[j] == out_alone[g], (name, r.defect, r.size, r.cap, "output differs from the call over the good reads alone")


CODECS = {"default": {}, "large_read_path": {"VBZ_HIP_SEGMENTED": 1}, "one_wavefront_path": {"VBZ_HIP_SEGMENTED": 0}}


@pytest.mark.parametrize("path", list(CODECS))
def test_catalogue(path):
    """every defect at every size in one batch: seven error verdicts per size, as the oracle alone gives them"""
    check(codec(**CODECS[path]), catalogue(), L0, 7 * len(SIZES))


@pytest.mark.parametrize("path", list(CODECS))
def test_inherited_and_gate_verdicts(path):
    """the previous stage's verdict (a frame cut in half) and the descriptor check's (a source offset outside the arena) come before
    anything the svb stage finds, and reach result[] of every consumer"""
    check(codec(**CODECS[path]), level1_rows(), L1, 2, consumer_errors=2)   # (the batch's two error rows, which no consumer leaves out)


@pytest.mark.parametrize("defect", ["last byte missing", "dst_cap + 2"])
def test_read_of_three_segments(defect):
    """the catalogue with two reads of 40 000 samples, one of them with the defect, on the forced large-read path: its verdict is the
    read's, decided once from what its three segments announce"""
    check(codec(VBZ_HIP_SEGMENTED=1), catalogue() + big_rows(defect), L0, 7 * len(SIZES) + 1)
