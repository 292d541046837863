"""The raw path calls for the tests on the MI355X (test_gpu_match_path, test_gpu_match_path_refusals): what match_span_support is to the
span calls.  vbz_gpu_match_path_batch over one pair table into canary-filled hit and row arenas with a guard entry behind each, and
vbz_gpu_match_best_batch over a span arena likewise.  A plain module: every assert carries its operands."""
import ctypes

import numpy as np
import torch

import match_path_ref as P
from match_support import HIT_CANARY, match_struct
from typed_support import i32
from vbz_compression_amd import _lib

EMPTY = list(P.EMPTY)


class PathArenas:
    """canary-filled hits and rows of n pairs, a guard entry (a guard row) behind each"""

    def __init__(self, c, n, stride):
        self.n = n
        self.hit = torch.full((n + 1, 4), HIT_CANARY, dtype=torch.int32, device=c.device)
        self.rows = torch.full((n + 1, stride, 2), HIT_CANARY, dtype=torch.int32, device=c.device)

    def untouched(self):
        return (self.hit.cpu().numpy().view(np.uint32) == HIT_CANARY).all() and (self.rows.cpu().numpy().view(np.uint32) == HIT_CANARY).all()

    def read(self):
        """(hit [n, 4], rows [n, stride, 2]) as uint32; the guards keep their canary"""
        hit, rows = self.hit.cpu().numpy().view(np.uint32), self.rows.cpu().numpy().view(np.uint32)
        assert (hit[self.n] == HIT_CANARY).all(), "the hit behind the last pair was written"
        assert (rows[self.n] == HIT_CANARY).all(), "the rows behind the last pair were written"
        return hit[: self.n], rows[: self.n]


def path_struct(max_width, flags=0, reserved=0):
    return _lib.GpuMatchPath(max_width, flags, reserved)


def stage_path(c, query, valid, quant, ref, ref_len, pairs, max_width):
    """vbz_gpu_match_path_batch -> (hit uint32 [pairs, 4], rows uint32 [pairs, stride, 2]).  query float32 [reads, N], valid any
    integers or None, pairs any integers [pairs, 4]; the query keeps its bits"""
    n, N = query.shape
    m, keep = match_struct(c, N, quant, ref, ref_len)
    q = torch.from_numpy(query).to(c.device)
    v = i32(valid).to(c.device) if valid is not None else None
    pr = i32(np.asarray(pairs, np.uint64).reshape(-1)).reshape(-1, 4).to(c.device)
    a = PathArenas(c, len(pairs), ref.shape[1])
    path = path_struct(max_width)
    torch.cuda.synchronize()
    rc = c.L.vbz_gpu_match_path_batch(c.ctx, len(pairs), n, q.data_ptr(), v.data_ptr() if v is not None else None, ctypes.byref(m), pr.data_ptr(),
                                      ctypes.byref(path), a.hit.data_ptr(), a.rows.data_ptr())
    c.synchronize()
    assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)
    assert (q.cpu().numpy().view(np.uint32) == query.view(np.uint32)).all(), "the path call wrote its query"
    return a.read()


def assert_paths(got, want, pairs, what):
    """hits and rows bit for bit"""
    (ghit, grows), (whit, wrows) = got, want
    bad = np.argwhere((ghit != whit).any(axis=-1))[:, 0]
    assert bad.size == 0, (what, "hit of pairs", [(int(p), list(pairs[p]), ghit[p].tolist(), whit[p].tolist()) for p in bad[:6]])
    bad = np.argwhere((grows != wrows).any(axis=-1))
    assert bad.size == 0, (what, "rows: pair, row", bad[:6].tolist(), [list(pairs[p]) for p, _ in bad[:3]], "got", [grows[tuple(b)].tolist() for b in bad[:6]],
                           "want", [wrows[tuple(b)].tolist() for b in bad[:6]])


def stage_best(c, spans, max_cost):
    """vbz_gpu_match_best_batch over spans uint32 [n, R, 4] -> uint32 [n, 4]; the guard entry keeps its canary"""
    n, R = spans.shape[0], spans.shape[1]
    s = torch.from_numpy(np.ascontiguousarray(spans).view(np.int32)).to(c.device)
    out = torch.full((n + 1, 4), HIT_CANARY, dtype=torch.int32, device=c.device)
    torch.cuda.synchronize()
    rc = c.L.vbz_gpu_match_best_batch(c.ctx, n, s.data_ptr(), R, max_cost, out.data_ptr())
    c.synchronize()
    assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)
    got = out.cpu().numpy().view(np.uint32)
    assert (got[n] == HIT_CANARY).all(), "the pair behind the last read was written"
    return got[:n]
