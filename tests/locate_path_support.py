"""The raw locate path calls for the tests on the MI355X (test_gpu_locate_path, test_gpu_locate_path_refusals): what match_path_support is
to the match path.  vbz_gpu_locate_path_batch over one pair table into canary-filled hit and row arenas with a guard entry behind each
(match_path_support.PathArenas), the same cells through vbz_gpu_match_path_batch with the roles swapped, and vbz_gpu_query_valid_batch
into a canary-filled table.  A plain module: every assert carries its operands."""
import ctypes

import numpy as np
import torch

import match_ref as M
from locate_support import locate_struct
from match_path_support import PathArenas, path_struct
from match_path_support import stage_path as match_stage_path
from match_support import HIT_CANARY
from typed_support import i32, ranges_struct

EMPTY = [0xFFFFFFFF, 0, 0, 0]


def stage_path(c, query, valid, quant, target, target_len, pairs, max_width):
    """vbz_gpu_locate_path_batch -> (hit uint32 [pairs, 4], rows uint32 [pairs, N, 2]).  query float32 [reads, N], valid and target_len
    any integers, pairs any integers [pairs, 4]; the query keeps its bits"""
    n, N = query.shape
    m, keep = locate_struct(c, N, quant, target, target_len)
    q = torch.from_numpy(np.array(query, np.float32)).to(c.device)
    v = i32(valid).to(c.device)
    pr = i32(np.asarray(pairs, np.uint64).reshape(-1)).reshape(-1, 4).to(c.device)
    a = PathArenas(c, len(pairs), N)
    path = path_struct(max_width)
    torch.cuda.synchronize()
    rc = c.L.vbz_gpu_locate_path_batch(c.ctx, len(pairs), n, q.data_ptr(), v.data_ptr(), ctypes.byref(m), pr.data_ptr(), ctypes.byref(path),
                                       a.hit.data_ptr(), a.rows.data_ptr())
    c.synchronize()
    assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)
    assert (q.cpu().numpy().view(np.uint32) == np.ascontiguousarray(query).view(np.uint32)).all(), "the path call wrote its query"
    return a.read()


def run_call(c, pc):
    """one call of locate_path_ref's catalogue"""
    query, valid, target, target_len = pc.call.arrays()
    return stage_path(c, query, valid, pc.call.quant, target, target_len, pc.pairs, pc.max_width)


def swapped_match_path(c, query, valid, quant, target, target_len, pairs, max_width):
    """the same cells through vbz_gpu_match_path_batch with the roles swapped (locate_support.swapped_match's construction: targets of at
    most 65 536 levels and without -128 written out as float32 "queries", at most 4 096 reads' levels as int8 "references" of M = n in rows
    of a multiple of 16) -> (hit, rows uint32 [pairs, N, 2]); the rows behind N are {0, 0}"""
    N, stride = query.shape[1], target.shape[1]
    assert stride <= 65536 and stride % 8 == 0 and len(query) <= 4096 and int(np.min(target)) > -128
    L = np.asarray(target_len, np.uint64)
    tvalid = np.where((L != 0) & (L <= stride), L, 0).astype(np.uint32)
    tq = np.ascontiguousarray(np.asarray(target, np.float32) / np.float32(quant))
    levels = np.zeros((len(query), (N + 15) // 16 * 16), np.int8)
    levels[:, :N] = M.quantize(query, quant)
    n = np.minimum(np.asarray(valid, np.uint64), N).astype(np.uint32)
    swapped = [(tg, rd, a, b) for rd, tg, a, b in pairs]
    hit, rows = match_stage_path(c, tq, tvalid, quant, levels, n, swapped, max_width)
    assert not rows[:, N:].any()
    return hit, rows[:, :N]


def stage_query_valid(c, result, query_len, begin=None, end=None):
    """vbz_gpu_query_valid_batch -> uint32 [n]; the guard entry behind the table keeps its canary"""
    n = len(result)
    res = i32(result).to(c.device)
    out = torch.full((n + 1,), HIT_CANARY, dtype=torch.int32, device=c.device)
    g, keep = ranges_struct(c, begin, end, 0)
    torch.cuda.synchronize()
    rc = c.L.vbz_gpu_query_valid_batch(c.ctx, n, res.data_ptr(), ctypes.byref(g) if (begin is not None or end is not None) else None, query_len,
                                       out.data_ptr())
    c.synchronize()
    assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)
    got = out.cpu().numpy().view(np.uint32)
    assert got[n] == HIT_CANARY, "the entry behind the last read was written"
    return got[:n]
