"""The warping path of chosen pairs in target coordinates on the MI355X (include/vbz_gpu.h: vbz_gpu_locate_path_batch,
vbz_gpu_query_valid_batch).  The path call runs locate_path_ref's catalogue -- every n of 1 ... 136 and both sides of every change of the
rows per lane against windows on both sides of the direction words' seams; the byte stream (every residue of a and b mod 4, a == 0,
b == L with L no multiple of 4, junk behind L, windows across the loader's block of 256 steps), a call a part; two-level alphabets and
plateaus; a run of the query's first level in front of a plant; target levels of -128; one data set under the packed and the wide key; a
window behind level 65 536 -- hits and rows bit for bit against numpy through canary arenas with a guard entry, the planted answers known
without the DP, every path re-costed.  The same cells through vbz_gpu_match_path_batch with the roles swapped give the same bytes wherever
that call can express them; group boundaries under a small cap change nothing; span -> best -> path gives the span's (cost, start); the
fused chain signal_locate_span -> query_valid -> best -> path runs with no host copy and is held to the numpy-decoded signal."""
import numpy as np
import pytest
import torch

import locate_path_ref as LP
import locate_span_ref as LS
import match_path_ref as P
import match_ref as M
from locate_path_support import EMPTY, run_call, stage_path, stage_query_valid, swapped_match_path
from locate_span_support import SpanCall, SpanRun
from locate_span_support import stage_arrays as span_stage_arrays
from match_path_support import assert_paths
from match_support import query_rows
from ranges_ref import pod5_signals
from test_gpu_locate import O, POD5_SHAPES, S, TO_END, pod5_targets, targets_for
from typed_support import Frames, codec, expect_results, frames_of, i32, sine_signal, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

CALLS = [(i, c.name) for i, c in enumerate(LP.catalogue())]
SWAPPABLE = [(i, name) for i, name in CALLS if LP.catalogue()[i].call.stride <= 65536]


def check_paths(pc, hit, rows):
    """every path re-costed from the quantised query, and the chain of its rows"""
    query, valid, target, target_len = pc.call.arrays()
    K = M.quantize(query, pc.call.quant)
    for p, (rd, tg, a, b) in enumerate(pc.pairs):
        n = min(int(valid[rd]), pc.call.N)
        r = rows[p, :n].astype(np.int64)
        assert int(hit[p][3]) == n and int(hit[p][1]) == b and r[0][0] == int(hit[p][2]) >= a and r[-1][1] == b, (pc.name, p)
        assert (r[:, 0] < r[:, 1]).all() and ((r[1:, 0] == r[:-1, 1]) | (r[1:, 0] == r[:-1, 1] - 1)).all(), (pc.name, p)
        assert P.recost(K[rd, :n], target[tg].astype(np.int64), r) == int(hit[p][0]), (pc.name, p)
        assert not rows[p, n:].any()


# ---- 1. the stage entry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [i for i, _ in CALLS], ids=[name for _, name in CALLS])
def test_path_catalogue(index):
    pc = LP.catalogue()[index]
    hit, rows = run_call(codec(), pc)
    for p, (phit, prows) in pc.planted.items():   # known without the DP
        assert hit[p].tolist() == list(phit) and rows[p, : phit[3]].tolist() == prows, (pc.name, "planted", p, hit[p].tolist(), phit)
    assert_paths((hit, rows), LP.expected(index), pc.pairs, pc.name)
    assert (hit[:, 0] != EMPTY[0]).all(), "every pair of the catalogue has a path"
    check_paths(pc, hit, rows)


def test_both_keys_give_identical_paths():
    """query_len 2 048: max_width 4 096 runs the packed key, 4 104 the wide one (csrc/match_select.h); one pair is 2 048 x 4 096"""
    c = codec()
    keys = [pc for pc in LP.catalogue() if pc.name.startswith("keys-")]
    assert [(pc.call.N, pc.max_width) for pc in keys] == [(2048, 4096), (2048, 4104)] and keys[0].pairs[0][2:] == (0, 4096)
    (hit, rows), (whit, wrows) = (run_call(c, pc) for pc in keys)
    assert (hit == whit).all() and (rows == wrows).all() and int(hit[0][3]) == 2048


def test_junk_behind_the_target_changes_nothing():
    pc = next(pc for pc in LP.catalogue() if pc.name == "bytes-junk")
    hit, rows = run_call(codec(), pc)
    assert (hit[0::2] == hit[1::2]).all() and (rows[0::2] == rows[1::2]).all()
    assert (pc.call.targets[0][1003:] != pc.call.targets[1][1003:]).any()


def test_a_window_behind_level_65536():
    pc = LP.catalogue()[-1]
    assert pc.name == "beyond" and pc.pairs[0][2] > 65536
    hit, rows = run_call(codec(), pc)
    (phit, prows), = pc.planted.values()
    assert hit[0].tolist() == list(phit) and rows[0, :200].tolist() == prows and not rows[0, 200:].any()


@pytest.mark.parametrize("index", [i for i, _ in SWAPPABLE], ids=[name for _, name in SWAPPABLE])
def test_swapped_match_path_gives_the_same_bytes(index):
    """every call the match path can express (at most 4 096 reads, L <= 65 536): the same cells both ways; -128 raised to -127 on both
    sides, as test_gpu_locate does"""
    pc = LP.catalogue()[index]
    c = codec()
    query, valid, target, target_len = pc.call.arrays()
    target = np.maximum(target, -127)
    got = stage_path(c, query, valid, pc.call.quant, target, target_len, pc.pairs, pc.max_width)
    want = swapped_match_path(c, query, valid, pc.call.quant, target, target_len, pc.pairs, pc.max_width)
    assert_paths(got, want, pc.pairs, pc.name)
    assert (got[0][:, 0] != EMPTY[0]).all()


@pytest.mark.parametrize("group", [1, 2, 72])
def test_group_boundaries_give_the_same_bytes(group):
    """a cap of `group` pairs' bits (72: the whole table); a cap below one pair's bits: every pair runs alone"""
    pc = next(pc for pc in LP.catalogue() if pc.name == "ties")
    assert len(pc.pairs) == 72 and (pc.call.N, pc.max_width) == (136, 304)
    words = 64 * (((63 + 304) * 4 + 15) // 16)   # match_path_groups.h: max_width 304, query_len 136 (four rows a lane)
    want = LP.expected(LP.catalogue().index(pc))
    for cap, launches in ((group * words * 4, (72 + group - 1) // group), (words * 4 - 4, 72) if group == 1 else (None, 1)):
        c = codec(VBZ_HIP_MATCH_PATH_CAP=cap) if cap is not None else codec()
        c.profile_reset()
        c.profile(True)
        got = run_call(c, pc)
        seen = c.profile_read().get("locate_path_forward", (0, 0.0))[0]
        c.profile(False)
        assert_paths(got, want, pc.pairs, ("cap", cap))
        assert seen == launches, ("groups", cap, seen, launches)


def test_span_then_best_then_path():
    """vbz_gpu_locate_span_batch -> best -> path on the device's own arenas: every hit's (cost, start) is the span's"""
    c = codec()
    call = next(x for x in LS.catalogue() if x.name == "span-planted-129")
    query, valid, target, target_len = call.arrays()
    n, G = len(query), len(target)
    got, spans_d = span_stage_arrays(c, query, valid, call.quant, target, target_len, keep_out=True)
    # every (read, target) of the arena as a pair, and the winners' table
    every = [(rd, tg, int(got[rd][tg][2]), int(got[rd][tg][1])) for rd in range(n) for tg in range(G)]
    width = (max(b - a for _, _, a, b in every) + 7) // 8 * 8
    hit, rows = stage_path(c, query, valid, call.quant, target, target_len, every, width)
    assert hit[:, :3].tolist() == [got[rd][tg][:3].tolist() for rd, tg, _, _ in every]
    earlier = [(rd, tg, a // 2, b) for rd, tg, a, b in every if b - a // 2 <= 2048]   # any a' <= start with the same b
    assert earlier
    hit2, _ = stage_path(c, query, valid, call.quant, target, target_len, earlier, 2048)
    assert hit2[:, :3].tolist() == [got[rd][tg][:3].tolist() for rd, tg, _, _ in earlier]
    dev = c.device
    pairs = c.match_best(spans_d[:n])
    lc = batch.Locate(call.N, call.quant)
    h, r = c.locate_path(torch.from_numpy(np.array(query)).to(dev), i32(valid).to(dev), torch.from_numpy(np.array(target)).to(dev), i32(target_len).to(dev),
                         pairs, width, lc)
    torch.cuda.synchronize()
    table = pairs.cpu().numpy().view(np.uint32)
    assert (table == P.best(got)).all()
    want = LP.paths(query, valid, call.quant, target, target_len, table, width)
    assert_paths((h.cpu().numpy().view(np.uint32), r.cpu().numpy().view(np.uint32)), want, table.tolist(), "winners")
    for i in range(n):
        assert want[0][i][:3].tolist() == got[i][int(table[i][1])][:3].tolist()


# ---- 2. query_valid and the fused chain -----------------------------------------------------------------------------------------------------
def test_query_valid():
    c = codec()
    E = LP.E_FIRST
    res = [4 * 100, 4 * 5, 0, E, 0xFFFFFFFF, 4 * 3000, 4 * 100, E + 7, 4 * 64, 4 * 65]
    for N in (8, 64, 2048, 65536):
        assert stage_query_valid(c, res, N).tolist() == LP.query_valid(res, N).tolist() == [min(r // 4, N) if r < E else 0 for r in res]
        bg = [90, 9, 0, 0, 0, 2990, TO_END, 0, 1, 64]
        en = [TO_END, 3, 7, 1, 1, 3001, 50, 9, 64, 65]
        assert stage_query_valid(c, res, N, bg, en).tolist() == LP.query_valid(res, N, bg, en).tolist()
        assert stage_query_valid(c, res, N, bg, None).tolist() == LP.query_valid(res, N, bg, None).tolist()
        assert stage_query_valid(c, res, N, None, en).tolist() == LP.query_valid(res, N, None, en).tolist()
    assert stage_query_valid(c, [], 64).tolist() == []


def chain(c, query_d, hits_d, result_d, N, bg, en, target, lens, want_q, valid_want, want_spans, what):
    """query_valid -> best -> path behind a fused span call, on its device arenas; held to the statement on the numpy-decoded signal"""
    dev = c.device
    valid = c.query_valid(result_d, N, begin=bg, end=en)
    pairs = c.match_best(hits_d)
    width = max(8, (int((want_spans[:, :, 1] - want_spans[:, :, 2]).max()) + 7) // 8 * 8)
    hit, rows = c.locate_path(query_d, valid, torch.from_numpy(target).to(dev), i32(lens).to(dev), pairs, width, batch.Locate(N, 32.0))
    torch.cuda.synchronize()
    assert u32(valid).tolist() == list(valid_want), (what, u32(valid).tolist(), valid_want)
    table = pairs.cpu().numpy().view(np.uint32)
    assert (table == P.best(want_spans)).all(), what
    want = LP.paths(want_q.view(np.float32), valid_want, 32.0, target, lens, table, width)
    got = (hit.cpu().numpy().view(np.uint32), rows.cpu().numpy().view(np.uint32))
    assert_paths(got, want, table.tolist(), what)
    for i in range(len(table)):
        if table[i][1] != P.NONE:
            assert got[0][i][:3].tolist() == want_spans[i][int(table[i][1])][:3].tolist(), (what, i)
        else:
            assert got[0][i].tolist() == EMPTY and not got[1][i].any(), (what, i)
    return got


def test_fused_chain_with_no_host_copy():
    """reads shorter than N, a read with an error verdict, a range table"""
    c = codec()
    rng = np.random.default_rng(4320)
    T = [5000, 3000, 300, 900, 0, 2049, 700]
    fr = Frames(c, [sine_signal(rng, t) for t in T], c.options(True, 2, 1, 1))
    src = fr.src.clone()
    size = fr.size.clone()
    size[1] = int(u32(fr.size)[1]) // 2   # the frame of read 1 cut off in its middle
    fr.size = size
    n, N = fr.n, 512
    bg, en = [3, 0, 8, 500, 0, 2001, TO_END], [TO_END, TO_END, 290, 2600, TO_END, 2040, 0]
    o, s = np.full(n, O, np.float32), np.full(n, S, np.float32)
    want_q, _, Tp = query_rows(fr.reads, bg, en, N, list(zip(o, s)))
    target, lens, planted = targets_for(want_q, [min(t, N) for t in Tp], 32.0, rng)
    dst = torch.zeros(fr.dst_bytes + 64, dtype=torch.uint8, device=c.device)
    res16 = torch.full((n,), -8, dtype=torch.int32, device=c.device)
    c.decompress(src, fr.off, fr.size, dst, fr.doff, fr.dcap, res16, fr.opts)
    torch.cuda.synchronize()
    un = u32(res16).tolist()
    assert [_lib.is_error(v) for v in un] == [False, True] + [False] * 5
    run = SpanRun(fr, target, lens, N, 32.0, begin=bg, end=en, offset=o, scale=s, src=src).check(expect={1: un[1]})
    valid_want = [0 if i == 1 else min(Tp[i], N) for i in range(n)]
    assert 0 < valid_want[2] < N and 0 < valid_want[5] < N and valid_want[0] == N and valid_want[4] == 0 and valid_want[6] == 0
    got = chain(c, run.a.query[:n], run.a.out[:n], run.result[:n], N, bg, en, target, lens, want_q, valid_want, run.want, "fused")
    assert got[0][1].tolist() == EMPTY and got[0][4].tolist() == EMPTY and got[0][0][0] != EMPTY[0] and int(got[0][2][3]) == valid_want[2]


def test_fused_chain_over_pod5_reads():
    c = codec()
    rows, first, frames = frames_of(71, POD5_SHAPES)
    n, N = len(first), 512
    rng = np.random.default_rng(4321)
    o, s = np.full(n, O, np.float32), np.full(n, S, np.float32)
    consts = list(zip(o, s))
    sig = pod5_signals(rows, first)
    bg, en = [3, 8, 3, 2000, 701, TO_END, 0, 5], [TO_END, 3000, 1000, 2100, TO_END, 0, TO_END, 400]
    target, lens = pod5_targets(sig, bg, en, N, consts, None, 0, rng)
    call = SpanCall(c, frames, rows, first, target, lens, N, begin=bg, end=en, offset=o, scale=s)
    assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
    expect_results(call, rows, first, 4)
    call.check(consts=consts)
    want_q, _, Tp = query_rows(sig, bg, en, N, consts)
    valid_want = [min(t, N) for t in Tp]
    assert any(0 < v < N for v in valid_want) and any(v == 0 for v in valid_want)
    chain(c, call.a.query[:n], call.a.out[:n], call.read_result[:n], N, bg, en, target, lens, want_q, valid_want, call.want, "pod5")


# ---- 3. the Python methods --------------------------------------------------------------------------------------------------------------------
def test_python_methods():
    c = codec()
    dev = c.device
    rng = np.random.default_rng(4322)
    z = rng.normal(0, 1.2, (5, 256)).astype(np.float32)
    target = rng.integers(-60, 61, (2, 4096)).astype(np.int8)
    target[0, 3001:3101] = batch.quantize_levels(z[2, :100], 32.0)   # the whole query of read 2 stands in target 0
    lens = [4095, 777]
    valid = [256, 255, 100, 0, 300]
    pairs = [(0, 0, 1, 300), (1, 1, 500, 777), (2, 0, 2990, 3101), (3, 0, 0, 8), (4, 1, 0, 256), (2, 0, 2990, 4096), (9, 0, 0, 8)]
    hit0 = torch.full((len(pairs), 4), 7, dtype=torch.int32, device=dev)
    hit, rows = c.locate_path(torch.from_numpy(z).to(dev), i32(valid).to(dev), torch.from_numpy(target).to(dev), i32(lens).to(dev),
                              i32(np.asarray(pairs).reshape(-1)).reshape(-1, 4).to(dev), 304, hit=hit0)
    torch.cuda.synchronize()
    assert hit is hit0 and tuple(rows.shape) == (len(pairs), 256, 2)
    got = (hit.cpu().numpy().view(np.uint32), rows.cpu().numpy().view(np.uint32))
    assert_paths(got, LP.paths(z, valid, 32.0, target, lens, pairs, 304), pairs, "method")
    assert got[0][2][:2].tolist() == [0, 3101] and int(got[0][2][3]) == 100 and int(got[1][2][99][1]) == 3101
    assert [h.tolist() == EMPTY for h in got[0]] == [False, False, False, True, False, True, True]
    res = i32([4 * 1000, LP.E_FIRST + 1, 4 * 17]).to(dev)
    out = torch.zeros(3, dtype=torch.int32, device=dev)
    assert c.query_valid(res, 256, out=out) is out and u32(c.query_valid(res, 256, begin=[990, 0, 20])).tolist() == [10, 0, 0]
    torch.cuda.synchronize()
    assert u32(out).tolist() == [256, 0, 17]
