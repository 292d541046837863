"""The warping path of chosen pairs on the MI355X (include/vbz_gpu.h: vbz_gpu_match_best_batch, vbz_gpu_match_path_batch).  The path call
runs match_path_ref's catalogue -- every reference length against every width on both sides of the direction words' seams, two- and
three-level alphabets where all three predecessors tie, sits on row 0 whole and cut by the window, M = 1, W = 1, level -128, one pair of
2 048 x 4 096, one data set on both sides of the host's choice between the packed and the wide kernel -- hits and rows bit for bit against
match_path_ref, canaries behind every arena, every path re-costed from the quantised query.  The best call: ties, all-empty rows, max_cost
at, above and below the minimum, R = 1, 4, 5 and 4 096.  The chain: signal_match_span -> match_best -> match_path with no host copy."""
import numpy as np
import pytest
import torch

import match_path_ref as P
import match_ref as M
import match_span_ref as S
from match_path_support import EMPTY, assert_paths, stage_best, stage_path
from match_support import query_rows
from typed_support import Frames, arena, codec, frames_of, i32
from vbz_compression_amd import batch

pytestmark = pytest.mark.gpu

CALLS = [(i, c.name) for i, c in enumerate(P.catalogue())]


def run_call(c, pc):
    query, valid, ref, ref_len = pc.call.arrays()
    return stage_path(c, query, valid, pc.call.quant, ref, ref_len, pc.pairs, pc.max_width)


@pytest.mark.parametrize("index", [i for i, _ in CALLS], ids=[name for _, name in CALLS])
def test_path_catalogue(index):
    pc = P.catalogue()[index]
    hit, rows = run_call(codec(), pc)
    want = P.expected(index)
    assert_paths((hit, rows), want, pc.pairs, pc.name)
    assert (hit[:, 0] != EMPTY[0]).all(), "every pair of the catalogue has a path"
    # every path re-costed from the quantised query, and the chain of its rows
    query, valid, ref, ref_len = pc.call.arrays()
    K = M.quantize(query, pc.call.quant)
    for p, (rd, rf, a, b) in enumerate(pc.pairs):
        m = int(ref_len[rf])
        r = rows[p, :m].astype(np.int64)
        assert int(hit[p][3]) == m and int(hit[p][1]) == b and r[0][0] == int(hit[p][2]) >= a and r[-1][1] == b, (pc.name, p)
        assert (r[:, 0] < r[:, 1]).all() and ((r[1:, 0] == r[:-1, 1]) | (r[1:, 0] == r[:-1, 1] - 1)).all(), (pc.name, p)
        assert P.recost(ref[rf, :m], K[rd], r) == int(hit[p][0]), (pc.name, p)
        assert not rows[p, m:].any()


def test_both_sides_of_the_hosts_rule_give_identical_paths():
    c = codec()
    rule = [pc for pc in P.catalogue() if pc.name.startswith("rule")]
    assert [(pc.call.N, pc.call.stride, pc.max_width) for pc in rule] == [(4096, 2048, 4096), (8192, 2048, 8192), (16384, 416, 16384), (32768, 416, 32768)]
    got = [run_call(c, pc) for pc in rule]
    for (hit, rows), pc in zip(got[1:], rule[1:]):
        assert (hit == got[0][0]).all(), pc.name
        assert (rows[:, :416] == got[0][1][:, :416]).all() and not got[0][1][:, 416:].any(), pc.name


def test_a_window_of_the_span_call_gives_its_cost_and_start():
    """(a, b) = the span call's (start, end), and a' <= start: the hit is the span call's"""
    c = codec()
    call = S.span_catalogue()[0]   # ties-3
    query, valid, ref, ref_len = call.arrays()
    spans = S.expected(0)
    pairs, want = [], []
    for rd in range(len(query)):
        for rf in range(len(ref)):
            cost, end, start, _ = (int(v) for v in spans[rd][rf])
            for a in {start, start // 2, 0}:
                pairs.append((rd, rf, a, end))
                want.append((cost, end, start, int(ref_len[rf])))
    hit, _ = stage_path(c, query, valid, call.quant, ref, ref_len, pairs, call.N)
    assert hit.tolist() == [list(w) for w in want]


# ---- the winners' table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 4, 5, 4096])
def test_best(R):
    c = codec()
    rng = np.random.default_rng(R)
    n = 9
    spans = np.zeros((n, R, 4), np.uint32)
    spans[:, :, 0] = rng.integers(10, 14, (n, R))   # four costs: ties wherever R > 1
    spans[:, :, 1] = rng.integers(100, 200, (n, R))
    spans[:, :, 2] = rng.integers(0, 100, (n, R))
    spans[1, :] = (EMPTY[0], 0, 0, 0)                # an all-empty row
    spans[2, : R // 2] = (EMPTY[0], 0, 0, 0)         # empty verdicts in front of the winner
    spans[3, :, 0] = 12                              # all tie: reference 0
    spans[4, :, 0] = 12
    spans[4, R - 1, 0] = 11                          # the last reference wins
    low = int(spans[0, :, 0].min())
    for max_cost in (0xFFFFFFFF, low, low + 1, low - 1, 0):
        got = stage_best(c, spans, max_cost)
        assert got.tolist() == P.best(spans, max_cost).tolist(), (R, max_cost)
    assert stage_best(c, spans, 0xFFFFFFFF)[1].tolist() == [1, P.NONE, 0, 0] and stage_best(c, spans, low - 1)[0].tolist() == [0, P.NONE, 0, 0]
    assert stage_best(c, spans, 0xFFFFFFFF)[3][1] == 0 and stage_best(c, spans, 0xFFFFFFFF)[4][1] == R - 1


# ---- the chain: span -> best -> path, nothing crossing to the host between them --------------------------------------------------------------
def test_chain_of_three_calls():
    c = codec()
    dev = c.device
    lens = [0, 9, 300, 513, 2049, 4101, 700]
    rows, first, frames = frames_of(81, [[n] for n in lens])
    fr = Frames(c, rows, batch.pod5_options(), comp=arena(c, frames, 64))
    rng = np.random.default_rng(9)
    o, sc = -330.0, 1.0 / 45.0
    n, N = len(lens), 512
    want_q, _, Tp = query_rows(rows, [None] * n, [None] * n, N, [(o, sc)] * n)
    z = want_q.view(np.float32)
    ref = np.zeros((4, 416), np.int8)
    ref[0, :150] = M.quantize(z[3, 40:190], 32.0)   # a stretch of read 3 itself
    ref[1, :400] = np.clip(np.repeat(rng.integers(-70, 71, 67), 6)[:400] + rng.integers(-6, 7, 400), -127, 127)
    ref[2, :33] = rng.integers(-3, 4, 33)
    rl = [150, 400, 33, 0]
    ref_d, len_d = torch.from_numpy(ref).to(dev), i32(rl).to(dev)
    od, sd = torch.full((n,), o, dtype=torch.float32, device=dev), torch.full((n,), sc, dtype=torch.float32, device=dev)
    res = torch.full((n,), -8, dtype=torch.int32, device=dev)
    match = batch.Match(N, 32.0)
    spans, query = c.signal_match_span(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, ref_d, len_d, match, scale=sd, offset=od)
    pairs = c.match_best(spans)
    hit, prow = c.match_path(query, None, ref_d, len_d, pairs, N, match)   # (valid None: the fused call's query arena, +0 behind a read's end)
    torch.cuda.synchronize()
    spans, pairs, hit, prow = (t.cpu().numpy().view(np.uint32) for t in (spans, pairs, hit, prow))
    assert (query.cpu().numpy().view(np.uint32) == want_q).all()
    assert pairs.tolist() == P.best(spans).tolist()
    assert pairs[0].tolist() == [0, P.NONE, 0, 0] and hit[0].tolist() == EMPTY and not prow[0].any()
    assert pairs[3][1] == 0 and hit[3][0] == 0
    for i in range(1, n):
        rf = int(pairs[i][1])
        assert rf != P.NONE and hit[i].tolist() == spans[i][rf][:3].tolist() + [rl[rf]], (i, hit[i].tolist(), spans[i][rf].tolist())
    whit, wrows = P.paths(z, None, 32.0, ref, rl, pairs, N)
    assert_paths((hit, prow), (whit, wrows), pairs.tolist(), "chain")
