"""The sweep of tests/match_sweep.py on the MI355X: every loop the compiler emits for csrc/match.hip, run.  A dense sweep of n, M and W
= 1 ... 136 with garbage behind every read's and every reference's end (A, C, G), one reference per (rows per lane, tracked row) of the
packed span kernel (B), paths for every class (D), stretched copies that make the traceback refetch inside one lane's stream (E) and the
packed key's bound with both fields full (F) -- each beside a twin in an arena that runs the wide kernel and must write the same words.
Everything goes through the stage helpers of match_support, match_span_support and match_path_support (canaries, guard rows) and is
compared bit for bit with match_ref.hits, match_span_ref.spans and match_path_ref.paths.  tests/test_match_sweep_host.py holds the
census on the CPU."""
import numpy as np
import pytest

import match_path_ref as P
import match_ref as M
import match_sweep as W
from match_path_support import assert_paths, stage_path
from match_span_support import stage_span
from match_support import assert_hits, stage
from typed_support import codec

pytestmark = pytest.mark.gpu


def run_path(c, pc):
    query, valid, ref, ref_len = pc.call.arrays()
    return stage_path(c, query, valid, pc.call.quant, ref, ref_len, pc.pairs, pc.max_width)


def check_walks(pc, hit, rows, pairs=None):
    """test_gpu_match_path.test_path_catalogue's checks of what the device wrote: the hit's fields, the chain of the rows, the path
    re-costed from the quantised query, zeros behind the reference's end"""
    query, valid, ref, ref_len = pc.call.arrays()
    K = M.quantize(query, pc.call.quant)
    for p in range(len(pc.pairs)) if pairs is None else pairs:
        rd, rf, a, b = pc.pairs[p]
        m = int(ref_len[rf])
        r = rows[p, :m].astype(np.int64)
        assert int(hit[p][3]) == m and int(hit[p][1]) == b and r[0][0] == int(hit[p][2]) >= a and r[-1][1] == b, (pc.name, p)
        assert (r[:, 0] < r[:, 1]).all() and ((r[1:, 0] == r[:-1, 1]) | (r[1:, 0] == r[:-1, 1] - 1)).all(), (pc.name, p)
        assert P.recost(ref[rf, :m], K[rd], r) == int(hit[p][0]), (pc.name, p)
        assert not rows[p, m:].any(), (pc.name, p)


def check_spans(c, call, spans, hits):
    """the span call against `spans`, the cost-only call against `hits`, the two launches against each other, `zero`"""
    got = stage_span(c, call)
    assert_hits(got, spans, call.name)
    assert (got[:, :, 3] == 0).all(), "zero"
    cost = stage_span(c, call, cost_only=True)
    assert_hits(cost, hits, (call.name, "vbz_gpu_match_batch"))
    assert_hits(got[:, :, :2], cost, (call.name, "against vbz_gpu_match_batch"))
    return got


# ---- A. dense ---------------------------------------------------------------------------------------------------------------------------------
def test_dense():
    c = codec()
    a = W.dense()
    assert_hits(stage(c, a), W.dense_hits(), a.name)
    check_spans(c, a, W.dense_spans(), W.dense_hits())


def test_dense_in_a_wide_arena():
    """the same rows at N = 65 536: the wide kernel, the same hits"""
    wide = W.widen(W.dense(), N=W.DENSE_WIDE_N)
    assert W.instantiation("span", wide.N, wide.stride, 100)[0] == W.SPAN_WIDE
    got = stage_span(codec(), wide)
    assert_hits(got, W.dense_spans(), wide.name)
    assert (got[:, :, 3] == 0).all(), "zero"


# ---- B. every instantiation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["packed", "wide"])
def test_every_instantiation(wide):
    b = W.widen(W.every(), N=W.EVERY_WIDE_N) if wide else W.every()
    assert W.packed(b.N, b.stride) != wide
    check_spans(codec(), b, W.every_spans(), W.every_hits())


# ---- C. dense paths -----------------------------------------------------------------------------------------------------------------------------
def test_dense_paths():
    pc = W.dense_paths()
    hit, rows = run_path(codec(), pc)
    assert_paths((hit, rows), W.dense_paths_expected(), pc.pairs, pc.name)
    check_walks(pc, hit, rows)


def test_dense_paths_under_the_wide_key():
    pc = W.dense_paths_wide()
    pick = list(W.dense_paths_wide_pick())
    whit, wrows = W.dense_paths_expected()
    hit, rows = run_path(codec(), pc)
    assert_paths((hit, rows), (whit[pick], wrows[pick]), pc.pairs, pc.name)
    check_walks(pc, hit, rows)


# ---- D. paths per class -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["packed", "wide"])
def test_paths_per_class(wide):
    pc = W.class_paths(wide)
    assert W.packed(pc.max_width, pc.call.stride) != wide
    hit, rows = run_path(codec(), pc)
    assert_paths((hit, rows), W.class_paths_expected(), pc.pairs, pc.name)
    check_walks(pc, hit, rows)


# ---- E. stretched copies ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["packed", "wide"])
def test_stretched_copies(wide):
    pc, what = W.stretched(wide)
    assert W.packed(pc.max_width, pc.call.stride) != wide
    hit, rows = run_path(codec(), pc)
    for p, ((_, rf, _, b), (i0, L)) in enumerate(zip(pc.pairs, what)):   # the planted answer, read off the device's words
        m = int(pc.call.ref_len[rf])
        assert hit[p].tolist() == [0, b, W.STRETCH_BG, m], (pc.name, p, hit[p].tolist())
        width = (rows[p, :m, 1].astype(np.int64) - rows[p, :m, 0]).tolist()
        assert width == [L if i == i0 else 1 for i in range(m)], (pc.name, p, m, i0, L)
    assert_paths((hit, rows), W.stretched_expected(), pc.pairs, pc.name)
    check_walks(pc, hit, rows)


# ---- F. the bound -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(W.BOUND)), ids=["%d-%d" % s for s in W.BOUND])
def test_the_packed_keys_bound(index):
    c = codec()
    N, stride = W.BOUND[index]
    f = W.bound(index)
    want = W.bound_spans(index)
    assert W.packed(N, stride) and want[0][0].tolist() == [254 * stride, N, N - 1, 0]
    got = stage_span(c, f)
    assert got[0][0].tolist() == [254 * stride, N, N - 1, 0], (f.name, got[0][0].tolist())
    assert_hits(got, want, f.name)
    wN, ws = W.bound_wide(N, stride)
    assert not W.packed(wN, ws)
    assert_hits(stage_span(c, W.widen(f, N=wN, stride=ws)), want, (f.name, "wide", wN, ws))
    pc, (whit, wrows) = W.bound_paths(index)
    hit, rows = run_path(c, pc)
    assert hit.tolist() == [[254 * stride, N, N - 1, stride]] and (rows[0] == np.array([N - 1, N], np.uint32)).all(), (f.name, hit.tolist())
    assert_paths((hit, rows), (whit, wrows), pc.pairs, pc.name)


# ---- G. consistency over A ------------------------------------------------------------------------------------------------------------------------
def test_the_window_of_every_dense_span_gives_its_hit():
    """(a, b) = (start, end) of the span of every pair of A: the path call's hit is {cost, end, start, M} of the span call"""
    pc, want = W.dense_windows()
    hit, rows = run_path(codec(), pc)
    bad = np.argwhere((hit != want).any(axis=-1))[:, 0]
    assert bad.size == 0, ("pairs", [(int(p), list(pc.pairs[p]), hit[p].tolist(), want[p].tolist()) for p in bad[:6]])
    check_walks(pc, hit, rows, range(0, len(pc.pairs), 7))
