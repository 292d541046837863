"""vbz_gpu_locate_levels_batch on the MI355X, bit for bit against eventalign_ref's numpy statement, canary words around every arena: planted
paths of every length and width, diagonals, one entry over many levels, one level holding many entries with the stall at every residue of
a 64-entry turn; the tables at the edges of their ranges; refused pairs, each alone among good ones; max_width at and above the widest."""
import re

import numpy as np
import pytest
import torch

import eventalign_ref as E
from eventalign_support import assert_levels, dev_u32, dev_u64, records_of, stage_levels
from typed_support import codec

pytestmark = pytest.mark.gpu

SHAPES, TABLES = E.levels_shapes(), E.levels_tables()


def _ids(names):
    return [re.sub(r"[^A-Za-z0-9]+", "-", n)[:60] for n in names]


@pytest.mark.parametrize("call", SHAPES, ids=_ids(c.name for c in SHAPES))
def test_path_shapes(call):
    want = call.expected()
    assert_levels(stage_levels(codec(), call), want, call)


@pytest.mark.parametrize("call", TABLES, ids=_ids(c.name for c in TABLES))
def test_tables(call):
    want = call.expected()
    assert_levels(stage_levels(codec(), call), want, call)


@pytest.mark.parametrize("name", E.BROKEN, ids=_ids(E.BROKEN))
def test_a_broken_pair_gets_no_levels(name):
    """each condition alone among good pairs, at the table's start, in its middle and at its end"""
    c = codec()
    for at in (0, 2, 4):
        call, p = E.levels_broken(name, at)
        want = call.expected()
        got = stage_levels(c, call)
        assert_levels(got, want, call)
        assert got[0][p] == 0 and not got[1][p].any() and (np.delete(got[0], p) > 0).all(), (name, at, got[0].tolist())


def test_max_width_at_and_above_the_widest():
    c = codec()
    rng = np.random.default_rng(5)
    paths = [E.random_path(rng, 50, 64, 3), E.random_path(rng, 9, 8, 0), E.random_path(rng, 70, 33, 900)]
    for W in (64, 72, 512):
        call = E.call_of("max_width %u" % W, rng, paths, W=W, gaps=True)
        want = call.expected()
        assert want[0].tolist() == [64, 8, 33]
        assert_levels(stage_levels(c, call), want, call)


def test_the_python_method():
    c = codec()
    call = TABLES[0]
    pairs, hit, rows, index, first, event_rows, start, n, moments, n_reads = call.arrays()
    want = call.expected()
    P = len(pairs)
    nl, lv = c.locate_levels(dev_u32(c, pairs).reshape(P, 4), dev_u32(c, hit).reshape(P, 4), dev_u32(c, rows).reshape(P, call.N, 2), dev_u64(c, first),
                             dev_u32(c, start), records_of(c, np.zeros(len(n)), n).reshape(-1, 4), dev_u64(c, moments).reshape(-1, 2), call.W,
                             index=dev_u32(c, index).reshape(n_reads, call.N))
    c.synchronize()
    assert nl.dtype == torch.int32 and tuple(lv.shape) == (P, call.W, 8)
    assert_levels((nl.cpu().numpy().view(np.uint32), lv.cpu().numpy().view(np.uint32)), want, call)
    sums = lv.view(torch.int64)[..., 2:].cpu().numpy().view(np.uint64)
    assert (sums[..., 0] == (want[1][..., 4].astype(np.uint64) | want[1][..., 5].astype(np.uint64) << np.uint64(32))).all()
