"""What vbz_gpu_locate_path_batch and vbz_gpu_query_valid_batch refuse (include/vbz_gpu.h).  On the host, -2 with nothing launched and
canary-filled hits and rows untouched: everything vbz_gpu_locate_batch refuses about locate, misalignment, path NULL or outside its rules,
NULL tables while the call has pairs -- valid among them, unlike the match path -- and implausible extents.  On the device, per pair: every
condition of the untrusted pair table, each alone in a table among good pairs that keep their answers, gives the empty verdict -- the hit
{0xFFFFFFFF, 0, 0, 0}, every row {0, 0}.  A call of no pairs is queued and writes nothing."""
import ctypes
import re

import numpy as np
import pytest
import torch

import locate_path_ref as LP
from locate_path_support import EMPTY, stage_path
from locate_support import locate_struct
from match_path_support import PathArenas, assert_paths, path_struct
from match_support import HIT_CANARY
from typed_support import codec, i32

pytestmark = pytest.mark.gpu

N, G, STRIDE, WIDTH = 32, 3, 64, 48


class Setup:
    def __init__(self):
        c = self.c = codec()
        rng = np.random.default_rng(4330)
        self.query = rng.normal(0, 1.5, (4, N)).astype(np.float32)
        self.target = rng.integers(-100, 101, (G, STRIDE)).astype(np.int8)
        self.target_len = [50, 64, 7]
        self.valid_host = [N, 20, 5000, 0]
        self.q = torch.from_numpy(self.query).to(c.device)
        self.valid = i32(self.valid_host).to(c.device)
        self.pairs = [(0, 0, 3, 40), (1, 1, 16, 64), (2, 2, 0, 7)]
        self.pr = i32(np.asarray(self.pairs, np.uint64).reshape(-1)).reshape(-1, 4).to(c.device)
        self.a = PathArenas(c, len(self.pairs), N)

    def call(self, m, path="ok", n_pairs=None, n_reads=4, query="ok", valid="ok", pairs="ok", hit="ok", rows="ok"):
        c = self.c
        pick = lambda v, t: t.data_ptr() if isinstance(v, str) else v   # noqa: E731
        pp = ctypes.byref(path_struct(WIDTH)) if isinstance(path, str) else (ctypes.byref(path) if path is not None else None)
        rc = c.L.vbz_gpu_locate_path_batch(c.ctx, len(self.pairs) if n_pairs is None else n_pairs, n_reads, pick(query, self.q), pick(valid, self.valid),
                                           ctypes.byref(m) if m is not None else None, pick(pairs, self.pr), pp, pick(hit, self.a.hit), pick(rows, self.a.rows))
        return rc, c.L.vbz_gpu_last_error(c.ctx).decode()

    def struct(self, **kw):
        args = {"N": N, "quant": 32.0, "target": self.target, "target_len": self.target_len}
        flags = {k: kw.pop(k) for k in ("flags", "reserved") if k in kw}
        args.update(kw)
        return locate_struct(self.c, args["N"], args["quant"], args["target"], args["target_len"], **flags)


def refused(got, text):
    rc, msg = got
    assert rc == -2 and text in msg, (rc, msg, text)


def test_host_refusals_launch_nothing():
    s = Setup()
    m, keep = s.struct()
    # NULL tables while the call has pairs: valid is REQUIRED here
    refused(s.call(None), "locate is NULL")
    refused(s.call(m, path=None), "path is NULL")
    for name in ("query", "valid", "pairs", "hit", "rows"):
        refused(s.call(m, **{name: None}), "is NULL")
    for field in ("target", "target_len"):
        m2, keep2 = s.struct()
        setattr(m2, field, None)
        refused(s.call(m2), "is NULL")
    # misalignment
    refused(s.call(m, query=s.q.data_ptr() + 4), "not 16-byte aligned")
    refused(s.call(m, hit=s.a.hit.data_ptr() + 8), "not 16-byte aligned")
    refused(s.call(m, pairs=s.pr.data_ptr() + 8), "not 16-byte aligned")
    refused(s.call(m, rows=s.a.rows.data_ptr() + 8), "not 16-byte aligned")
    m2, keep2 = s.struct()
    m2.target = m2.target + 8
    refused(s.call(m2), "not 16-byte aligned")
    # the path struct
    for width in (0, 4, 12, 65544, 1 << 31):
        refused(s.call(m, path=path_struct(width)), "path is NULL or outside the rules")
    refused(s.call(m, path=path_struct(WIDTH, flags=1)), "outside the rules")
    refused(s.call(m, path=path_struct(WIDTH, reserved=1 << 40)), "outside the rules")
    # everything vbz_gpu_locate_batch refuses about locate
    for kw in ({"N": 0}, {"N": 4}, {"N": 36}, {"N": 2056}, {"quant": 0.0}, {"quant": -1.0}, {"quant": float("nan")}, {"quant": float("inf")}, {"flags": 1},
               {"reserved": 1}):
        refused(s.call(s.struct(**kw)[0]), "locate outside the rules")
    for field, v in (("n_targets", 0), ("n_targets", 4097), ("target_stride", 0), ("target_stride", 24), ("target_stride", (1 << 30) + 16)):
        m2, keep2 = s.struct()
        setattr(m2, field, v)
        refused(s.call(m2), "locate outside the rules")
    # (the extent rules -- n_pairs * N * 8, n_reads * N * 4, G * target_stride beyond 2^46 bytes -- are the host's own arithmetic in 64 bits: with
    # N <= 2 048, G <= 4 096 and target_stride <= 2^30 no count of 32 bits reaches them; the largest declarable arenas are accepted)
    m2, keep2 = s.struct(N=2048)
    m2.n_targets, m2.target_stride = 4096, 1 << 30
    assert s.call(m2, n_pairs=0, n_reads=0xFFFFFFFF)[0] == 0
    torch.cuda.synchronize()
    assert s.a.untouched() and (s.q.cpu().numpy().view(np.uint32) == s.query.view(np.uint32)).all()
    # ... and the same arguments, unspoilt, run
    assert s.call(m)[0] == 0
    s.c.synchronize()
    hit, rows = s.a.read()
    assert_paths((hit, rows), LP.paths(s.query, s.valid_host, 32.0, s.target, s.target_len, s.pairs, WIDTH), s.pairs, "unspoilt")
    assert (hit[:, 0] != EMPTY[0]).all()


def test_no_pairs():
    """queued, nothing launched, nothing written, NULL tables allowed; a NULL context is -1"""
    s = Setup()
    m, keep = s.struct()
    s.c.profile_reset()
    s.c.profile(True)
    assert s.call(m, n_pairs=0)[0] == 0
    assert s.call(m, n_pairs=0, pairs=None, hit=None, rows=None, query=None, valid=None)[0] == 0
    launches = s.c.profile_read().get("locate_path_forward", (0, 0.0))[0]
    s.c.profile(False)
    torch.cuda.synchronize()
    assert launches == 0 and s.a.untouched()
    refused(s.call(m, n_pairs=0, path=path_struct(12)), "outside the rules")   # bad arguments stay refused
    assert s.c.L.vbz_gpu_locate_path_batch(None, 0, 0, None, None, None, None, None, None, None) == -1


BIG = 0xFFFFFFFF
GOOD = [(0, 0, 3, 40), (1, 1, 16, 64), (2, 2, 0, 7), (2, 0, 2, 50), (1, 1, 63, 64)]
BAD = {
    "read >= n_reads": (4, 0, 0, 8), "read far out": (BIG, 0, 0, 8), "ref >= G": (0, 3, 0, 8), "the best call's none": (0, LP.NONE, 0, 0),
    "begin == end": (0, 0, 8, 8), "begin > end": (0, 0, 9, 8), "begin far out": (0, 0, BIG, 8), "n == 0": (3, 0, 0, 8), "end > L": (0, 0, 10, 51),
    "end far out": (0, 0, 0, BIG), "end > L, L < stride": (1, 2, 0, 8), "wider than max_width": (0, 1, 0, 49), "all far out": (BIG, BIG, BIG, BIG),
    "a wrapping width": (0, 3, BIG, BIG),
}


@pytest.mark.parametrize("name", list(BAD), ids=[re.sub(r"[^A-Za-z0-9]+", "-", k) for k in BAD])
def test_an_untrusted_pair_gets_the_empty_verdict(name):
    """each condition alone in a table among good pairs, at its start, in its middle and at its end"""
    s = Setup()
    for at in (0, 2, len(GOOD)):
        pairs = GOOD[:at] + [BAD[name]] + GOOD[at:]
        want = LP.paths(s.query, s.valid_host, 32.0, s.target, s.target_len, pairs, WIDTH)
        got = stage_path(s.c, s.query, s.valid_host, 32.0, s.target, s.target_len, pairs, WIDTH)
        assert_paths(got, want, pairs, name)
        for p in range(len(pairs)):
            assert (got[0][p].tolist() == EMPTY) == (p == at), (name, p, pairs[p], got[0][p].tolist())
        assert not got[1][at].any()


@pytest.mark.parametrize("target_len,dead", [([50, 0, 7], (1,)), ([65, 64, BIG], (0, 2)), ([50, 64, 0], (2,))], ids=["L0", "L-above-stride", "L0-last"])
def test_refused_target_lengths(target_len, dead):
    """L_g == 0 or L_g > target_stride: every pair of that target, beside the others"""
    s = Setup()
    want = LP.paths(s.query, s.valid_host, 32.0, s.target, target_len, GOOD, WIDTH)
    got = stage_path(s.c, s.query, s.valid_host, 32.0, s.target, target_len, GOOD, WIDTH)
    assert_paths(got, want, GOOD, target_len)
    for p, pr in enumerate(GOOD):
        assert (got[0][p].tolist() == EMPTY) == (pr[1] in dead), (p, pr, got[0][p].tolist())


def test_query_valid_refusals():
    c = codec()
    L = c.L
    res = i32([400, 8, 0]).to(c.device)
    out = torch.full((4,), HIT_CANARY, dtype=torch.int32, device=c.device)
    for args in ((3, None, None, 64, out.data_ptr()), (3, res.data_ptr(), None, 64, None), (3, res.data_ptr(), None, 0, out.data_ptr()),
                 (3, res.data_ptr(), None, 4, out.data_ptr()), (3, res.data_ptr(), None, 60, out.data_ptr()), (3, res.data_ptr(), None, 65544, out.data_ptr()),
                 (0, None, None, 12, None)):
        assert L.vbz_gpu_query_valid_batch(c.ctx, *args) == -2, args
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == HIT_CANARY).all()
    assert L.vbz_gpu_query_valid_batch(c.ctx, 0, None, None, 64, None) == 0 and L.vbz_gpu_query_valid_batch(None, 0, None, None, 64, None) == -1
