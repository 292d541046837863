"""What vbz_gpu_match_path_batch and vbz_gpu_match_best_batch refuse (include/vbz_gpu.h).  On the host, -2 with nothing launched and
canary-filled hits and rows untouched: NULL tables while the call has pairs, misalignment, path flags / reserved, max_width outside its
rule, everything vbz_gpu_match is refused for, implausible extents.  On the device, per pair: every condition of the untrusted pair table
gives the empty verdict -- the hit {0xFFFFFFFF, 0, 0, 0}, every row {0, 0} -- beside good pairs that keep their answers.  Calls of 0 and 1
pairs and of a group boundary - 1, + 0, + 1 pairs under a small cap (VBZ_HIP_MATCH_PATH_CAP, read when the context is created) give what
one group gives."""
import ctypes

import numpy as np
import pytest
import torch

import match_path_ref as P
from match_path_support import EMPTY, PathArenas, assert_paths, path_struct, stage_path
from match_support import HIT_CANARY, match_struct
from typed_support import codec, i32
from vbz_compression_amd import _lib

pytestmark = pytest.mark.gpu

N, R, STRIDE, WIDTH = 64, 3, 32, 48


class Setup:
    def __init__(self, c=None):
        c = self.c = c or codec()
        rng = np.random.default_rng(94)
        self.query = rng.normal(0, 1.5, (4, N)).astype(np.float32)
        self.ref = rng.integers(-100, 101, (R, STRIDE)).astype(np.int8)
        self.ref_len = [20, 32, 7]
        self.q = torch.from_numpy(self.query).to(c.device)
        self.valid = i32([N, N, 40, 0]).to(c.device)
        self.pairs = [(0, 0, 3, 40), (1, 1, 0, 48), (2, 2, 30, 40)]
        self.pr = i32(np.asarray(self.pairs, np.uint64).reshape(-1)).reshape(-1, 4).to(c.device)
        self.a = PathArenas(c, len(self.pairs), STRIDE)

    def call(self, m, path="ok", n_pairs=None, n_reads=4, query="ok", valid="ok", pairs="ok", hit="ok", rows="ok"):
        c = self.c
        pick = lambda v, t: t.data_ptr() if isinstance(v, str) else v
        pp = ctypes.byref(path_struct(WIDTH)) if isinstance(path, str) else (ctypes.byref(path) if path is not None else None)
        rc = c.L.vbz_gpu_match_path_batch(c.ctx, len(self.pairs) if n_pairs is None else n_pairs, n_reads, pick(query, self.q), pick(valid, self.valid),
                                          ctypes.byref(m) if m is not None else None, pick(pairs, self.pr), pp, pick(hit, self.a.hit), pick(rows, self.a.rows))
        return rc, c.L.vbz_gpu_last_error(c.ctx).decode()

    def struct(self, **kw):
        args = {"N": N, "quant": 32.0, "ref": self.ref, "ref_len": self.ref_len}
        flags = {k: kw.pop(k) for k in ("flags", "reserved") if k in kw}
        args.update(kw)
        return match_struct(self.c, args["N"], args["quant"], args["ref"], args["ref_len"], **flags)


def refused(got, text):
    rc, msg = got
    assert rc == -2 and text in msg, (rc, msg, text)


def test_host_refusals_launch_nothing():
    s = Setup()
    m, keep = s.struct()
    # NULL tables while the call has pairs (valid may be NULL)
    refused(s.call(None), "match is NULL")
    refused(s.call(m, path=None), "path is NULL")
    for name in ("query", "pairs", "hit", "rows"):
        refused(s.call(m, **{name: None}), "is NULL")
    for field in ("ref", "ref_len"):
        m2, keep2 = s.struct()
        setattr(m2, field, None)
        refused(s.call(m2), "is NULL")
    # misalignment
    refused(s.call(m, query=s.q.data_ptr() + 4), "not 16-byte aligned")
    refused(s.call(m, hit=s.a.hit.data_ptr() + 8), "not 16-byte aligned")
    refused(s.call(m, pairs=s.pr.data_ptr() + 8), "not 16-byte aligned")
    refused(s.call(m, rows=s.a.rows.data_ptr() + 8), "not 16-byte aligned")
    m2, keep2 = s.struct()
    m2.ref = m2.ref + 8
    refused(s.call(m2), "not 16-byte aligned")
    # the path struct
    for width in (0, 4, 12, 65544, 1 << 31):
        refused(s.call(m, path=path_struct(width)), "path is NULL or outside the rules")
    refused(s.call(m, path=path_struct(WIDTH, flags=1)), "outside the rules")
    refused(s.call(m, path=path_struct(WIDTH, reserved=1 << 40)), "outside the rules")
    # everything vbz_gpu_match is refused for
    for kw in ({"N": 0}, {"N": 60}, {"N": 65544}, {"quant": 0.0}, {"quant": float("nan")}, {"quant": float("inf")}, {"flags": 1}, {"reserved": 1}):
        refused(s.call(s.struct(**kw)[0]), "match outside the rules")
    for field, v in (("n_refs", 0), ("n_refs", 4097), ("ref_stride", 0), ("ref_stride", 24), ("ref_stride", 2064)):
        m2, keep2 = s.struct()
        setattr(m2, field, v)
        refused(s.call(m2), "match outside the rules")
    # extents: n_reads * N * 4 beyond 2^46 bytes (n_pairs * ref_stride * 8 stays below 2^46 for every n_pairs of 32 bits: the check is the
    # host's own arithmetic in 64 bits)
    m2, keep2 = s.struct(N=65536)
    refused(s.call(m2, n_reads=0xFFFFFFFF), "not plausible")
    torch.cuda.synchronize()
    assert s.a.untouched() and (s.q.cpu().numpy().view(np.uint32) == s.query.view(np.uint32)).all()
    # ... and the same arguments, unspoilt, run
    assert s.call(m)[0] == 0 and s.call(m, valid=None)[0] == 0
    s.c.synchronize()
    hit, rows = s.a.read()
    assert (hit[:, 0] != EMPTY[0]).all()
    # no pairs: queued, nothing written, NULL tables allowed
    s2 = Setup()
    assert s2.call(m, n_pairs=0, pairs=None, hit=None, rows=None, query=None)[0] == 0
    torch.cuda.synchronize()
    assert s2.a.untouched()
    assert s.c.L.vbz_gpu_match_path_batch(None, 0, 0, None, None, None, None, None, None, None) == -1


def test_best_refusals():
    c = codec()
    spans = torch.full((4, 3, 4), 7, dtype=torch.int32, device=c.device)
    out = torch.full((5, 4), HIT_CANARY, dtype=torch.int32, device=c.device)
    L = c.L
    for args in ((4, None, 3, 9, out.data_ptr()), (4, spans.data_ptr(), 3, 9, None), (4, spans.data_ptr() + 8, 3, 9, out.data_ptr()),
                 (4, spans.data_ptr(), 3, 9, out.data_ptr() + 4), (4, spans.data_ptr(), 0, 9, out.data_ptr()), (4, spans.data_ptr(), 4097, 9, out.data_ptr()),
                 (0xFFFFFFFF, spans.data_ptr(), 4096, 9, out.data_ptr())):
        assert L.vbz_gpu_match_best_batch(c.ctx, *args) == -2, args
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == HIT_CANARY).all()
    assert L.vbz_gpu_match_best_batch(c.ctx, 0, None, 3, 9, None) == 0 and L.vbz_gpu_match_best_batch(None, 0, None, 3, 9, None) == -1


def test_untrusted_pairs_get_the_empty_verdict():
    s = Setup()
    big = 0xFFFFFFFF
    good = [(0, 0, 3, 40), (1, 1, 0, 48), (2, 2, 30, 40), (2, 0, 0, 40), (1, 2, 63, 64)]
    bad = [(4, 0, 0, 8), (big, 0, 0, 8), (0, 3, 0, 8), (0, P.NONE, 0, 0), (0, 0, 8, 8), (0, 0, 9, 8), (0, 0, big, 8), (0, 0, 0, 65), (0, 0, 0, big), (2, 0, 0, 41),
           (3, 0, 0, 1), (0, 0, 0, 49), (0, 0, 15, 64), (0, 3, big, big), (big, big, big, big)]
    pairs = [p for g, b in zip(good, bad) for p in (g, b)] + bad[len(good) :]
    for ref_len, dead in (([20, 32, 7], ()), ([20, 0, 7], (1,)), ([33, 32, big], (0, 2))):   # M_r == 0, M_r > ref_stride
        want = P.paths(s.query, [N, N, 40, 0], 32.0, s.ref, ref_len, pairs, WIDTH)
        got = stage_path(s.c, s.query, [N, N, 40, 0], 32.0, s.ref, ref_len, pairs, WIDTH)
        assert_paths(got, want, pairs, ref_len)
        for p, pr in enumerate(pairs):
            empty = pr in bad or pr[1] in dead
            assert (got[0][p].tolist() == EMPTY) == empty, (p, pr, got[0][p].tolist())
            assert not empty or not got[1][p].any()
    # valid NULL: every row has N samples, read 3 and the tail of read 2 included
    pairs = [(3, 0, 0, 48), (2, 2, 30, 64), (2, 0, 0, 65)]
    got = stage_path(s.c, s.query, None, 32.0, s.ref, s.ref_len, pairs, WIDTH)
    assert_paths(got, P.paths(s.query, None, 32.0, s.ref, s.ref_len, pairs, WIDTH), pairs, "valid NULL")
    assert got[0][0][0] != EMPTY[0] and got[0][2].tolist() == EMPTY


@pytest.mark.parametrize("n_pairs", [0, 1, 3, 4, 5, 9])
def test_groups_under_a_small_cap(n_pairs):
    """a cap of four pairs' bits: calls of a group boundary - 1, + 0, + 1 pairs and of three groups write what one group writes"""
    words = 64 * ((63 + 8) * 1 // 16 + 1)   # match_path_groups.h: max_width 8, ref_stride 16 (one row a lane)
    small = codec(VBZ_HIP_MATCH_PATH_CAP=4 * words * 4)
    rng = np.random.default_rng(3)
    query = rng.integers(-3, 4, (5, 16)).astype(np.float32)
    ref = rng.integers(-3, 4, (2, 16)).astype(np.int8)
    ref_len = [5, 16]
    pairs = [(p % 5, p % 2, p % 7, p % 7 + 1 + p % 8) for p in range(n_pairs)]
    pairs = [pr if p != 2 else (9, 0, 0, 8) for p, pr in enumerate(pairs)]   # an empty verdict inside the first group
    want = P.paths(query, None, 1.0, ref, ref_len, pairs, 8)
    for c in (small, codec()):
        c.profile_reset()
        c.profile(True)
        got = stage_path(c, query, None, 1.0, ref, ref_len, pairs, 8)
        launches = c.profile_read().get("match_path_forward", (0, 0.0))[0]
        c.profile(False)
        assert_paths(got, want, pairs, ("cap", c is small))
        assert launches == ((n_pairs + 3) // 4 if c is small else min(n_pairs, 1)), ("groups", c is small, n_pairs, launches)
