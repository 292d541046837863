"""What vbz_gpu_squiggle_batch and vbz_gpu_levels_fit_batch refuse on the host (include/vbz_gpu.h): -2 with nothing launched and the
canary-filled arenas untouched, and the same arguments, unspoilt, run.  And every invalid-pair condition of the fit, one at a time: the
bad pair keeps the prior's constants with used = ok = 0, its neighbours are unharmed."""
import ctypes

import numpy as np
import pytest
import torch

import squiggle_ref as R
from squiggle_support import FitTables, SquiggleTables, assert_fit, assert_squiggle, stage_fit
from typed_support import codec
from vbz_compression_amd import _lib

pytestmark = pytest.mark.gpu


def refused(got, text):
    rc, msg = got
    assert rc == -2 and text in msg, (rc, msg, text)


def test_squiggle_refusals_launch_nothing():
    c = codec()
    call = [t for t in R.squiggle_cases() if t.name == "lower case and U"][0]
    s = SquiggleTables(c, call)
    refused(s.run(c, sq=None), "squiggle is NULL")
    for kw in ({"k": 0}, {"k": 10}, {"n_seqs": 0}, {"n_seqs": 2049}, {"n_seqs": 4097, "flags": 0}, {"seq_stride": 0}, {"seq_stride": 8}, {"seq_stride": 3000},
               {"seq_stride": (1 << 30) + 16}, {"target_stride": 0}, {"target_stride": 24}, {"target_stride": (1 << 30) + 16}, {"flags": 4}, {"flags": 0x80000001},
               {"quant": 0.0}, {"quant": -1.0}, {"quant": float("nan")}, {"quant": float("inf")}):
        refused(s.run(c, sq=s.struct(**kw)), "outside the rules")
    for name in ("seq", "seq_len", "model"):
        refused(s.run(c, sq=s.struct(**{name: None})), "is NULL")
    for name in ("target", "target_len", "masked"):
        refused(s.run(c, **{name: None}), "is NULL")
    refused(s.run(c, sq=s.struct(seq=s.seq.data_ptr() + 4)), "not 16-byte aligned")
    refused(s.run(c, target=s.target.ptr() + 8), "not 16-byte aligned")
    refused(s.run(c, level=s.level.ptr() + 4), "not 16-byte aligned")
    assert c.L.vbz_gpu_squiggle_batch(None, None, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert s.untouched()
    # ... and the same arguments, unspoilt, run
    assert s.run(c)[0] == 0
    c.synchronize()
    assert_squiggle(s.read(), call.expected(), call)


def test_levels_fit_refusals_launch_nothing():
    c = codec()
    call = R.fit_cases()[0]
    s = FitTables(c, call)
    refused(s.run(c, locate=None), "locate is NULL")
    for kw in ({"query_len": 0}, {"query_len": 12}, {"query_len": 2056}, {"n_targets": 0}, {"n_targets": 4097}, {"target_stride": 8}, {"target_stride": 360},
               {"target_stride": (1 << 30) + 16}, {"flags": 1}, {"reserved": 1}, {"quant": 0.0}, {"quant": float("nan")}, {"quant": float("inf")}):
        refused(s.run(c, locate=s.locate(**kw)), "locate outside the rules")
    refused(s.run(c, locate=s.locate(target=s.target.data_ptr() + 4)), "not 16-byte aligned")
    for name in ("target", "target_len"):
        refused(s.run(c, locate=s.locate(**{name: None})), "is NULL")
    refused(s.run(c, fit=None), "levels fit is NULL")
    refused(s.run(c, fit=_lib.GpuLevelsFit(call.W, 0, 0, 1)), "outside the rules")
    for w in (0, 4, 12, 65544, 1 << 31):
        refused(s.run(c, fit=_lib.GpuLevelsFit(w, 0, 0, 0)), "outside the rules")
    for name in ("pairs", "hit", "n_levels", "levels", "out", "offset", "scale"):
        refused(s.run(c, **{name: None}), "is NULL")
    for name, p in (("pairs", s.pairs.data_ptr()), ("hit", s.hit.data_ptr()), ("levels", s.levels.data_ptr()), ("out", s.out.ptr())):
        refused(s.run(c, **{name: p + 8}), "not 16-byte aligned")
    refused(s.run(c, n_pairs=0xFFFFFFFF, fit=_lib.GpuLevelsFit(65536, 0, 0, 0)), "not plausible")   # n_pairs * max_width * 32 beyond 2^46
    assert s.run(c, n_pairs=0, pairs=None, hit=None, n_levels=None, levels=None, out=None, offset=None, scale=None, sums=None, prior=None)[0] == 0
    refused(s.run(c, n_pairs=0, fit=_lib.GpuLevelsFit(12, 0, 0, 0)), "outside the rules")           # bad arguments stay refused
    assert c.L.vbz_gpu_levels_fit_batch(None, 0, 0, None, None, None, None, None, None, None, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert s.untouched()
    # ... and the same arguments, unspoilt, run
    assert s.run(c)[0] == 0
    c.synchronize()
    assert_fit(s.read(), call.expected(), call)


def test_every_invalid_pair_condition_alone():
    c = codec()
    for name, call, bad in R.invalid_pair_calls():
        got = stage_fit(c, call)
        want_out, want_sums = call.expected()
        assert_fit(got, (want_out, want_sums), call)
        out = got[0]
        assert out[bad][2:].tolist() == [0, 0] and out[0][2:].tolist() == [40, 1] and out[2][2:].tolist() == [40, 1], (name, out.tolist())
