"""The refit chain on the device: squiggle(BOTH) -> segment -> events -> events_query -> locate_span -> match_best -> locate_path ->
locate_levels -> levels_fit -> the events call again with the fitted tables as its per-read offset and scale -> events_query ->
locate_span -> match_best, all queued on one stream and synchronised once at the end, over tests/refit_chain.py's planted reads.  Every
table is held to its call's numpy statement bit for bit; test_squiggle_ref asserts that those statements find the planted strand and
stretch in both rounds with no read's cost rising, and the same conditions are asserted here on the device's tables."""
import numpy as np
import pytest
import torch

import refit_chain as RC
from typed_support import Frames, codec, i32, u32
from vbz_compression_amd import batch

pytestmark = pytest.mark.gpu


def test_two_rounds_on_one_stream():
    c = codec()
    dev = c.device
    seq, model, signals, plan = RC.planted()
    want = RC.numpy_chain()
    fr = Frames(c, signals, c.options(True, 2, 1, 1))
    res = torch.full((fr.n,), -8, dtype=torch.int32, device=dev)
    cap = want["cap"]
    loc = batch.Locate(query_len=RC.N, quant=RC.QUANT)

    def round_of(first, start, offset, scale):
        rec = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        mom = torch.zeros((cap, 2), dtype=torch.int64, device=dev)
        c.signal_events(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, first, start, scale=scale, offset=offset, moments=mom, arena=rec)
        query, valid, index = c.events_query(first, rec, RC.N, min_n=RC.MIN_N)
        spans = c.locate_span(query, valid, target, target_len, loc)
        return {"rec": rec, "mom": mom, "query": query, "valid": valid, "index": index, "spans": spans, "pairs": c.match_best(spans)}

    target, target_len, masked, _ = c.squiggle(torch.from_numpy(seq).to(dev), i32([RC.BASES]).to(dev), torch.from_numpy(model).to(dev), RC.K, RC.STRIDE,
                                               quant=RC.QUANT, both=True)
    first, start = c.signal_segment(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, start=torch.empty(cap, dtype=torch.int32, device=dev))
    one = round_of(first, start, torch.full((fr.n,), RC.OFFSET0, dtype=torch.float32, device=dev), torch.full((fr.n,), RC.SCALE0, dtype=torch.float32, device=dev))
    hit, rows = c.locate_path(one["query"], one["valid"], target, target_len, one["pairs"], RC.W, loc)
    n_levels, levels = c.locate_levels(one["pairs"], hit, rows, first, start, one["rec"], one["mom"], RC.W, index=one["index"])
    fit, offset, scale, sums = c.levels_fit(one["pairs"], hit, n_levels, levels, target, target_len, fr.n, loc, min_samples=RC.MIN_N, sums=True)
    two = round_of(first, start, offset, scale)
    c.synchronize()   # the one synchronisation

    raw = lambda t: t.cpu().numpy().view(np.uint64 if t.dtype == torch.int64 else np.uint32)   # noqa: E731
    assert (target.cpu().numpy() == want["target"]).all() and (u32(target_len) == want["target_len"]).all() and (u32(masked) == want["masked"]).all()
    assert first.cpu().numpy().tolist() == want["first"].tolist()
    total = int(want["first"][-1])
    assert (u32(start)[:total] == want["start"][:total]).all()
    got = {"target_len": want["target_len"], "masked": want["masked"]}
    for name, dev_round in (("one", one), ("two", two)):
        got[name] = {}
        for key in ("rec", "mom", "query", "valid", "index", "spans", "pairs"):
            g = raw(dev_round[key])
            w = want[name][key]
            if key in ("rec", "mom"):
                g, w = g[:total], w[:total]
            assert g.shape == w.shape and (g == w).all(), (name, key, np.argwhere(g != w)[:4].tolist())
            got[name][key] = g
    for key, t in (("hit", hit), ("rows", rows), ("n_levels", n_levels), ("levels", levels), ("fit", fit)):
        g = raw(t)
        assert g.shape == want[key].shape and (g == want[key]).all(), (key, np.argwhere(g != want[key])[:4].tolist())
    assert (sums.cpu().numpy() == want["sums"]).all()
    assert (raw(fit)[:, 0] == offset.cpu().numpy().view(np.uint32)).all() and (raw(fit)[:, 1] == scale.cpu().numpy().view(np.uint32)).all()
    got["fit"] = raw(fit)
    RC.assert_conditions(got)   # the stated conditions, on the device's own tables
