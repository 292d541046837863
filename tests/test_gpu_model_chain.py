"""The model chain on the device: squiggle(prior, BOTH) and squiggle_kmers -> segment -> events -> events_query -> locate_span -> match_best ->
locate_path -> locate_levels -> levels_fit -> levels_pile -> pile_kmers -> model_update -> squiggle(new model) -> the events call again with
the fitted tables -> events_query -> locate_span -> match_best, all queued on one stream and synchronised once at the end, over
tests/model_chain.py's planted reads.  Every table is held to its call's numpy statement bit for bit; test_pile_ref asserts that those
statements recover the moved k-mers and halve the summed cost with no read's cost rising, and the same conditions are asserted here on the
device's tables."""
import numpy as np
import pytest
import torch

import model_chain as MC
from typed_support import Frames, codec, i32, u32
from vbz_compression_amd import batch

pytestmark = pytest.mark.gpu


def test_two_rounds_and_a_model_update_on_one_stream():
    c = codec()
    dev = c.device
    seq, true, prior, moved, signals, plan = MC.planted()
    want = MC.numpy_chain()
    fr = Frames(c, signals, c.options(True, 2, 1, 1))
    res = torch.full((fr.n,), -8, dtype=torch.int32, device=dev)
    cap = want["cap"]
    loc = batch.Locate(query_len=MC.N, quant=MC.QUANT)
    seq_d, len_d, prior_d = torch.from_numpy(seq).to(dev), i32([MC.BASES]).to(dev), torch.from_numpy(prior).to(dev)

    def round_of(first, start, offset, scale, target, target_len):
        rec = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        mom = torch.zeros((cap, 2), dtype=torch.int64, device=dev)
        c.signal_events(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, first, start, scale=scale, offset=offset, moments=mom, arena=rec)
        query, valid, index = c.events_query(first, rec, MC.N, min_n=MC.MIN_N)
        spans = c.locate_span(query, valid, target, target_len, loc)
        return {"rec": rec, "mom": mom, "query": query, "valid": valid, "index": index, "spans": spans, "pairs": c.match_best(spans)}

    target, target_len, masked, _ = c.squiggle(seq_d, len_d, prior_d, MC.K, MC.STRIDE, quant=MC.QUANT, both=True)
    kmer, kmer_len = c.squiggle_kmers(seq_d, len_d, MC.K, MC.STRIDE, both=True)
    first, start = c.signal_segment(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, start=torch.empty(cap, dtype=torch.int32, device=dev))
    one = round_of(first, start, torch.full((fr.n,), MC.OFFSET0, dtype=torch.float32, device=dev), torch.full((fr.n,), MC.SCALE0, dtype=torch.float32, device=dev),
                   target, target_len)
    hit, rows = c.locate_path(one["query"], one["valid"], target, target_len, one["pairs"], MC.W, loc)
    n_levels, levels = c.locate_levels(one["pairs"], hit, rows, first, start, one["rec"], one["mom"], MC.W, index=one["index"])
    fit, offset, scale, _ = c.levels_fit(one["pairs"], hit, n_levels, levels, target, target_len, fr.n, loc, min_samples=MC.MIN_N)
    pile = c.levels_pile(one["pairs"], hit, n_levels, levels, target, target_len, fr.n, fix=MC.FIX, fit=fit, require_ok=True, locate=loc, min_samples=MC.MIN_N)
    kmer_pile = c.pile_kmers(pile, kmer, kmer_len, MC.K)
    model, sd = c.model_update(kmer_pile, prior_d, MC.K, fix=MC.FIX, min_obs=MC.MIN_OBS, sd=True)
    target2, target2_len, masked2, _ = c.squiggle(seq_d, len_d, model, MC.K, MC.STRIDE, quant=MC.QUANT, both=True)
    two = round_of(first, start, offset, scale, target2, target2_len)
    c.synchronize()   # the one synchronisation

    raw = lambda t: t.cpu().numpy().view(np.uint64 if t.dtype == torch.int64 else np.uint32)   # noqa: E731
    assert (target.cpu().numpy() == want["target"]).all() and (u32(target_len) == want["target_len"]).all() and (u32(masked) == want["masked"]).all()
    assert (raw(kmer) == want["kmer"]).all() and (u32(kmer_len) == want["kmer_len"]).all()
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
    for key, t in (("pile", pile), ("kmer_pile", kmer_pile), ("model", model), ("sd", sd)):
        g = raw(t).reshape(want[key].shape)
        assert (g == want[key]).all(), (key, np.argwhere(g != want[key])[:4].tolist())
        got[key] = g
    assert (target2.cpu().numpy() == want["target2"]).all() and (u32(target2_len) == want["target_len"]).all() and (u32(masked2) == want["masked"]).all()
    MC.assert_conditions(got)   # the stated conditions, on the device's own tables
