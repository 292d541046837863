"""Eventalign on the device: encoded reads -> segment -> events (records and moments) -> events_query -> locate_span -> match_best ->
locate_path -> locate_levels, queued on one stream with no host copy between the calls, over a dozen short step-signal reads cut from two
planted targets -- one read failing, one with fewer events than N -- and the same chain over POD5 reads of two rows.  Every table is held
to the numpy statement of its call: segment_ref, events_ref, eventalign_ref, locate_span_ref, match_path_ref.best, locate_path_ref,
eventalign_ref."""
import numpy as np
import pytest
import torch

import eventalign_ref as E
import events_ref as EV
import locate_path_ref as LP
import locate_span_ref as LS
import match_path_ref as MP
import pod5_ref as PD
import segment_ref as S
from typed_support import Frames, arena, codec, i32, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

N, W, QUANT, MIN_N, L, STRIDE = 256, 512, 32.0, 5, 600, 608
SCALE = 1.0 / 256.0   # a level g of a target is 8 g counts of signal: mean * QUANT = counts / 8
FAILING, SHORT = 5, 8


def planted(seed):
    """(targets int8 [2, STRIDE], the reads' signals, (target, first level, levels) per read)"""
    rng = np.random.default_rng(seed)
    target = np.zeros((2, STRIDE), np.int8)
    for g in range(2):
        v = [int(rng.integers(-100, 101))]
        while len(v) < L:   # neighbours at least 20 levels apart: every step is a boundary under noise of 4 counts
            nxt = int(rng.integers(-100, 101))
            if abs(nxt - v[-1]) >= 20:
                v.append(nxt)
        target[g, :L] = v
    reads, plan = [], []
    for i in range(12):
        g, m = i % 2, (40 if i == SHORT else int(rng.integers(270, 330)))
        a = int(rng.integers(0, L - m))
        dwell = rng.integers(6, 15, m)
        dwell[7::25] = 16
        x = np.repeat(target[g, a:a + m].astype(np.float64) * 8, dwell)
        for q in (np.cumsum(dwell) - dwell)[7::25]:   # a spike of three samples inside a long dwell: an event below MIN_N, the level in two events
            x[q + 6:q + 9] += 300
        x += rng.normal(0, 4, len(x))
        reads.append(np.clip(np.rint(x), -32768, 32767).astype(np.int16))
        plan.append((g, a, m))
    return target, reads, plan


def run_chain(c, target, segment, events, cap, verdict):
    """the calls behind the decode-specific two, one synchronisation at the end -> every table as numpy"""
    dev = c.device
    tg, tl = torch.from_numpy(target).to(dev), i32([L, L]).to(dev)
    loc = batch.Locate(query_len=N, quant=QUANT)
    first, start = segment(torch.empty(cap, dtype=torch.int32, device=dev))
    rec = torch.zeros((int(start.numel()), 4), dtype=torch.int32, device=dev)
    mom = torch.zeros((int(start.numel()), 2), dtype=torch.int64, device=dev)
    events(first, start, rec, mom)
    query, valid, index = c.events_query(first, rec, N, min_n=MIN_N, result=verdict())
    spans = c.locate_span(query, valid, tg, tl, loc)
    pairs = c.match_best(spans)
    hit, rows = c.locate_path(query, valid, tg, tl, pairs, W, loc)
    n_levels, levels = c.locate_levels(pairs, hit, rows, first, start, rec, mom, W, index=index)
    c.synchronize()
    return {"first": first.cpu().numpy(), "start": u32(start).astype(np.uint32), "rec": rec.cpu().numpy().view(np.uint32), "mom": mom.cpu().numpy().view(np.uint64),
            "query": query.cpu().numpy(), "valid": u32(valid), "index": index.cpu().numpy().view(np.uint32), "spans": spans.cpu().numpy().view(np.uint32),
            "pairs": pairs.cpu().numpy().view(np.uint32), "hit": hit.cpu().numpy().view(np.uint32), "rows": rows.cpu().numpy().view(np.uint32),
            "n_levels": n_levels.cpu().numpy().view(np.uint32), "levels": levels.cpu().numpy().view(np.uint32), "verdict": u32(verdict())}


def check_chain(d, target, signals, plan, failed):
    n = len(signals)
    # segment and events
    st = [np.zeros(0, np.uint32) if i in failed else S.starts(x) for i, x in enumerate(signals)]
    want_first = np.concatenate([[0], np.cumsum([len(v) for v in st])]).astype(np.int64)
    total, cap = int(want_first[-1]), len(d["start"])
    assert d["first"].tolist() == want_first.tolist() and total > 2000
    assert d["start"][:total].tolist() == np.concatenate(st).tolist()
    want = [EV.event_rows(x, None, None, st[i].tolist(), 0.0, SCALE) for i, x in enumerate(signals)]
    rec, mom = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want]).view(np.uint64)
    assert (d["rec"][:total] == rec).all() and (d["mom"][:total] == mom).all()
    assert all(_lib.is_error(int(d["verdict"][i])) == (i in failed) for i in range(n))
    # the query
    query, valid, index = E.events_query(want_first.astype(np.uint64), cap, d["rec"][:, 0], d["rec"][:, 2], N, MIN_N, d["verdict"])
    assert (d["query"].view(np.uint32) == query).all() and (d["valid"] == valid).all() and (d["index"] == index).all()
    assert valid[FAILING] == 0 and 0 < valid[SHORT] < N and sum(int(v) == N for v in valid) >= 8, valid.tolist()
    assert any((index[i, :valid[i]] != np.arange(valid[i])).any() for i in range(n)), "no event was dropped"
    # span, best, path
    tl = [L, L]
    spans = LS.spans(d["query"], valid, QUANT, target, tl)
    assert (d["spans"] == spans).all()
    pairs = MP.best(spans)
    assert (d["pairs"] == pairs).all()
    hit, rows = LP.paths(d["query"], valid, QUANT, target, tl, pairs, W)
    assert (d["hit"] == hit).all() and (d["rows"] == rows).all()
    # the levels
    n_levels, levels = E.levels(pairs, hit, rows, index, want_first.astype(np.uint64), cap, d["start"], d["rec"][:, 2], d["mom"], n, N, W)
    assert (d["n_levels"] == n_levels).all() and (d["levels"] == levels).all()
    for i, (g, a, m) in enumerate(plan):   # the chain found what was planted
        if i in failed:
            assert pairs[i].tolist() == [i, LP.NONE, 0, 0] and n_levels[i] == 0 and not levels[i].any()
            continue
        assert pairs[i][1] == g and a - 3 <= hit[i][2] <= a + 3 and n_levels[i] == hit[i][1] - hit[i][2] > 0.9 * min(m, N) - 3, (i, plan[i], hit[i].tolist())
        lv = levels[i, :n_levels[i]]
        assert (lv[:, 3] >= 1).all() and (lv[1:, 0] >= lv[:-1, 0]).all() and lv[-1, 1] <= len(signals[i])
        mean = lv[:, 4:6].copy().view(np.int64)[:, 0] / np.maximum(lv[:, 2], 1) / 8.0     # the level's mean in target units, from its exact moments
        close = np.abs(mean - target[g, hit[i][2]:hit[i][1]]) < 3
        assert close.mean() > 0.9, (i, float(close.mean()))


def test_chain_over_encoded_reads():
    c = codec()
    target, reads, plan = planted(61)
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    size = fr.size.clone()
    size[FAILING] = int(u32(fr.size)[FAILING]) // 2   # the frame of one read cut off in its middle
    res = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    scale, offset = torch.full((fr.n,), SCALE, dtype=torch.float32, device=c.device), torch.zeros(fr.n, dtype=torch.float32, device=c.device)

    def segment(start):
        return c.signal_segment(fr.src, fr.off, size, fr.doff, fr.dcap, res, fr.opts, start=start)

    def events(first, start, rec, mom):
        c.signal_events(fr.src, fr.off, size, fr.doff, fr.dcap, res, fr.opts, first, start, scale=scale, offset=offset, moments=mom, arena=rec)

    d = run_chain(c, target, segment, events, sum(S.max_rows(len(x), 2) for x in reads), lambda: res)
    check_chain(d, target, reads, plan, {FAILING})


def test_chain_over_pod5_reads_of_two_rows():
    c = codec()
    dev = c.device
    target, reads, plan = planted(62)
    rng = np.random.default_rng(63)
    rows, first_row = [], []
    for x in reads:
        cut = int(rng.integers(1, len(x) - 1))
        first_row.append(len(rows))
        rows += [x[:cut], x[cut:]]
    frames = [PD.compress_row(x) for x in rows]
    frames[2 * FAILING + 1] = frames[2 * FAILING + 1][: len(frames[2 * FAILING + 1]) // 2]   # the second row of one read cut off
    src, off, size = arena(c, frames, 16)
    row_samples = i32([len(x) for x in rows]).to(dev)
    res = torch.full((len(rows),), -8, dtype=torch.int32, device=dev)
    rr = torch.full((len(reads),), -8, dtype=torch.int32, device=dev)
    scale, offset = torch.full((len(reads),), SCALE, dtype=torch.float32, device=dev), torch.zeros(len(reads), dtype=torch.float32, device=dev)

    def segment(start):
        return c.pod5_signal_segment(src, off, size, row_samples, first_row, res, start=start, read_result=rr)[:2]

    def events(first, start, rec, mom):
        c.pod5_signal_events(src, off, size, row_samples, first_row, res, first, start, scale=scale, offset=offset, moments=mom, arena=rec, read_result=rr)

    d = run_chain(c, target, segment, events, sum(S.max_rows(len(x), 2) for x in reads), lambda: rr)
    check_chain(d, target, reads, plan, {FAILING})
