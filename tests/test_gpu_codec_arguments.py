"""The arguments of GpuCodec's stage methods on the MI355X -- match, locate, match_best, match_path, locate_path, query_valid, events_query,
locate_levels, squiggle, levels_fit and range_samples -- over the smallest tables (2 reads, query_len 8, 2 references or targets of stride
16, max_width 8, k 1): (a) every caller-given output comes back as the same object and holds what the call that allocates its own
returns; (b) a wrong dtype, a non-contiguous tensor and a wrong shape, of one input and of one output per method, raise AssertionError
with nothing queued -- the canary-filled output arenas are untouched after a synchronisation; (c) match_path runs without valid and
locate_path refuses that, and their rows are [p, ref_stride, 2] and [p, query_len, 2].  The library is compared with itself at two call
shapes: what the calls compute is the other GPU tests' subject."""
import functools

import numpy as np
import pytest
import torch

from eventalign_support import GUARD, Guarded
from typed_support import codec, i32
from vbz_compression_amd import batch

pytestmark = pytest.mark.gpu

READS, N, STRIDE, W, K = 2, 8, 16, 8, 1
THREE_STATE = ("index", "level", "sums")   # True allocates, False leaves out, a tensor is taken


class Spec:
    """one method: its tensor arguments by name, its other arguments, the outputs it takes (in the order it returns them), and which
    input and output the refusals are tried on (shape_in: the input with a shape rule, where bad_in has none)"""

    def __init__(self, args, fixed, outs, bad_in, bad_out=None, shape_in=None):
        self.args, self.fixed, self.outs, self.bad_in, self.bad_out, self.shape_in = args, fixed, outs, bad_in, bad_out, shape_in or bad_in


def run(c, name, spec, **over):
    got = getattr(c, name)(**{**spec.args, **spec.fixed, **over})
    return got if isinstance(got, tuple) else (got,)


@functools.lru_cache(maxsize=None)
def specs():
    """the chain of calls once: every method's arguments are what the one before it left"""
    c = codec()
    dev = c.device
    rng = np.random.default_rng(20261021)

    # match: the references are stretches of the reads' own levels
    q_levels = rng.integers(-100, 100, (READS, N)).astype(np.int8)
    query = torch.from_numpy((q_levels / 32.0).astype(np.float32)).to(dev)
    valid = i32([N, N - 2]).to(dev)
    ref = np.zeros((2, STRIDE), np.int8)
    ref[0, :4], ref[1, :5] = q_levels[0, 2:6], q_levels[1, 0:5]
    ref, ref_len = torch.from_numpy(ref).to(dev), i32([4, 5]).to(dev)
    m_spans = c.match_span(query, valid, ref, ref_len)
    m_pairs = c.match_best(m_spans)

    # squiggle -> the targets of the locate family
    seq = torch.from_numpy(rng.choice(np.frombuffer(b"ACGT", np.uint8), (2, STRIDE))).to(dev)
    seq_len = i32([STRIDE, STRIDE - 4]).to(dev)
    model = torch.tensor([-2.5, -0.75, 0.5, 2.25], dtype=torch.float32, device=dev)
    sq = Spec(dict(seq=seq, seq_len=seq_len, model=model), dict(k=K, target_stride=STRIDE), ["target", "target_len", "masked", "level"], "seq_len", "target")
    target, target_len, _, _ = run(c, "squiggle", sq)
    t_host = target.cpu().numpy()

    # events whose means are stretches of the targets: 9 and 8 rows, one of read 0 too short to count
    first = torch.tensor([0, 9, 17], dtype=torch.int64, device=dev)
    n = np.array([3, 2, 0, 4, 2, 5, 3, 2, 6] + [2, 3, 4, 2, 5, 3, 2, 4], np.uint32)
    mean = np.concatenate([np.insert(t_host[0, 3:11] / 32.0, 2, 9.0), t_host[1, 1:9] / 32.0]).astype(np.float32)
    rec = np.zeros((17, 4), np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2] = mean.view(np.uint32), 0x3F800000, n
    records = i32(rec.reshape(-1)).to(dev).reshape(17, 4)
    start = i32(np.concatenate([np.cumsum(n[:9]) - n[:9], np.cumsum(n[9:]) - n[9:]])).to(dev)
    mom = np.stack([np.rint(mean * n * 64), np.rint(mean * mean * n * 4096)], 1).astype(np.int64)
    moments = torch.from_numpy(mom).to(dev)
    verdict = i32([4 * 27, 4 * 25]).to(dev)
    ev = Spec(dict(event_first=first, records=records, result=verdict), dict(query_len=N, min_n=1), ["query", "valid", "index"], "records", "index")
    e_query, e_valid, e_index = run(c, "events_query", ev, index=True)
    l_spans = c.locate_span(e_query, e_valid, target, target_len)
    l_pairs = c.match_best(l_spans)
    lp = Spec(dict(query=e_query, valid=e_valid, target=target, target_len=target_len, pairs=l_pairs), dict(max_width=W), ["hit", "rows"], "valid", "rows")
    hit, rows = run(c, "locate_path", lp)
    ll = Spec(dict(pairs=l_pairs, hit=hit, rows=rows, event_first=first, start=start, records=records, moments=moments, index=e_index),
              dict(max_width=W), ["n_levels", "levels"], "hit", "levels")
    n_levels, lv = run(c, "locate_levels", ll)
    prior = torch.tensor([[0.25, 1.5], [-0.5, 0.75]], dtype=torch.float32, device=dev)
    begin, end = i32([1, 0]).to(dev), i32([20, 1 << 31]).to(dev)
    c.synchronize()
    return {
        "match": Spec(dict(query=query, valid=valid, ref=ref, ref_len=ref_len), {}, ["out"], "valid", "out"),
        "locate": Spec(dict(query=e_query, valid=e_valid, target=target, target_len=target_len), {}, ["out"], "valid", "out"),
        "match_best": Spec(dict(spans=m_spans), dict(max_cost=1000), ["out"], "spans", "out"),
        "match_path": Spec(dict(query=query, valid=valid, ref=ref, ref_len=ref_len, pairs=m_pairs), dict(max_width=W), ["hit", "rows"], "pairs", "rows"),
        "locate_path": lp,
        "query_valid": Spec(dict(result=verdict, begin=begin, end=end), dict(query_len=N), ["out"], "result", "out", shape_in="begin"),
        "events_query": ev,
        "locate_levels": ll,
        "squiggle": sq,
        "levels_fit": Spec(dict(pairs=l_pairs, hit=hit, n_levels=n_levels, levels=lv, target=target, target_len=target_len, prior=prior),
                           dict(n_reads=READS, locate=batch.Locate(query_len=N), min_samples=1), ["out", "offset", "scale", "sums"], "n_levels", "offset"),
        "range_samples": Spec(dict(samples=i32([27, 25]).to(dev), begin=begin, end=end), {}, [], "samples", shape_in="begin"),
    }


METHODS = ["match", "locate", "match_best", "match_path", "locate_path", "query_valid", "events_query", "locate_levels", "squiggle", "levels_fit",
           "range_samples"]


class Given:
    """a caller's output of `like`'s shape and dtype: a view of a canary-filled arena between two guards"""

    def __init__(self, c, like):
        nbytes = like.numel() * like.element_size()
        assert nbytes and nbytes % 4 == 0, (like.shape, like.dtype)
        self.g = Guarded(c, nbytes // 4)
        self.t = self.g.t[GUARD:GUARD + self.g.words].view(like.dtype).view(like.shape)


def own(c, name, spec):
    """the call that allocates its own outputs"""
    return run(c, name, spec, **{k: True for k in spec.outs if k in THREE_STATE})


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def bad_forms(t):
    """(what, tensor) of the three refusals of a good tensor t: another dtype of the same width, the same values at stride 2, one entry short"""
    other = {torch.int32: torch.float32, torch.float32: torch.int32, torch.int64: torch.float64, torch.int8: torch.uint8, torch.uint8: torch.int8}[t.dtype]
    strided = t.repeat_interleave(2, dim=-1)[..., ::2]
    assert strided.shape == t.shape and not strided.is_contiguous()
    return [("dtype", t.view(other)), ("non-contiguous", strided), ("shape", t.reshape(-1)[:-1].contiguous())]


@pytest.mark.parametrize("name", METHODS)
def test_given_outputs_come_back_and_hold_the_same(name):
    c, spec = codec(), specs()[name]
    want = own(c, name, spec)
    assert len(want) == max(len(spec.outs), 1) and all(isinstance(t, torch.Tensor) for t in want), name
    given = {k: Given(c, w) for k, w in zip(spec.outs, want)}
    back = run(c, name, spec, **{k: g.t for k, g in given.items()})
    c.synchronize()
    for k, w, b in zip(spec.outs, want, back):
        assert b is given[k].t, (name, k)
        given[k].g.read(k)   # (the guards around it)
        assert same_bits(w, b), (name, k, w.cpu().tolist(), b.cpu().tolist())
    if not spec.outs:   # (range_samples takes no output: two calls give the same table)
        assert same_bits(want[0], back[0]), (name, want[0].tolist(), back[0].tolist())
    for k in spec.outs:
        if k in THREE_STATE:
            assert run(c, name, spec, **{k: False})[spec.outs.index(k)] is None, (name, k)


@pytest.mark.parametrize("name", METHODS)
def test_bad_tensors_are_refused_before_anything_is_queued(name):
    c, spec = codec(), specs()[name]
    like = dict(zip(spec.outs, own(c, name, spec)))
    tried = [(spec.shape_in if what == "shape" else spec.bad_in, what) for what in ("dtype", "non-contiguous", "shape")]
    tried += [(spec.bad_out, what) for what in ("dtype", "non-contiguous", "shape")] if spec.bad_out else []
    for k, what in tried:
        given = {o: Given(c, w) for o, w in like.items()}
        good = spec.args[k] if k in spec.args else given[k].t
        bad = dict(bad_forms(good))[what]
        before = bad.clone()
        torch.cuda.synchronize()
        with pytest.raises(AssertionError):
            run(c, name, spec, **{**{o: g.t for o, g in given.items()}, k: bad})
        torch.cuda.synchronize()
        assert all(g.g.untouched() for g in given.values()), (name, k, what)
        assert same_bits(before.contiguous(), bad.contiguous()), (name, k, what)


def test_the_two_path_calls_differ_in_valid_and_rows():
    c, s = codec(), specs()
    mp, lp = s["match_path"], s["locate_path"]
    hit, rows = run(c, "match_path", mp, valid=None)
    c.synchronize()
    p = int(mp.args["pairs"].shape[0])
    assert tuple(hit.shape) == (p, 4) and tuple(rows.shape) == (p, STRIDE, 2), (hit.shape, rows.shape)
    given = {o: Given(c, w) for o, w in zip(lp.outs, run(c, "locate_path", lp))}
    assert tuple(given["hit"].t.shape) == (p, 4) and tuple(given["rows"].t.shape) == (p, N, 2), (given["hit"].t.shape, given["rows"].t.shape)
    torch.cuda.synchronize()
    with pytest.raises((AssertionError, AttributeError)):   # (valid is required: None has no dtype to state)
        run(c, "locate_path", lp, valid=None, **{o: g.t for o, g in given.items()})
    torch.cuda.synchronize()
    assert all(g.g.untouched() for g in given.values())
