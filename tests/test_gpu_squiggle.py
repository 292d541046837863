"""vbz_gpu_squiggle_batch on the MI355X, bit for bit against tests/squiggle_ref.py over its catalogue -- every k, L on each side of every
seam of the kernel's cut, the four flag combinations, invalid bases at the seams, refused lengths, special values in the model, with and
without the level arena, 70 000 bases at k = 9 -- canary words around every arena; GpuCodec.squiggle into given tensors; and the tie to the
locate kernels' own quantiser: a window of a level row as the query of vbz_gpu_locate_span_batch is found in the target row of the same
call at cost 0, exactly where it was cut."""
import numpy as np
import pytest
import torch

import squiggle_ref as R
from squiggle_support import assert_squiggle, stage_squiggle
from typed_support import codec, i32, u32
from vbz_compression_amd import batch

pytestmark = pytest.mark.gpu


def test_catalogue_bit_for_bit():
    c = codec()
    for call in R.squiggle_cases():
        assert_squiggle(stage_squiggle(c, call), call.expected(), call)


def test_a_palindrome_gives_two_equal_rows():
    c = codec()
    call = [t for t in R.squiggle_cases() if t.name.startswith("a palindrome")][0]
    target, target_len, masked, level = stage_squiggle(c, call)
    assert target_len.tolist() == [1396, 1396] and (target[0] == target[1]).all() and (level[0] == level[1]).all() and target[0].any()


def test_codec_method_into_given_tensors():
    c = codec()
    call = [t for t in R.squiggle_cases() if t.name == "lower case and U"][0]
    dev = c.device
    seq, seq_len = torch.from_numpy(call.seq).to(dev), i32(call.seq_len).to(dev)
    model = torch.from_numpy(call.model.view(np.float32).copy()).to(dev)
    want = call.expected()
    target, target_len, masked, level = c.squiggle(seq, seq_len, model, call.k, call.target_stride, quant=call.quant, both=True, level=True)
    given = (torch.full_like(target, 7), torch.full_like(target_len, 7), torch.full_like(masked, 7), torch.full_like(level, 7.0))
    back = c.squiggle(seq, seq_len, model, call.k, call.target_stride, quant=call.quant, both=True, level=given[3], target=given[0], target_len=given[1],
                      masked=given[2])
    none = c.squiggle(seq, seq_len, model, call.k, call.target_stride, quant=call.quant, both=True)
    c.synchronize()
    assert all(a is b for a, b in zip(back, given)) and none[3] is None
    for t, tl, mk, lv in ((target, target_len, masked, level), given, none):
        assert (t.cpu().numpy() == want[0]).all() and (u32(tl) == want[1]).all() and (u32(mk) == want[2]).all()
        assert lv is None or (lv.cpu().numpy().view(np.uint32) == want[3]).all()


def rc_index(index, k):
    """the table entry of a k-mer's reverse complement"""
    out = 0
    for _ in range(k):
        out, index = out * 4 + 3 - index % 4, index // 4
    return out


def distinct_neighbours(rng, model, n, k):
    """a sequence whose consecutive k-mers have different quantised levels on both strands: a cost-0 path through it has diagonal steps alone"""
    q = R.quantise(model.view(np.uint32), 32.0).astype(np.int64)
    codes = [int(x) for x in rng.integers(0, 4, k)]
    index = sum(x * 4 ** (k - 1 - i) for i, x in enumerate(codes))
    while len(codes) < n:
        for b in rng.permutation(4):
            nxt = (index * 4 + int(b)) % 4 ** k
            if q[nxt] != q[index] and q[rc_index(nxt, k)] != q[rc_index(index, k)]:
                codes.append(int(b))
                index = nxt
                break
        else:
            raise AssertionError("no base gives another level on both strands")
    return bytes(b"ACGT"[x] for x in codes)


def test_levels_as_a_query_are_found_where_they_were_cut():
    c = codec()
    dev = c.device
    rng = np.random.default_rng(2505)
    k, n, N = 5, 5000, 2048
    model = (rng.permutation(1024) % 201 - 100).astype(np.float32) / np.float32(32)
    text = distinct_neighbours(rng, model, n, k)
    call = R.SquiggleCall("distinct neighbours", k, [text], model, R.BOTH)
    want_target, want_len, _, want_level = call.expected()
    windows = []   # (row, first level, width): stretches whose neighbours differ on that row, so that the stretch is unique
    for row in (0, 1):
        same = np.flatnonzero(want_target[row, 1:want_len[row]] == want_target[row, :want_len[row] - 1])
        for width in (8, 100, 777, 2048):
            for first in rng.integers(0, int(want_len[row]) - width, 40):
                if not ((same >= first) & (same < first + width - 1)).any():
                    windows.append((row, int(first), width))
                    break
    assert len(windows) == 8, windows
    target, target_len, masked, level = c.squiggle(torch.from_numpy(call.seq).to(dev), i32(call.seq_len).to(dev), torch.from_numpy(model).to(dev), k,
                                                   call.target_stride, both=True, level=True)
    query = torch.zeros((len(windows), N), dtype=torch.float32, device=dev)
    for i, (row, first, width) in enumerate(windows):
        query[i, :width] = level[row, first:first + width]
    valid = i32([w for _, _, w in windows]).to(dev)
    spans = c.locate_span(query, valid, target, target_len, batch.Locate(query_len=N, quant=32.0))
    c.synchronize()
    assert (target.cpu().numpy() == want_target).all() and (level.cpu().numpy().view(np.uint32) == want_level).all()
    got = spans.cpu().numpy().view(np.uint32)
    for i, (row, first, width) in enumerate(windows):
        assert got[i, row].tolist() == [0, first + width, first, 0], (i, windows[i], got[i].tolist())
