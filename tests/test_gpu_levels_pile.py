"""vbz_gpu_levels_pile_batch on the MI355X, bit for bit against tests/pile_ref.py over level arenas built in numpy: widths 1, 63, 64, 65, 129
and max_width, start at every residue of 4, depth 1, 2, 64 and 300 on one stretch, staggered overlaps, G = 1 and 3, both signs of sum, u at
+-2^24 and beyond, every skip condition alone and counted in the count word's high half, fit NULL and given, REQUIRE_OK, CLEAR and adding over
a dirty arena -- canary words around every arena; every invalid-pair condition alone touches nothing; two calls without CLEAR equal one over
the concatenated pairs; a level arena that locate_levels itself wrote; and GpuCodec.levels_pile."""
import numpy as np
import pytest
import torch

import eventalign_ref as E
import pile_ref as P
from eventalign_support import stage_levels
from pile_support import GuardedPile, assert_pile, stage_pile
from typed_support import codec, i32

pytestmark = pytest.mark.gpu


def test_catalogue_bit_for_bit():
    c = codec()
    for call in P.pile_cases():
        assert_pile(stage_pile(c, call), call.expected(), call.name)


def test_skips_are_counted_in_the_high_half():
    c = codec()
    for call in [t for t in P.pile_cases() if t.name.startswith("skip")]:
        got = stage_pile(c, call)
        cells = slice(11, 11 + 130)
        kept, skipped = got[0, cells] & np.uint64(0xFFFFFFFF), got[0, cells] >> np.uint64(32)
        assert (kept + skipped == 3).all() and skipped[[0, 63, 64, 129]].tolist() == [3, 3, 3, 3] and int(skipped.sum()) >= 12, (call.name, skipped.tolist())
        assert int(got[1, cells].sum()) == 9 * int(kept.sum()), call.name   # a skipped level adds to nothing else


def test_every_invalid_pair_condition_alone_touches_nothing():
    c = codec()
    for name, call in P.invalid_pair_calls():
        got = stage_pile(c, call)
        assert_pile(got, call.expected(), name)
        assert int((got[0] & np.uint64(0xFFFFFFFF)).sum() + (got[0] >> np.uint64(32)).sum()) == 80, name   # the two good pairs' levels, no more


def test_two_calls_without_clear_equal_one():
    c = codec()
    whole, first, second = P.split_call()
    arena = GuardedPile(c, whole.n_cells)
    stage_pile(c, first, arena)
    got = stage_pile(c, second, arena)
    assert_pile(got, whole.expected(), "two calls")
    assert_pile(stage_pile(c, whole), got, "one call")


def test_an_arena_that_locate_levels_wrote():
    c = codec()
    call = E.levels_tables()[0]   # index with gaps: seven paths, a long stall among them
    n_levels, levels = stage_levels(c, call)
    pairs, hit = np.asarray(call.arrays()[0], np.uint32), np.asarray(call.arrays()[1], np.uint32)
    G = int(pairs[:, 1].max()) + 1
    T = (int(hit[:, 1].max()) + 16) // 16 * 16
    pc = P.PileCall("locate_levels' arena", [T] * G, T, call.W, n_reads=call.arrays()[-1], min_samples=2)
    pc.arrays = lambda: (pairs, hit, n_levels, levels, call.arrays()[-1], None)
    got = stage_pile(c, pc)
    assert_pile(got, pc.expected(), pc.name)
    assert int((got[0] & np.uint64(0xFFFFFFFF)).sum()) > 0


def test_codec_method():
    c = codec()
    dev = c.device
    call = [t for t in P.pile_cases() if t.name == "fit given, REQUIRE_OK"][0]
    pairs, hit, n_levels, levels, n_reads, fit = call.arrays()
    t = [i32(a.reshape(-1)).to(dev).reshape(a.shape) for a in (pairs, hit, n_levels, levels)]
    target, target_len = torch.zeros((2, call.T), dtype=torch.int8, device=dev), i32(call.target_len).to(dev)
    fit_d = i32(fit.reshape(-1)).to(dev).reshape(fit.shape)
    want = call.expected().view(np.int64).reshape(4, 2, call.T)
    made = c.levels_pile(*t, target, target_len, n_reads, fit=fit_d, require_ok=True)
    given = torch.full_like(made, 7)
    back = c.levels_pile(*t, target, target_len, n_reads, fit=fit_d, require_ok=True, clear=True, pile=given)
    twice = c.levels_pile(*t, target, target_len, n_reads, fit=fit_d, require_ok=True, pile=made.clone())
    c.synchronize()
    assert back is given and (made.cpu().numpy() == want).all() and (given.cpu().numpy() == want).all()
    assert (twice.cpu().numpy() == 2 * want).all()
