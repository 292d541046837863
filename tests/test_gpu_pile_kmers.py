"""vbz_gpu_pile_kmers_batch on the MI355X, bit for bit against tests/pile_ref.py: k = 1 ... 9 at L up to a few thousand with the table in LDS
and with global adds (DIRECT) at every k, so both sides of the LDS rule wherever it lands; every position on one k-mer; marks and keys
beyond 4^k; target_len 0 and beyond the stride; rows 1 and 5; CLEAR and accumulate over a dirty arena; all-zero cells -- canary words around
the k-mer arena; the pile of a position pile equals a direct per-k-mer pile of the levels; and GpuCodec.pile_kmers."""
import numpy as np
import pytest
import torch

import pile_ref as P
from pile_support import assert_pile, stage_pile, stage_pile_kmers
from typed_support import codec, i32

pytestmark = pytest.mark.gpu


def test_catalogue_bit_for_bit():
    c = codec()
    for call in P.pile_kmers_cases():
        assert_pile(stage_pile_kmers(c, call), call.expected(), call.name)


def test_positions_then_kmers_equal_a_direct_pile_of_the_levels():
    c = codec()
    rng = np.random.default_rng(2811)
    call = [t for t in P.pile_cases() if t.name == "staggered overlaps"][0]
    pile = stage_pile(c, call)
    for k in (2, 6):
        kmer = rng.integers(0, 4 ** k, (2, call.T)).astype(np.uint32)
        kc = P.KmersPileCall("after levels_pile, k %d" % k, k, kmer, call.target_len, pile)
        got = stage_pile_kmers(c, kc)
        direct = np.zeros((4, 4 ** k), np.uint64)
        pairs, hit, n_levels, levels, n_reads, fit = call.arrays()
        for p in range(len(pairs)):
            keep, u, ns = P.level_values(levels[p, :n_levels[p]], 0.0, 1.0, call.fix, 0, 0)
            key = kmer[pairs[p][1], hit[p][2]:hit[p][1]].astype(np.int64)
            for q, v in enumerate((np.where(keep, np.uint64(1), P.SKIP), np.where(keep, ns, np.uint64(0)), u.astype(np.uint64), (u * u).astype(np.uint64))):
                np.add.at(direct[q], key, v)
        assert_pile(got, direct, kc.name)


def test_codec_method():
    c = codec()
    dev = c.device
    call = [t for t in P.pile_kmers_cases() if t.name == "k 4 rows 5"][0]
    rows, T = call.kmer.shape
    pile = torch.from_numpy(call.pile.view(np.int64).reshape(4, rows, T).copy()).to(dev)
    kmer, target_len = i32(call.kmer.reshape(-1)).to(dev).reshape(rows, T), i32(call.target_len).to(dev)
    want = call.expected().view(np.int64)
    made = c.pile_kmers(pile, kmer, target_len, 4)
    given = torch.full_like(made, 7)
    back = c.pile_kmers(pile, kmer, target_len, 4, clear=True, direct=True, kmer_pile=given)
    twice = c.pile_kmers(pile, kmer, target_len, 4, kmer_pile=made.clone())
    c.synchronize()
    assert back is given and (made.cpu().numpy() == want).all() and (given.cpu().numpy() == want).all() and (twice.cpu().numpy() == 2 * want).all()
