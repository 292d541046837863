"""vbz_gpu_squiggle_kmers_batch on the MI355X, bit for bit against tests/pile_ref.py over squiggle_ref's catalogue: k = 1 ... 9, all four flag
combinations, invalid bases at every slot of a lane's 24 bytes, lengths around a lane's 16 and a wavefront's 1 024 -- canary words around
every arena; the squiggle call's int8 target recomputed from model[kmer] equals that call's; the marks fall where that call counts."""
import numpy as np
import pytest

import pile_ref as P
import squiggle_ref as R
from pile_support import stage_kmers
from squiggle_support import stage_squiggle
from typed_support import codec

pytestmark = pytest.mark.gpu


def test_catalogue_bit_for_bit():
    c = codec()
    seen = set()
    for call in P.kmers_cases():
        kmer, target_len = stage_kmers(c, call)
        want, want_len = P.squiggle_kmers(call.seq, call.seq_len, call.k, call.target_stride, call.flags)
        bad = np.argwhere(kmer != want)
        assert bad.size == 0, (call.name, len(bad), bad[:6].tolist(), [hex(int(kmer[tuple(b)])) for b in bad[:6]], [hex(int(want[tuple(b)])) for b in bad[:6]])
        assert (target_len == want_len).all(), (call.name, target_len.tolist(), want_len.tolist())
        seen.add((call.k, call.flags))
    assert seen >= {(k, f) for k in range(1, 10) for f in (0, 1, 2, 3)}, sorted(seen)


def test_the_squiggle_calls_target_from_model_of_kmer():
    c = codec()
    for call in [t for t in R.squiggle_cases() if "invalid bases" in t.name or "special values" in t.name or "refused lengths" in t.name]:
        kmer, kmer_len = stage_kmers(c, call)
        target, target_len, masked, level = stage_squiggle(c, call)
        live = kmer != P.MARK
        m = np.where(live, call.model[np.where(live, kmer, 0)], np.uint32(0))
        assert (kmer_len == target_len).all(), call.name
        assert (np.where(live, R.quantise(m, call.quant), np.int8(0)) == target).all(), call.name
        assert level is None or (m == level).all(), call.name
        inside = np.arange(call.target_stride)[None, :] < target_len[:, None]
        assert ((~live & inside).sum(axis=1) == masked).all(), (call.name, masked.tolist())   # the marks in front of L are the masked k-mers
        assert not (live & ~inside).any(), call.name
