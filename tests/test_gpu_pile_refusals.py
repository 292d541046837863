"""What the four pile-up calls refuse on the host (include/vbz_gpu_pile.h): -2 with nothing launched and every arena as it was, canaries and
held words alike, and the same arguments, unspoilt, run."""
import pytest
import torch

import pile_ref as P
import squiggle_ref as R
from pile_support import KmersPileTables, KmersTables, PileTables, UpdateTables, assert_pile
from typed_support import codec

pytestmark = pytest.mark.gpu


def refused(got, text):
    rc, msg = got
    assert rc == -2 and text in msg, (rc, msg, text)


def test_levels_pile_refusals_launch_nothing():
    c = codec()
    call = [t for t in P.pile_cases() if t.name == "added to a dirty arena"][0]
    call.use_fit = True
    s = PileTables(c, call)
    refused(s.run(c, locate=None), "locate is NULL")
    for kw in ({"query_len": 0}, {"query_len": 12}, {"query_len": 2056}, {"n_targets": 0}, {"n_targets": 4097}, {"target_stride": 8}, {"target_stride": 360},
               {"target_stride": (1 << 30) + 16}, {"flags": 1}, {"reserved": 1}, {"quant": 0.0}, {"quant": float("nan")}, {"quant": float("inf")}):
        refused(s.run(c, locate=s.locate(**kw)), "locate outside the rules")
    refused(s.run(c, locate=s.locate(target=s.target.data_ptr() + 4)), "not 16-byte aligned")
    for name in ("target", "target_len"):
        refused(s.run(c, locate=s.locate(**{name: None})), "is NULL")
    refused(s.run(c, params=None), "levels pile is NULL")
    for kw in ([{"max_width": w} for w in (0, 4, 12, 65544, 1 << 31)] + [{"flags": f} for f in (4, 8, 0x80000001)]
               + [{"fix": f} for f in (0.0, -1.0, float("nan"), float("inf"), -float("inf"))] + [{"reserved0": 1}, {"reserved1": 1}, {"reserved2": 1}]):
        refused(s.run(c, params=s.params(**kw)), "outside the rules")
    for name in ("pairs", "hit", "n_levels", "levels", "pile"):
        refused(s.run(c, **{name: None}), "is NULL")
    refused(s.run(c, n_pairs=0, pile=None), "is NULL")   # the pile is needed with no pairs too
    for name, p in (("pairs", s.pairs.data_ptr()), ("hit", s.hit.data_ptr()), ("levels", s.levels.data_ptr()), ("fit", s.fit.data_ptr()), ("pile", s.pile.ptr())):
        refused(s.run(c, **{name: p + 8}), "not 16-byte aligned")
    refused(s.run(c, n_pairs=0xFFFFFFFF, params=s.params(max_width=65536)), "not plausible")        # n_pairs * max_width * 32 beyond 2^46
    refused(s.run(c, locate=s.locate(n_targets=4096, target_stride=1 << 30)), "not plausible")     # G * target_stride * 32 beyond 2^46 (2^47 here)
    refused(s.run(c, n_pairs=0, params=s.params(max_width=12)), "outside the rules")                # bad arguments stay refused with no pairs
    assert c.L.vbz_gpu_levels_pile_batch(None, 0, 0, None, None, None, None, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert s.pile.untouched()
    assert s.run(c, n_pairs=0, pairs=None, hit=None, n_levels=None, levels=None, fit=None)[0] == 0   # no pairs, no CLEAR: good, and nothing changes
    c.synchronize()
    assert s.pile.untouched()
    # ... and the same arguments, unspoilt, run
    assert s.run(c)[0] == 0
    c.synchronize()
    assert_pile(s.pile.read("the pile"), call.expected(), call.name)


def test_squiggle_kmers_refusals_launch_nothing():
    c = codec()
    call = [t for t in R.squiggle_cases() if t.name == "lower case and U"][0]
    s = KmersTables(c, call)
    refused(s.run(c, sq=None), "squiggle is NULL")
    for kw in ({"k": 0}, {"k": 10}, {"n_seqs": 0}, {"n_seqs": 2049}, {"n_seqs": 4097, "flags": 0}, {"seq_stride": 0}, {"seq_stride": 8}, {"seq_stride": 3000},
               {"seq_stride": (1 << 30) + 16}, {"target_stride": 0}, {"target_stride": 24}, {"target_stride": (1 << 30) + 16}, {"flags": 4}, {"flags": 0x80000001},
               {"quant": 0.0}, {"quant": -1.0}, {"quant": float("nan")}, {"quant": float("inf")}):
        refused(s.run(c, sq=s.struct(**kw)), "outside the rules")
    for name in ("seq", "seq_len"):
        refused(s.run(c, sq=s.struct(**{name: None})), "is NULL")
    for name in ("kmer", "target_len"):
        refused(s.run(c, **{name: None}), "is NULL")
    refused(s.run(c, sq=s.struct(seq=s.seq.data_ptr() + 4)), "not 16-byte aligned")
    refused(s.run(c, kmer=s.kmer.ptr() + 8), "not 16-byte aligned")
    assert c.L.vbz_gpu_squiggle_kmers_batch(None, None, None, None) == -1
    torch.cuda.synchronize()
    assert s.untouched()
    assert s.run(c)[0] == 0   # (model NULL: not read)
    c.synchronize()
    kmer, target_len = s.read()
    want, want_len = P.squiggle_kmers(call.seq, call.seq_len, call.k, call.target_stride, call.flags)
    assert (kmer == want).all() and (target_len == want_len).all()


def test_pile_kmers_refusals_launch_nothing():
    c = codec()
    call = [t for t in P.pile_kmers_cases() if t.name == "k 5: added to a dirty arena"][0]
    s = KmersPileTables(c, call)
    refused(s.run(c, params=None), "pile kmers is NULL")
    for kw in ({"k": 0}, {"k": 10}, {"rows": 0}, {"rows": 4097}, {"target_stride": 0}, {"target_stride": 8}, {"target_stride": 520}, {"target_stride": (1 << 30) + 16},
               {"flags": 2}, {"flags": 8}, {"flags": 0x80000001}):
        refused(s.run(c, params=s.params(**kw)), "outside the rules")
    for name in ("target_len", "kmer", "pile", "kmer_pile"):
        refused(s.run(c, **{name: None}), "is NULL")
    for name, p in (("kmer", s.kmer.data_ptr()), ("pile", s.pile.data_ptr()), ("kmer_pile", s.kmer_pile.ptr())):
        refused(s.run(c, **{name: p + 8}), "not 16-byte aligned")
    refused(s.run(c, params=s.params(rows=4096, target_stride=1 << 30)), "not plausible")
    assert c.L.vbz_gpu_pile_kmers_batch(None, None, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert s.kmer_pile.untouched()
    assert s.run(c)[0] == 0
    c.synchronize()
    assert_pile(s.kmer_pile.read("the k-mer pile"), call.expected(), call.name)


def test_model_update_refusals_launch_nothing():
    c = codec()
    call = [t for t in P.update_cases() if t.name == "k 6"][0]
    s = UpdateTables(c, call)
    refused(s.run(c, params=None), "model update is NULL")
    for kw in ({"k": 0}, {"k": 10}, {"flags": 1}, {"fix": 0.0}, {"fix": -2.0}, {"fix": float("nan")}, {"fix": float("inf")}):
        refused(s.run(c, params=s.params(**kw)), "outside the rules")
    for name in ("kmer_pile", "prior", "model"):
        refused(s.run(c, **{name: None}), "is NULL")
    refused(s.run(c, kmer_pile=s.kmer_pile.data_ptr() + 8), "not 16-byte aligned")
    assert c.L.vbz_gpu_model_update_batch(None, None, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert s.untouched()
    assert s.run(c)[0] == 0
    c.synchronize()
    model, sd = s.read()
    want_model, want_sd = call.expected()
    assert (model == want_model).all() and (sd == want_sd).all()
