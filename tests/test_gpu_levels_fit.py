"""vbz_gpu_levels_fit_batch on the MI355X, bit for bit against tests/squiggle_ref.py over level arenas built in numpy: widths 1 ... 65 536,
K at 0, 1 and 2, flat targets, falling and level lines, both filters on each side of a turn's seam, means at the bound, wrapped sums, every
residue of a dword, stretches that end at L_g, the extreme case, with and without the prior and the sums -- canary words around every
arena; an exact-recovery case with no tolerance; and GpuCodec.levels_fit into given tensors."""
import numpy as np
import pytest
import torch

import squiggle_ref as R
from squiggle_support import assert_fit, stage_fit
from typed_support import codec, i32
from vbz_compression_amd import batch

pytestmark = pytest.mark.gpu


def test_catalogue_bit_for_bit():
    c = codec()
    for call in R.fit_cases():
        assert_fit(stage_fit(c, call), call.expected(), call)


def test_exact_recovery_has_no_tolerance():
    c = codec()
    call = R.exact_call()
    out, offset, scale, sums = stage_fit(c, call)
    for p, (a, b) in enumerate(call.planted):
        assert out[p][3] == 1 and offset[p:p + 1].view(np.float32)[0] == np.float32(-b), (p, a, b, out[p].tolist())
        assert scale[p:p + 1].view(np.float32)[0] == np.float32(1.0 / (a * 32.0)), (p, a, b, out[p].tolist())


def test_codec_method_into_given_tensors():
    c = codec()
    dev = c.device
    call = R.fit_cases()[0]
    pairs, hit, n_levels, levels, n_reads, prior = call.arrays()
    want_out, want_sums = call.expected()
    t = [i32(a.reshape(-1)).to(dev).reshape(a.shape) for a in (pairs, hit, n_levels, levels)]
    target, target_len = torch.from_numpy(call.target).to(dev), i32(call.target_len).to(dev)
    pr = torch.from_numpy(prior.view(np.float32).copy()).to(dev)
    loc = batch.Locate(query_len=128, quant=call.quant)
    out, offset, scale, sums = c.levels_fit(*t, target, target_len, n_reads, loc, prior=pr, sums=True)
    given = (torch.full_like(out, 7), torch.full_like(offset, 7.0), torch.full_like(scale, 7.0), torch.full_like(sums, 7))
    back = c.levels_fit(*t, target, target_len, n_reads, loc, prior=pr, sums=given[3], out=given[0], offset=given[1], scale=given[2])
    none = c.levels_fit(*t, target, target_len, n_reads, loc, prior=pr)
    c.synchronize()
    assert all(a is b for a, b in zip(back, given)) and none[3] is None
    for o, of, sc, sm in ((out, offset, scale, sums), given, none):
        assert (o.cpu().numpy().view(np.uint32) == want_out).all()
        assert (of.cpu().numpy().view(np.uint32) == want_out[:, 0]).all() and (sc.cpu().numpy().view(np.uint32) == want_out[:, 1]).all()
        assert sm is None or (sm.cpu().numpy() == want_sums).all()
