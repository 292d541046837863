"""vbz_gpu_model_update_batch on the MI355X, bit for bit against tests/pile_ref.py: n on both sides of min_obs, a count word with skipped in
its high half, negative sums, var rounding below zero, the prior's 32 bits (NaN payloads, -0) kept, prior in place, sd NULL, k = 1 ... 9 --
canary words around both outputs; and GpuCodec.model_update."""
import numpy as np
import pytest
import torch

import pile_ref as P
from pile_support import stage_update
from typed_support import codec

pytestmark = pytest.mark.gpu


def test_catalogue_bit_for_bit():
    c = codec()
    for call in P.update_cases():
        model, sd = stage_update(c, call)
        want_model, want_sd = call.expected()
        bad = np.flatnonzero(model != want_model)
        assert bad.size == 0, (call.name, "model", bad[:6].tolist(), [hex(int(v)) for v in model[bad[:6]]], [hex(int(v)) for v in want_model[bad[:6]]])
        assert (sd is None) == (not call.use_sd)
        if sd is not None:
            bad = np.flatnonzero(sd != want_sd)
            assert bad.size == 0, (call.name, "sd", bad[:6].tolist(), [hex(int(v)) for v in sd[bad[:6]]], [hex(int(v)) for v in want_sd[bad[:6]]])


def test_codec_method():
    c = codec()
    dev = c.device
    call = [t for t in P.update_cases() if t.name == "k 6"][0]
    kp = torch.from_numpy(call.kmer_pile.view(np.int64).copy()).to(dev)
    prior = torch.from_numpy(call.prior.view(np.float32).copy()).to(dev)
    want_model, want_sd = call.expected()
    model, sd = c.model_update(kp, prior, 6, min_obs=call.min_obs, sd=True)
    none = c.model_update(kp, prior, 6, min_obs=call.min_obs)
    place = prior.clone()
    back = c.model_update(kp, place, 6, min_obs=call.min_obs, model=place)
    c.synchronize()
    assert none[1] is None and back[0] is place
    for m in (model, none[0], place):
        assert (m.cpu().numpy().view(np.uint32) == want_model).all()
    assert (sd.cpu().numpy().view(np.uint32) == want_sd).all()
