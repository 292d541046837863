"""The timed instantiation of the staged encoder's planning launch (VBZ_HIP_PHASE_TIMING=2, experiments build of the library): a
measurement aid, but it must plan what the product's launch plans -- the same frames byte for byte -- and it must report both roles."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = r"""
import hashlib, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import gpu_util as G, oracle_lib as O
from vbz_compression_amd import _lib
reads = [O.synth_signal(5, 9100 + i, n) for i, n in enumerate([100000, 65536, 33333, 4096, 1640, 250000, 17, 0] * 3)]
opts = _lib.CompressionOptions(True, 2, 1, 1)
frames = G.compress(reads, opts)
back = G.decompress(frames, [a.nbytes for a in reads], opts)
for a, f, b in zip(reads, frames, back):
    assert not isinstance(f, int) and not isinstance(b, int) and b.tobytes() == a.tobytes()
    assert O.decompress(f, a.nbytes, O.options(True, 2, 1, 1)).tobytes() == a.tobytes()
print("frames", sum(len(f) for f in frames), hashlib.sha256(b"".join(f.tobytes() for f in frames)).hexdigest())
""" % (ROOT, os.path.join(ROOT, "tests"))


def _frames(env):
    r = subprocess.run([sys.executable, "-c", CODE], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("frames")][-1].split()
    return line[1:3], r.stderr


def test_timed_planning_launch_writes_the_same_frames():
    from vbz_compression_amd import _lib

    plain, _ = _frames(dict(os.environ, VBZ_HIP_PHASE_TIMING="0", VBZ_HIP_SEGMENTED="0"))
    timed, err = _frames(dict(os.environ, VBZ_HIP_PHASE_TIMING="2", VBZ_HIP_SEGMENTED="0", VBZ_HIP_LIB=_lib.EXPERIMENTS_LIB_PATH))
    assert timed == plain
    lines = [ln for ln in err.splitlines() if ln.startswith("vbz_hip phase cycles/read (zstd_plan:")]
    assert any(", role 0, n=" in ln for ln in lines) and any(", role 1, n=" in ln for ln in lines), err[-2000:]
    # the bench-sized reads plan in both roles: some wavefront of each role reported non-zero counters
    role0 = [ln for ln in lines if ", role 0, n=" in ln]
    assert any(" p1=0 " not in ln for ln in role0), role0   # the tokeniser ran
