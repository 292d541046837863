"""zstd_pack_kernel's wrapper -- frame header, the loop over a read's two regions, the give-back exits, the checkpoint trailer -- held to
the fused encoder's frames on the reads at its edges.  A backstop to test_gpu_soak_slice's staged-against-fused test: that one has the
shapes that leave the staged form, this one the sizes at which the wrapper itself changes what it writes.

An int16 read of n samples becomes an svb stream of N = ceil(n / 4) control bytes + one or two data bytes per sample; the wrapper looks at
N: below SPLIT_MIN (zstd_encode.hip) the stream is one region, from there on control bytes and data bytes are a region each; the frame
header's content size takes one byte below 256, two below 65 792, four from there on."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _split_min():
    src = open(os.path.join(ROOT, "vbz_compression_amd", "csrc", "zstd_encode.hip")).read()
    return int(re.search(r"constexpr uint32_t SPLIT_MIN = (\d+);", src).group(1))


CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import gpu_util as G, oracle_lib as O, typed_support as T
from vbz_compression_amd import _lib
SPLIT_MIN = int(sys.argv[1])
rng = np.random.default_rng(17)
def stream_bytes(a):
    return len(O.svb_compress(a, 2, True))
def one_byte(n, steps):   # every delta one data byte, but for `steps` steps of 300 (two bytes each)
    a = rng.integers(-50, 51, n)
    for p in np.linspace(n // 3, n - 1, steps).astype(int) if steps else []:
        a[p:] += 300
    return a.astype(np.int16)
def two_byte(n):          # every delta two data bytes
    return (np.where(np.arange(n) & 1, -1000, 1000) + rng.integers(-50, 51, n)).astype(np.int16)
def with_stream_of(N):    # a read of one-byte deltas whose svb stream is exactly N bytes
    n = max(k for k in range(N + 1) if k + (k + 3) // 4 <= N)
    a = one_byte(n, N - (n + (n + 3) // 4))
    assert stream_bytes(a) == N, (N, n, stream_bytes(a))
    return a
n2 = max(k for k in range(SPLIT_MIN) if 2 * k + (k + 3) // 4 < SPLIT_MIN)   # two-byte deltas: the last read of one region
# the sample counts themselves, on the benchmark's generator
reads = [O.synth_signal(5, 9000 + i, n) for i, n in enumerate([0, 1, SPLIT_MIN // 2 - 1, SPLIT_MIN // 2, 255, 256, 65791, 65792, 100003])]
# ... and reads whose STREAMS stand at those sizes: the last of one region and the first of two (one-byte and two-byte deltas),
# the frame header's three forms
reads += [with_stream_of(SPLIT_MIN - 1), with_stream_of(SPLIT_MIN), two_byte(n2), two_byte(n2 + 1)]
reads += [with_stream_of(N) for N in (255, 256, 65791, 65792)]
assert stream_bytes(reads[-6]) < SPLIT_MIN <= stream_bytes(reads[-5]), (stream_bytes(reads[-6]), stream_bytes(reads[-5]))
opts = _lib.CompressionOptions(True, 2, 1, 1)
ref = O.options(True, 2, 1, 1)
out = {}
for staged in (1, 0):
    for trailers in (1, 0):
        c = T.codec(VBZ_HIP_STAGED_ENCODE=staged, VBZ_HIP_TRAILERS=trailers, VBZ_HIP_SEGMENTED=0, VBZ_HIP_ROUTING=0)
        G.codec = lambda: c
        frames = G.compress(reads, opts)                                  # slots of the exact bound
        for a, f in zip(reads, frames):
            assert not isinstance(f, int), (len(a), f)
            assert O.decompress(f, a.nbytes, ref).tobytes() == a.tobytes(), len(a)
        caps = [len(f) - 1 for f in frames]                               # one byte short of what that frame needs
        tight = G.run_stage(lambda cc, *x: cc.compress(*x, opts, sized=False), reads, caps)
        for a, f in zip(reads, tight):                                    # (a frame that does fit: the same read without its trailer)
            assert isinstance(f, int) or O.decompress(f, a.nbytes, ref).tobytes() == a.tobytes(), len(a)
        out["%%d%%d" %% (staged, trailers)] = [[f if isinstance(f, int) else hashlib.sha256(f.tobytes()).hexdigest() for f in fs] for fs in (frames, tight)]
        out["given_back%%d%%d" %% (staged, trailers)] = sum(isinstance(f, int) for f in tight)
print("RESULT", json.dumps(out))
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_pack_wrapper_writes_the_fused_encoders_frames():
    """Frames of the staged encoder against VBZ_HIP_STAGED_ENCODE=0 (one child process, a context per setting), byte for byte: reads of 0, 1,
    SPLIT_MIN / 2 - 1, SPLIT_MIN / 2, 255, 256, 65 791, 65 792 and 100 003 samples, and reads whose svb streams are SPLIT_MIN - 1 and
    SPLIT_MIN bytes (the last of one region, the first of two) and 255, 256, 65 791 and 65 792 bytes (the frame header's three
    content-size forms); each into a slot of the exact bound and into one a byte shorter than its frame (the give-back exits: the
    same verdict, or the same frame without its trailer); with and without checkpoint trailers."""
    r = subprocess.run([sys.executable, "-c", CHILD, str(_split_min())], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][7:])
    for trailers in "10":
        for k, what in enumerate(("exact slots", "tight slots")):
            a, b = got["1" + trailers][k], got["0" + trailers][k]
            differ = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
            assert not differ, (trailers, what, differ)
    # the tight slots did take the give-back exits: without a trailer to drop, hardly a frame gets a byte shorter
    assert got["given_back10"] >= 10, got["given_back10"]
