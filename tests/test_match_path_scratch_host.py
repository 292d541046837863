"""CPU test of MatchPathScratch (vbz_compression_amd/csrc/scratch_tables.h), the scratch of one group of a path call, held to what
tests/test_scratch_tables_host.py holds every other table to: the measuring pass leaves every pointer null and returns what the carving
pass returns; every array starts 16-byte aligned, lies inside a buffer of exactly the measured size, overlaps no other and has the
documented element size and count -- pairs x match_path_groups.h's words a pair of direction bits, and one cost a pair; the size is at
least the end of the last array plus 512 bytes; measuring 2^32 - 1 pairs of the largest window does not wrap.
tests/host/match_path_scratch_harness.cpp prints scratch_tables_harness.cpp's format; it makes no HIP call and runs without a device."""
import os
import shutil
import subprocess

import pytest

from vbz_compression_amd.build import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MAX = 0xFFFFFFFF
CARVED = [(0, 8, 16), (1, 8, 16), (3, 8, 16), (5, 136, 2048), (1, 4096, 2048), (97, 2048, 416), (7, 65536, 144)]
MEASURED = [(N_MAX, 65536, 2048), (N_MAX, 8, 16), (8192, 65536, 2048)]


def pair_words(width, stride):
    """match_path_groups.h, stated once more: 64 x ceil((max_width + 63) c / 16), c the rows per lane of ref_stride"""
    c = next(c for c in (1, 2, 4, 8, 16, 32) if 64 * c >= stride)
    return 64 * (((width + 63) * c + 15) // 16)


def case(dims, measure_only):
    return "MatchPathScratch:%d,%d,%d%s" % (dims + (":m" if measure_only else "",))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("match_path_scratch") / "harness")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "vbz_compression_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "host", "match_path_scratch_harness.cpp")])
    cases = [case(d, False) for d in CARVED] + [case(d, True) for d in MEASURED]
    out = subprocess.run([exe] + cases, capture_output=True, text=True, check=True).stdout
    rep = {}
    for ln in out.splitlines():
        w = ln.split()
        if w[0] == "case":
            cur = rep[w[1]] = (dict(zip(w[2::2], (int(v) for v in w[3::2]))), [])
        else:
            cur[1].append((w[1],) + tuple(int(v) for v in w[2:]))
    assert sorted(rep) == sorted(cases)
    return rep


def test_carve_places_what_it_measured(report):
    for dims in CARVED:
        head, arrays = report[case(dims, False)]
        total = head["measured"]
        assert head["carved"] == total and head["null_when_measuring"] == 1, (dims, head)
        assert [(a[0], a[1], a[2]) for a in arrays] == [("t.bits", 4, dims[0] * pair_words(dims[1], dims[2])), ("t.cost", 4, dims[0])], dims
        spans = []
        for name, elem, count, off, off_again in arrays:
            assert off == off_again, (dims, name)
            assert off >= 0 and off % 16 == 0 and off + elem * count <= total, (dims, name, off, total)
            spans.append((off, off + elem * count, name))
        spans.sort()
        for (_, end, a), (start, _, b) in zip(spans, spans[1:]):
            assert end <= start, (dims, a, b)
        assert total >= max(e for _, e, _ in spans) + 512, (dims, total)


def test_measuring_does_not_wrap(report):
    for dims in MEASURED:
        head, _ = report[case(dims, True)]
        need = 4 * dims[0] * pair_words(dims[1], dims[2]) + 4 * dims[0]
        assert need > 0xFFFFFFFF   # (a case that could not show a wrap checks nothing)
        assert head["null_when_measuring"] == 1 and head["measured"] >= need + 512, (dims, head, need)
