"""CPU test of vbz_compression_amd/csrc/scratch_tables.h, the layouts of the host's device scratch: every table's carve() both measures
(base == nullptr) and places its arrays, and a buffer is allocated from the measurement alone -- so the measurement must cover what the
carve places.  tests/host/scratch_tables_harness.cpp runs, per table and per set of dimensions, the measuring pass and then the carving
pass into a malloc of exactly the measured size (and once more into another block), and prints every array's offset, element size and
count.  Held here, per case:

- both passes return the same size, and the measuring pass leaves every pointer null (it yields no addresses, so "the same offsets"
  is: the same total, and the same offsets from two carving passes at different bases);
- every array starts 16-byte aligned, lies inside the buffer, overlaps no other, and has the element size and the count the struct
  documents (EXPECT below: this file's own statement of them, e.g. n + 1 for SegTables::first and the window scan);
- the size is at least the end of the last array plus 512 bytes (MetaCarver::bytes(): a quarter more + 512);
- measuring alone, 2^32 - 1 reads and 2^31 - 1 segments: the size is no less than the arrays' bytes (no 32-bit wrap).

The program makes no HIP call and runs without a device; it is built with hipcc because the header includes vbz_kernels.h."""
import os
import shutil
import subprocess

import pytest

from vbz_compression_amd.build import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = (0, 1, 3, 5, 1024, 65536)
N_MAX = 0xFFFFFFFF
NORM_READ, POD5_ROW, POD5_READ, FLOAT2, UINT2 = 80, 16, 16, 8, 8
ROUTE_MAX_READS, ROUTE_CAND_WORDS = 16, 4096   # (the second is the caller's to give: any count will do here)


def _per_read(*arrays):
    return lambda n: [(name, elem, n + extra if per_n else extra) for name, elem, per_n, extra in arrays]


# table -> (dimension sets to carve, dimension sets to measure only, dims -> [(array, element bytes, count)])
EXPECT = {
    "StageSlots": ([(n,) for n in N], [(N_MAX,)], _per_read(("t.svb_off", 8, 1, 0), ("t.svb_cap", 4, 1, 0), ("t.svb_size", 4, 1, 0), ("t.gate", 4, 1, 0),
                                                             ("t.deep_d", 4, 1, 0), ("t.key_raw", 4, 1, 0), ("t.gate2", 4, 1, 0))),
    "SplitTables": ([(n,) for n in N], [(N_MAX,)], _per_read(("t.svb_off", 8, 1, 0), ("t.svb_cap", 4, 1, 0), ("t.gate", 4, 1, 0), ("t.svb_size", 4, 1, 0))),
    "CanonGates": ([(n,) for n in N], [(N_MAX,)], _per_read(("t.counts", 4, 0, 4), ("t.gate_small", 4, 1, 0), ("t.gate_large", 4, 1, 0))),
    "TypedSlots": ([(n,) for n in N], [(N_MAX,)], _per_read(("t.off16", 8, 1, 0), ("t.cap16", 4, 1, 0), ("t.cal", FLOAT2, 1, 0))),
    "NormTables": ([(n,) for n in N], [(N_MAX,)], _per_read(("t.st", NORM_READ, 1, 0), ("t.ss", FLOAT2, 1, 0))),
    "SizedTables": ([(n,) for n in N], [(N_MAX,)], _per_read(("t.pay_off", 8, 1, 0), ("t.pay_size", 4, 1, 0), ("t.orig_size", 4, 1, 0), ("t.gate", 4, 1, 0))),
    "WindowScratch": ([(n,) for n in N], [(N_MAX,)], _per_read(("t.scan", 8, 1, 1), ("t.count", 4, 1, 0))),
    "SegTables": ([(n, s) for n in N for s in (1, 5)], [(n, 0x7FFFFFFF) for n in N] + [(N_MAX, 5), (N_MAX, 0x7FFFFFFF)],
                  lambda n, s: [("t.first", 4, n + 1), ("t.gate", 4, n), ("t.val", 4, s), ("t.off", 8, s), ("t.run", 4, s)]),
    "RouteTables": ([(n, ROUTE_MAX_READS, ROUTE_CAND_WORDS) for n in N], [(N_MAX, ROUTE_MAX_READS, ROUTE_CAND_WORDS)],
                    lambda n, m, c: [("t.gate_small", 4, n), ("t.large.src_off", 8, m), ("t.large.dst_off", 8, m), ("t.large.src_size", 4, m),
                                     ("t.large.dst_cap", 4, m), ("t.large.gate", 4, m), ("t.result", 4, m), ("t.large.map", 4, m),
                                     ("t.large.cal", FLOAT2, m), ("t.large.row", 8, m), ("t.norm", NORM_READ, m), ("t.large.count", 4, 4), ("t.cand", 4, c)]),
    "Pod5Tables": ([(0, 0), (1, 1), (7, 3), (200, 1)], [(N_MAX, N_MAX)],
                   lambda rows, r: [("t.pr.bad", 4, 4), ("t.pr.rows", POD5_ROW, rows), ("t.pr.reads", POD5_READ, r), ("t.cal", FLOAT2, r),
                                    ("t.pr.range", UINT2, r)]),
}


def _case(table, dims, measure_only):
    return "%s:%s%s" % (table, ",".join(str(d) for d in dims), ":m" if measure_only else "")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """One build and one run over every case: case -> ({measured, carved, null_when_measuring}, [(array, elem, count, offset, offset again)])"""
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("scratch_tables") / "harness")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "vbz_compression_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "host", "scratch_tables_harness.cpp")])
    cases = [_case(t, d, False) for t, (carved, _, _) in EXPECT.items() for d in carved]
    cases += [_case(t, d, True) for t, (_, measured, _) in EXPECT.items() for d in measured]
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


@pytest.mark.parametrize("table", sorted(EXPECT))
def test_carve_places_what_it_measured(report, table):
    carved, _, expect = EXPECT[table]
    for dims in carved:
        head, arrays = report[_case(table, dims, False)]
        total = head["measured"]
        assert head["carved"] == total and head["null_when_measuring"] == 1, (dims, head)
        assert [(a[0], a[1], a[2]) for a in arrays] == expect(*dims), dims   # the arrays, their element sizes, the documented counts
        spans = []
        for name, elem, count, off, off_again in arrays:
            assert off == off_again, (dims, name)
            assert off >= 0 and off % 16 == 0 and off + elem * count <= total, (dims, name, off, total)
            spans.append((off, off + elem * count, name))
        spans.sort()
        for (_, end, a), (start, _, b) in zip(spans, spans[1:]):
            assert end <= start, (dims, a, b)
        assert total >= max(e for _, e, _ in spans) + 512, (dims, total)


@pytest.mark.parametrize("table", sorted(EXPECT))
def test_measuring_does_not_wrap(report, table):
    _, measured, expect = EXPECT[table]
    for dims in measured:
        head, _ = report[_case(table, dims, True)]
        need = sum(elem * count for _, elem, count in expect(*dims))
        assert need > 0xFFFFFFFF   # (a case that could not show a wrap checks nothing)
        assert head["null_when_measuring"] == 1 and head["measured"] >= need + 512, (dims, head, need)
