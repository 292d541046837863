"""CPU test of vbz_compression_amd/csrc/match_select.h, the host's choice between the packed and the wide span kernel: plain host code,
so tests/host/match_select_main.cpp -- a stand-alone program -- is built with the address and undefined-behaviour sanitizers and sweeps
every (query_len, ref_stride) inside the header's limits, and arguments outside them.  It exits non-zero on the first pair where the
answer is "packed" and a key could wrap, or "wide" inside the packed rule."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_only_where_nothing_wraps(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "match_select")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "vbz_compression_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "match_select_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-2000:])
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[2]) > 0 and int(words[4]) > 0 and int(words[2]) + int(words[4]) == 8192 * 128, r.stdout
