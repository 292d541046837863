"""CPU test of vbz_compression_amd/csrc/match_path_groups.h, the host's sizing of a path call's scratch and of its groups: plain host
code, so tests/host/match_path_groups_main.cpp -- a stand-alone program -- is built with the address and undefined-behaviour sanitizers
and sweeps every (max_width, ref_stride) inside the header's limits, caps from 0 to 2^64 - 1, and arguments outside the limits.  It exits
non-zero on the first case where a group is empty or larger than the call, exceeds the cap although one pair fits, a pair's words do not
cover what the forward kernel stores, a count wraps in 32 bits, or the packed / wide choice disagrees with its inequality in 64 bits."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_groups_fit_the_cap_and_nothing_wraps(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "match_path_groups")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "vbz_compression_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "match_path_groups_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-2000:])
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[2]) > 100000 and int(words[4]) > 0 and int(words[6]) > 0 and int(words[4]) + int(words[6]) == 8192 * 128, r.stdout
