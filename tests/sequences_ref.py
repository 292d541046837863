"""The plain statement of what the encoder's entropy stage (vbz_compression_amd/csrc/zstd_encode.hip) must find in a block: which bytes
become matches, which stay literals, and which decoder checkpoints go into the frame's trailer.  Numpy and Python integers only; the
constants are read from the sources, so the statement follows them.  tests/test_sequences_ref.py holds it to a brute-force loop,
tests/test_gpu_encoder_sequences.py holds the device's frames to it.

Runs (tokenise_runs<false>, the control bytes of an svb stream): mark every position whose byte equals the byte in front of it; the
positions that lie in RMIN - 1 or more consecutive marks are matched (the morphological opening of the marks by RMIN - 1) and every
maximal stretch of them is one sequence with offset 1.  A run of r >= RMIN equal bytes is therefore one literal (its first byte, which
nothing in front of it equals) and a match of r - 1: the rule is "equal bytes", not "zero bytes".

Periods (tokenise_runs<true> over period_mask, the long-repeat matcher): the same with "equals the byte D in front of it", an opening by
RPER, and a chunk [begin, end) of the region tokenised as if nothing stood in front of it (the marks in front of `begin` do not count,
though a match's source may lie there).  No byte of such a match stays a literal."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(path, pattern):
    m = re.search(pattern, open(os.path.join(ROOT, "vbz_compression_amd", "csrc", path)).read())
    assert m, (path, pattern)
    return int(m.group(1)) << int(m.group(2)) if m.lastindex == 2 else int(m.group(1))


RMIN = _constant("vbz_kernels.h", r"#define VBZ_RMIN (\d+)")
RPER = _constant("zstd_encode.hip", r"constexpr uint32_t RPER = (\d+);")
BLOCK_MAX = _constant("zstd_encode.hip", r"constexpr uint32_t BLOCK_MAX = (\d+)u << (\d+);")
CP_MIN_SPACING = _constant("zstd_encode.hip", r"constexpr uint32_t CP_MIN_SPACING = (\d+);")
CP_MAX = 64   # encode_zero_run_sequences: at most 63 checkpoints and the start, one decoder lane each
# the large-read path cuts a control-byte region into spans of at most KEYSPAN bytes (twice that from KEYSPAN_LARGE_FROM control bytes
# on; KEYSPAN_SHARED where the read's data bytes share one table: one- and two-byte integers), evenly: span j of n is [K j / n, K (j + 1) / n)
KEYSPAN = _constant("zstd_encode.hip", r"#define VBZ_KEYSPAN_KB (\d+)") << 10
KEYSPAN_SHARED = _constant("zstd_encode.hip", r"#define VBZ_KEYSPAN_SHARED_KB (\d+)") << 10
KEYSPAN_LARGE_FROM = _constant("zstd_encode.hip", r"KEYSPAN_LARGE_FROM = (\d+)u << (\d+);")
TOK_MIN = 256   # a region below this is not tokenised (zstd_encode.hip: S >= 256 && S <= BLOCK_MAX)
# a stream below SPLIT_MIN is not cut into control and data bytes: it is ONE region, tokenised as a whole, on every path
SPLIT_MIN = _constant("zstd_encode.hip", r"constexpr uint32_t SPLIT_MIN = (\d+);")


def key_spans(K, shared=False):
    """the extents the large-read path cuts a control-byte region of K bytes into"""
    limit = KEYSPAN_SHARED if shared else (2 * KEYSPAN if K >= KEYSPAN_LARGE_FROM else KEYSPAN)
    n = (K + limit - 1) // limit
    return [(K * j // n, K * (j + 1) // n) for j in range(n)]


def _opened(m, r):
    """the morphological opening of the boolean marks by r: [(a, b)], every maximal stretch m[a .. b] of r or more marks"""
    edges = np.diff(np.concatenate([[0], m.astype(np.int8), [0]]))
    first, behind = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)
    return [(int(a), int(b) - 1) for a, b in zip(first, behind) if b - a >= r]


def _sequences(x, matched):
    """(pairs, literals) of the stretches `matched` of x: pairs (literal length, match length), literals = every byte
    outside the stretches, the tail behind the last one included"""
    keep = np.ones(len(x), bool)
    pairs, at = [], 0
    for a, b in matched:
        pairs.append((a - at, b - a + 1))
        keep[a : b + 1] = False
        at = b + 1
    return pairs, x[keep]


def runs_ref(block_bytes, rmin=None):
    """(pairs, literals) of a block of control bytes: pairs = [(literal length, match length)] of its sequences, all with offset 1;
    literals = the bytes that stay, the tail behind the last sequence included (so the tail is len(literals) - sum of the literal lengths)"""
    rmin = RMIN if rmin is None else rmin
    x = np.ascontiguousarray(block_bytes).view(np.uint8).reshape(-1)
    m = np.zeros(len(x), bool)
    m[1:] = x[1:] == x[:-1]
    return _sequences(x, _opened(m, rmin - 1))


def period_ref(region, begin, end, D, rper=None):
    """(pairs, literals) of the chunk region[begin : end] under the distance D: pairs = [(literal length, match length)] of its sequences,
    every one with the explicit offset D; literals as runs_ref's"""
    rper = RPER if rper is None else rper
    x = np.ascontiguousarray(region).view(np.uint8).reshape(-1)
    m = np.zeros(len(x), bool)
    if D < len(x):
        m[D:] = x[D:] == x[: len(x) - D]
    return _sequences(x[begin:end], _opened(m[begin:end], rper))


def checkpoint_spacing(nseq):
    spacing = CP_MIN_SPACING
    while (nseq + spacing - 1) // spacing > CP_MAX:
        spacing *= 2
    return spacing


def checkpoints_ref(seqs_of_block):
    """(spacing, words) of a block's checkpoint trailer from its listing (oracle_lib.zstd_sequences' records of that block): word j is what
    a decoder holds at the head of sequence (j + 1) x spacing -- unread bits | literal-length state << 20 | match-length state << 26"""
    nseq = len(seqs_of_block)
    spacing = checkpoint_spacing(nseq)
    words = []
    for j in range((nseq - 1) // spacing if nseq else 0):
        s = seqs_of_block[(j + 1) * spacing]
        unread, ll_state, ml_state = int(s["unread"]), int(s["ll_state"]), int(s["ml_state"])
        assert 0 <= unread < 1 << 20 and ll_state < 64 and ml_state < 64, (unread, ll_state, ml_state)
        words.append(unread | ll_state << 20 | ml_state << 26)
    return spacing, words
