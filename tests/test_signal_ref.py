"""signal_ref.typed_bits, the one statement of the typed store, held to an independent formulation: the same float32 arithmetic, rounded to
float16 and bfloat16 by torch instead of numpy's cast and the integer round-to-nearest-even.  Every 16-bit sample value, signed and
unsigned, under calibrations that reach zero, the chunk pad, overflow to infinity, an infinite scale and NaN, and under seeded ones from
the ranges the device tests draw theirs from (offset in [-600, 600), scale in [0.01, 2.5))."""
import numpy as np
import pytest
import torch

import signal_ref as SR

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
FIXED = [(0.0, 1.0), (-7.0, 1.0), (0.0, 1e5), (0.0, 3e38), (600.0, 3e38), (1.0, float("inf")), (float("nan"), 1.0), (0.0, float("nan")),
         (float("-inf"), 1.0), (-37.5, 0.173)]


def calibrations():
    rng = np.random.default_rng(2024)
    return FIXED + list(zip(rng.uniform(-600.0, 600.0, 36).astype(np.float32).tolist(), rng.uniform(0.01, 2.5, 36).astype(np.float32).tolist()))


def torch_bits(x, o, s, dtype):
    y = (torch.from_numpy(x.astype(np.int32)).to(torch.float32) + torch.tensor(o, dtype=torch.float32)) * torch.tensor(s, dtype=torch.float32)
    if dtype == "f32":
        return y.view(torch.int32).numpy().view(np.uint32)
    return y.to(TORCH[dtype]).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("signed", [True, False], ids=["int16", "uint16"])
def test_typed_bits_against_torch(signed, dtype):
    x = np.arange(65536, dtype=np.uint16)
    x = x.view(np.int16) if signed else x
    nans = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for o, s in calibrations():
            want_nan = np.isnan((x.astype(np.float32) + np.float32(o)) * np.float32(s))
            a, b = SR.typed_bits(x, o, s, dtype), torch_bits(x, o, s, dtype)
            assert a.dtype == b.dtype == (np.uint32 if dtype == "f32" else np.uint16)
            bad = np.flatnonzero((a != b) & ~want_nan)
            assert bad.size == 0, (o, s, "sample", int(x[bad[0]]), hex(int(a[bad[0]])), hex(int(b[bad[0]])))
            assert SR.is_nan_bits(a[want_nan], dtype).all() and SR.is_nan_bits(b[want_nan], dtype).all(), (o, s)
            assert not SR.is_nan_bits(a[~want_nan], dtype).any(), (o, s)
            nans += int(want_nan.sum())
    assert nans == 2 * 65536 + int(signed)   # (the NaN offset, the NaN scale, and 0 x inf at the sample -1)


def test_pad_bits_are_the_pad_rounded_once():
    assert SR.pad_bits(-7.0, "f32") == np.float32(-7.0).view(np.uint32)
    assert SR.pad_bits(-7.0, "f16") == np.float16(-7.0).view(np.uint16)
    assert SR.pad_bits(-7.0, "bf16") == 0xC0E0
    with np.errstate(over="ignore"):
        assert SR.pad_bits(65519.0, "f16") == 0x7BFF and SR.pad_bits(65520.0, "f16") == 0x7C00   # the last value below the tie, and the tie
    assert SR.pad_bits(float("inf"), "bf16") == 0x7F80


def test_chunk_rule_is_strictly_increasing_and_covers_the_read():
    for L, S in ((8, 8), (16, 8), (1024, 1000), (4096, 1024)):
        for mode, ea in (("pad", 0), ("end", 1), ("end", 6), ("end", 8), ("end", 4096)):
            for T in (0, 1, L - 1, L, L + 1, L + S - 1, L + S, L + S + 1, 5 * S + 3, 100_003):
                st = SR.chunk_starts(T, L, S, mode, ea)
                assert len(st) == (0 if T == 0 else 1 if T <= L else -(-(T - L) // S) + 1), (T, L, S, mode, ea)
                if T > L:
                    assert st[-1] + L >= T and st[0] == 0 and all(b - a <= S for a, b in zip(st, st[1:])), (T, L, S, mode, ea, st[-2:])
                assert SR.table_of([T, T], L, S, mode, ea).tolist() == [0, len(st), 2 * len(st)]
