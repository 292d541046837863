#!/usr/bin/env python3
"""CPU model of fast_streams_kernel's refill path (zstd_decode_fast.hip): how many periods of a wavefront execute the path and for how
many lanes, by period and trigger.  No GPU needed.

64 lanes, one stream each of `symbols` symbols whose code lengths are normal (mean 6.5 bits, sd 2, clipped to 1 .. 11); the first 64-byte
line holds 0 .. 63 bytes above the stream's end; a 32-dword ring filled with two lines at the start; one look at the ring per period; a
request is committed at the end of its period.  Trigger 0 is every lane for itself (a refill as soon as 16 dwords or fewer are unread);
a trigger T > 0 refills every lane that has room in the periods in which some lane with input left holds T unread dwords or fewer.
The model also reports the lowest number of unread dwords a lane with input left ever saw at the top of a period.

    python tools/stream_refill_model.py [wavefronts] [symbols]
"""
import sys

import numpy as np

RING, BATCH, LANES = 32, 16, 64


def run(period, trigger, waves, symbols, seed=1):
    rng = np.random.default_rng(seed)
    periods = refills = issued = 0
    low_water = RING
    for _ in range(waves):
        lens = np.clip(np.rint(rng.normal(6.5, 2.0, (LANES, symbols))), 1, 11).astype(np.int64)
        pad = rng.integers(0, 64, LANES)
        start = 8 * pad + rng.integers(1, 9, LANES)          # bits gone before the first symbol: the bytes above the end, the end mark
        total = start + lens.sum(axis=1)
        lines = (total + 511) // 512                        # lines the stream touches
        fetched = np.minimum(lines, 2)
        widx = fetched * BATCH
        used = start.copy()                                 # bits consumed
        cum = np.cumsum(lens, axis=1)
        for p in range(symbols // period):
            unread = widx - (used - 1) // 32
            more = fetched < lines
            if more.any():
                low_water = min(low_water, int(unread[more].min()))   # (a lane whose last line is in the ring may drain it)
            can = more & (unread <= RING - BATCH)
            go = True if trigger == 0 else bool((more & (unread <= trigger)).any())
            took = int(can.sum()) if go else 0
            periods += 1
            refills += 1 if took else 0
            issued += took
            used = start + cum[:, (p + 1) * period - 1]
            if go:
                widx = widx + can * BATCH
                fetched = fetched + can
    return periods, refills, issued, low_water


def main():
    waves = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    symbols = int(sys.argv[2]) if len(sys.argv) > 2 else 1776
    print("period trigger  periods  with_refill  share  share_per_16  lanes_per_refill  low_water")
    for period, trigger in ((16, 0), (16, 13), (16, 12), (8, 0), (8, 7), (8, 8), (4, 0), (4, 5)):
        n, r, i, lw = run(period, trigger, waves, symbols - symbols % 16)
        print("%6d %7d %8d %12d  %.3f  %12.3f  %16.1f  %9d" % (period, trigger, n, r, r / n, r / n * 16 / period, i / max(r, 1), lw))


if __name__ == "__main__":
    main()
