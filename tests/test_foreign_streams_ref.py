"""tests/foreign_streams.py against the CPU oracle: decode() is the oracle's int16 zig-zag decode of streams with any codes, and the
catalogue holds what tests/test_gpu_foreign_streams.py relies on -- counted here, from the oracle and numpy alone, so the device tests
cannot shrink unnoticed."""
import numpy as np
import pytest

import foreign_streams as F
import oracle_lib as O

E_STREAM = 0xFFFFFFFB
L0 = O.options(True, 2, 0, 1)


@pytest.fixture(scope="module")
def rows():
    return F.catalogue(np.random.default_rng(61))


def oracle(stream, n):
    return O.decompress(stream, 2 * n, L0)


def same(stream, n):
    want, got = oracle(stream, n), F.decode(stream, n)
    if isinstance(want, int):
        assert want == E_STREAM and got is None, (hex(want), got is None)
        return False
    assert got is not None and got[0].tobytes() == want.tobytes(), (n, int(np.argmax(got[0].view(np.uint8) != want)) // 2 if got is not None else None)
    return True


def test_constants_are_the_kernels():
    assert F.BUF == 2 * F.T * 3 // 2 + 48 == 6192 and F.SEG_TILES == 8, (F.BUF, F.SEG_TILES)


def test_decode_is_the_oracle_on_every_row(rows):
    errors = [r.name for r in rows if not same(r.stream, r.n)]
    # the oracle decodes all rows but the "without bytes" and "byte missing" ones
    assert errors == [r.name for r in rows if "error" in r.tags], errors
    assert len(errors) == 4 and sum("without bytes" in r.tags for r in rows) == 2 and sum("byte missing" in r.tags for r in rows) == 2
    for r in rows:
        assert r.n <= 40_000, (r.name, r.n)
        if "intact" in r.tags or "buf" in r.tags or "noise" in r.tags:
            assert len(F.wide_values(r.stream, r.n)) == 0, r.name


def test_decode_is_the_oracle_on_random_control_bytes():
    rng = np.random.default_rng(67)
    sizes = [1, 2, 7, 8, 9, 31, 32, 33, 9000] + rng.integers(1, 9001, 91).tolist()
    assert len(sizes) == 100
    for n in sizes:
        assert same(F.random_stream(rng, n), n), n


def test_intact_rows_are_the_reads_the_oracle_compressed():
    rng = np.random.default_rng(5)
    for kind in F.KINDS:
        x = F.KINDS[kind](rng, 3 * F.T + 5)
        got = F.decode(F.compress(x), len(x))
        assert got is not None and np.array_equal(got[0], x), kind


def test_wide_codes_where_the_mask_is_off(rows):
    """at least 8 rows hold a wide code in the reference's scalar tail, and there the 16-bit mask would change the output"""
    off = []
    for r in rows:
        got = F.decode(r.stream, r.n)
        if got is None:
            continue
        wide = F.wide_values(r.stream, r.n)
        if len(wide) and not got[1][wide].all():
            masked = F.decode(r.stream, r.n, body=True)[0]
            assert not np.array_equal(masked, got[0]), r.name
            off.append(r.name)
    assert len(off) >= 8, off


def test_wide_codes_where_the_body_predicates_disagree(rows):
    """at least 2 rows hold a wide code whose group of eight is a whole one in front of the last (the index says body) with fewer than
    32 data bytes left where it begins (the byte count says tail)"""
    found = []
    for r in rows:
        if "error" in r.tags:
            continue
        _, off, _, present = F.layout(r.stream, r.n)
        for v in F.wide_values(r.stream, r.n):
            by_index = (v >> 3) < (r.n >> 3)
            by_bytes = present - off[(v >> 3) << 3] >= 32
            if by_index != by_bytes:
                found.append(r.name)
    assert len(set(found)) >= 2, found
    assert set(found) >= {r.name for r in rows if "last groups" in r.tags}, found


def test_where_the_pair_loop_hands_over(rows):
    exits = {r.name: F.pair_exit(r.stream, r.n, 0) for r in rows}
    whole = {r.name: r.n // F.P for r in rows}
    at = {e[0] for e in exits.values() if e is not None}
    assert 0 in at and 1 in at and any(p >= 3 for p in at), sorted(at)
    assert any(e is not None and e[0] == whole[name] - 1 for name, e in exits.items()), "no exit at a last whole pair"
    assert any(e is None for e in exits.values())
    for reason in (F.WIDE, F.SHORT, F.OVER):
        assert sum(e is not None and e[1] == reason for e in exits.values()) >= 2, reason
    for r in rows:
        if "intact" in r.tags:
            assert exits[r.name] is None, (r.name, exits[r.name])
        if "byte missing" in r.tags:   # met while the final pair is planned
            assert exits[r.name] == (r.n // F.P - 1, F.SHORT), (r.name, exits[r.name])
    want = {"noise fills pair 0": (0, F.OVER), "noise fills pair 1": (1, F.OVER), "noise fills pair 3": (3, F.OVER),
            "noise fills the last whole pair": (2, F.OVER), "a pair half noise fits": None}
    assert {k: exits[k] for k in want} == want


@pytest.mark.parametrize("addr16", [0, 1, 7, 15])
def test_limit_rows_lie_on_either_side_of_the_buffer_limit(addr16):
    rows = F.catalogue(np.random.default_rng(61), addr16)
    fits, over = [r for r in rows if "fits" in r.tags], [r for r in rows if "over" in r.tags]
    assert len(fits) == len(over) == 1
    for r, want in ((fits[0], None), (over[0], (1, F.OVER))):
        _, off, _, _ = F.layout(r.stream, r.n)
        size = int(off[2 * F.P] - off[F.P])
        mis = (addr16 + (r.n + 3) // 4 + int(off[F.P])) % 16
        assert mis + size + 16 == F.BUF + (0 if want is None else 1), (r.name, mis, size)
        assert F.pair_exit(r.stream, r.n, addr16) == want, r.name


def test_ranges_and_segments_start_where_their_first_value_lies(rows):
    """pair_exit over a segment of the large-read path: the wide code at value 20 003 ends the second segment's loop at its first pair,
    and no other segment's"""
    r = next(r for r in rows if r.name == "three segments, code 3 at value 20 003")
    got = [F.pair_exit(r.stream, r.n, 0, k * F.SEG, min(r.n, (k + 1) * F.SEG)) for k in range(3)]
    assert got == [None, (0, F.WIDE), None], got
    assert F.pair_exit(r.stream, r.n, 0) == (20_003 // F.P, F.WIDE)


def test_size_of_the_catalogue(rows):
    total = sum(r.n for r in rows)
    print(len(rows), "rows,", total, "samples")
    assert len(rows) >= 48 and total <= 1_200_000, (len(rows), total)
    assert sum("wide" in r.tags and "error" not in r.tags for r in rows) >= 2 * (11 + 3) + 2
