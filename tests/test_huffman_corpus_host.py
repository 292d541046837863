"""The serial host statement of the Huffman table construction (zstd_entropy.h: huf_build_pm, huf_write_tree -- what the device's
wave-parallel builders must reproduce byte for byte, tests/test_gpu_huffman_tables.py) on the adversarial histograms of
tests/huffman_corpus.py: exact optimality under the length limit, both readers of the tree description, libzstd's construction as the
yardstick, and the conditions the corpus itself has to meet so that no side exit goes untested."""
import collections
import ctypes
import heapq

import numpy as np
import pytest

import entropy_host as E
import huffman_corpus as C


def optimum_cost(counts, limit):
    """The cost in bits of an optimal prefix code for the positive integer weights `counts` with no word longer than `limit`:
    package-merge (Larmore & Hirschberg) over Python integers.  Every level's list is the leaves merged with the pairs of the level below;
    the 2n - 2 lightest items of the last level are the solution and their weights add up to sum(count x length)."""
    leaves = sorted(int(c) for c in counts)
    n = len(leaves)
    assert n >= 2 and (1 << limit) >= n
    level = leaves
    for _ in range(limit - 1):
        level = sorted(leaves + [level[i] + level[i + 1] for i in range(0, len(level) - 1, 2)])
    return sum(level[: 2 * n - 2])


def huffman_cost(counts):
    """the cost of an unlimited Huffman code: the sum of all merged weights"""
    heap = [int(c) for c in counts]
    heapq.heapify(heap)
    total = 0
    while len(heap) > 1:
        s = heapq.heappop(heap) + heapq.heappop(heap)
        total += s
        heapq.heappush(heap, s)
    return total


def _limit(h):
    return E.lib().h_optimal_table_log(11, min(int(h.sum()), 128 << 10), int(np.flatnonzero(h).max()), 1)


def _build(fn, h, limit):
    u8p, u16p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint32)
    cnt = np.ascontiguousarray(h, np.uint32)
    nb, code = np.zeros(256, np.uint8), np.zeros(256, np.uint16)
    tl = fn(cnt.ctypes.data_as(u32p), int(np.flatnonzero(h).max()), limit, nb.ctypes.data_as(u8p), code.ctypes.data_as(u16p))
    return tl, nb, code


def _coded():
    """the regions with two values or more: every one a table can be asked for"""
    return [r for r in C.regions() if np.count_nonzero(r.counts) >= 2]


@pytest.fixture(scope="module")
def facts():
    """per region: limit, table log, lengths, tree description, the way through the tree writer, exact optimum, unlimited optimum"""
    out = {}
    for r in _coded():
        limit = _limit(r.counts)
        tl, nb, tree = E.tree_description_counts(r.counts, package_merge=True)
        present = r.counts[r.counts > 0]
        out[r.name] = dict(limit=limit, tl=tl, nb=nb, tree=tree, report=E.weights_report(nb, int(np.flatnonzero(r.counts).max()), tl),
                           optimum=optimum_cost(present, limit), unlimited=huffman_cost(present))
    return out


def test_package_merge_is_the_exact_optimum_on_the_corpus(facts):
    """huf_build_pm at the limit optimal_table_log gives, against the package-merge over Python integers above: the same cost, a
    complete prefix-free canonical code, table log == longest word <= limit, a word for exactly the values that occur."""
    H = E.lib()
    for r in _coded():
        f = facts[r.name]
        limit = f["limit"]
        tl, nb, code = _build(H.h_huf_build_pm, r.counts, limit)
        assert (nb == f["nb"]).all() and tl == f["tl"], r.name
        assert ((nb > 0) == (r.counts > 0)).all(), r.name
        assert tl == nb.max() <= limit, (r.name, tl, limit)
        assert sum(1 << (limit - int(x)) for x in nb if x) == 1 << limit, r.name
        words = sorted(format(int(code[s]), "0%db" % nb[s]) for s in range(256) if nb[s])
        assert all(not b.startswith(a) for a, b in zip(words, words[1:])), r.name
        cost = int((r.counts * nb.astype(np.int64)).sum())
        assert cost == f["optimum"], (r.name, limit, cost, f["optimum"])
        assert cost >= f["unlimited"], r.name


def test_package_merge_never_longer_than_libzstd_on_the_corpus(facts):
    """the same histogram and limit through libzstd's construction (Huffman tree + HUF_setMaxHeight): never cheaper"""
    H = E.lib()
    longer = 0
    for r in _coded():
        f = facts[r.name]
        tl, nb, _ = _build(H.h_huf_build, r.counts, f["limit"])
        z = int((r.counts * nb.astype(np.int64)).sum())
        assert f["optimum"] <= z, (r.name, f["optimum"], z)
        longer += z > f["optimum"]
    assert longer >= 3   # (the limit binds hard on the Fibonacci counts: libzstd's repair is not optimal there)


def test_both_readers_give_the_lengths_back(facts):
    """The tree description read by the decoders' reader (zstd_tables.h: huf_read_weights) and by the test suite's own
    (entropy_host.weights_from_tree): the statement's lengths, all of the description used."""
    read = 0
    for r in _coded():
        f = facts[r.name]
        if f["tree"] is None:
            assert f["report"][1] == "none", r.name
            continue
        assert f["report"][1] == ("direct" if f["tree"][0] >= 128 else "fse") and f["report"][3] == len(f["tree"]), r.name
        used, log, w = E.huf_read_weights(f["tree"], 11)
        assert used == len(f["tree"]) and log == f["tl"], (r.name, used, log)
        lengths = np.zeros(256, np.uint8)
        lengths[: len(w)] = [log + 1 - int(x) if x else 0 for x in w]
        assert (lengths == f["nb"]).all(), r.name
        assert (E.weights_from_tree(f["tree"]) == f["nb"]).all(), r.name
        read += 1
    assert read >= 60


def test_the_corpus_reaches_every_exit(facts):
    """Conditions on the corpus, not measurements: each must hold or the device tests above it compare less than they claim."""
    R = {r.name: r for r in C.regions()}
    kinds = collections.Counter(f["report"][1] for f in facts.values())
    assert kinds["direct"] >= 3 and kinds["fse"] >= 40 and kinds["none"] >= 3, kinds
    # the four exits of huf_write_tree_wave to the serial writer
    weights = {name: [f["tl"] + 1 - int(x) if x else 0 for x in f["nb"][: int(np.flatnonzero(R[name].counts).max())]] for name, f in facts.items()}
    all_equal = [n for n, f in facts.items() if f["report"][0] == 0 and len(weights[n]) > 1 and len(set(weights[n])) == 1]
    each_once = [n for n, f in facts.items() if f["report"][0] == 0 and len(weights[n]) > 1 and len(set(weights[n])) == len(weights[n])]
    second = [n for n, f in facts.items() if f["report"][0] == 2]
    no_pay = [n for n, f in facts.items() if f["report"][0] in (1, 2) and f["report"][1] != "fse"]
    assert len(all_equal) >= 3 and len(each_once) >= 2 and len(second) >= 3 and len(no_pay) >= 1, (all_equal, each_once, second, no_pay)
    assert {facts[n]["report"][1] for n in all_equal} == {"direct", "none"} and {facts[n]["report"][1] for n in each_once} == {"direct"}
    assert {facts[n]["report"][1] for n in no_pay} == {"direct"}   # (above 128 symbols no description was found that does not pay)
    assert len(facts["equal_64"]["tree"]) == 33 and len(facts["equal_128"]["tree"]) == 65
    assert sum(f["report"][2] > 0 for f in facts.values()) >= 10   # low-probability weights
    # the limit binds (the unlimited optimum is out of reach) at every limit value that occurs
    limits = sorted(set(f["limit"] for f in facts.values()))
    binding = sorted(set(f["limit"] for f in facts.values() if f["optimum"] > f["unlimited"]))
    assert limits == binding and limits[0] == 5 and limits[-1] == 11, (limits, binding)
    assert facts["fibonacci_21"]["limit"] == 11 and facts["fibonacci_16"]["limit"] == 10 and facts["fibonacci_12"]["limit"] == 7
    # alphabet sizes, and full-length codes over the full alphabet
    sizes = set(int(np.count_nonzero(r.counts)) for r in C.regions())
    assert {1, 2, 3, 128, 129, 255, 256} <= sizes, sorted(sizes)
    assert any(f["tl"] == 11 and np.count_nonzero(R[n].counts) == 256 for n, f in facts.items())
    # region_plan's rules, both sides
    rule = {(int(r.counts.max()) - ((len(r.data) >> 7) + 4)) for r in C.regions() if r.family == "small"}
    assert {0, 1} <= rule
    assert C.plan_estimate(R["small600_just_paying"].counts)[0] == "huffman"
    mode, est = C.plan_estimate(R["small600_just_not_paying"].counts)
    assert mode == "raw" and est is not None
    assert len(R["small63"].data) == 63 and {64, 65, 300, 600} <= set(len(r.data) for r in C.regions() if r.family == "small")
    # what may be compared bit for bit is never sampled; no arrangement has a run the tokeniser would take, but where none exists
    for r in C.regions():
        assert r.sampled == (len(r.data) >= C.SAMPLE_FROM and np.count_nonzero(r.counts) >= C.SAMPLE_SEEN)
        assert r.sampled == (r.family == "sampled"), r.name
        no_way = int(r.counts.max()) > (C.RMIN - 1) * (len(r.data) - int(r.counts.max()) + 1)   # more than 11 to every gap
        assert r.runs == (r.family == "zeros" or no_way), (r.name, C.longest_run(r.data))
        if r.family not in ("few", "zeros"):
            assert 4 * r.counts[0] <= len(r.data), r.name
    assert sum(r.sampled for r in C.regions()) >= 3 and sum(r.family == "zeros" for r in C.regions()) == 3
    assert sum(r.family == "random" for r in C.regions()) == 40

