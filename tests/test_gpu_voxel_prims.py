"""The voxelisation's hand-written device primitives on caller data (test hooks of the C ABI): the onesweep radix sort (32-bit keys, and
64-bit keys as two halves), the prefix scans and the single-pass leaf segmentation -- no vendor library is linked.  Bit-exact against numpy: a stable sort is unique, and so is the run-length structure of a sorted
array.  Sizes straddle the tile sizes: a sort tile and a segmentation tile hold 512 x items elements, items chosen by size (the sort: debug
switch sort_items; the segmentation: 2 up to 65 536 positions, 4 up to 262 144, 16 above); a scan tile holds 4096."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 4095, 4096, 8191, 8192, 8193, 16385, 100_003, 1_510_720]
# a sort tile holds 512 x items pairs, items = 2, 4, 8 or 16 (debug switch sort_items; tests/test_gpu_size_edges.py runs these comparisons once per value)
TILE_EDGES = [1023, 1024, 1025, 2047, 2048, 2049, 4097]


def _keys(rng, n, bits, kind):
    hi = (1 << bits) - 1 if bits < 32 else 0xFFFFFFFF
    if kind == "random":
        return rng.integers(0, hi + 1, n, dtype=np.uint64).astype(np.uint32)
    if kind == "equal":
        return np.full(n, hi // 3, np.uint32)
    if kind == "sorted":
        return np.sort(rng.integers(0, hi + 1, n, dtype=np.uint64).astype(np.uint32))
    if kind == "reverse":
        return np.sort(rng.integers(0, hi + 1, n, dtype=np.uint64).astype(np.uint32))[::-1].copy()
    if kind == "coherent":  # like leaf codes of a scan: long runs of equal upper digits, few distinct values
        base = rng.integers(0, max(1, hi >> 6) + 1, max(1, n // 500 + 1), dtype=np.uint64)
        k = (np.repeat(base, 500)[:n] << 6) | rng.integers(0, 64, n, dtype=np.uint64)
        return (k & hi).astype(np.uint32)
    raise ValueError(kind)


def _check_sort32(opts, n):
    """Every sort runs on each context of `opts` in turn, against one numpy reference."""
    rng = np.random.default_rng(n)
    cases = [(8, "random"), (17, "coherent"), (24, "random"), (32, "random")] if n > 100_000 else \
            [(b, k) for b in (1, 7, 8, 9, 16, 17, 24, 25, 32) for k in ("random", "equal", "sorted", "reverse", "coherent")]
    for bits, kind in cases:
        keys = _keys(rng, n, bits, kind)
        vals = rng.permutation(n).astype(np.uint32)
        order = np.argsort(keys, kind="stable")
        for i, opt in enumerate(opts):
            ks, vs = opt.sortPairs(keys, vals, bits)
            assert np.array_equal(ks, keys[order]), (n, bits, kind, i)
            assert np.array_equal(vs, vals[order]), (n, bits, kind, i)
    # bits above end_bit are ignored: sorting on the low byte only keeps the input order inside a bucket
    keys = _keys(rng, n, 32, "random")
    vals = np.arange(n, dtype=np.uint32)
    order = np.argsort(keys & 0xFF, kind="stable")
    for opt in opts:
        ks, vs = opt.sortPairs(keys, vals, 8)
        assert np.array_equal(ks, keys[order]) and np.array_equal(vs, order.astype(np.uint32))
    # ... also when end_bit is not a multiple of 8: the last pass must mask its digit (random bits above end_bit)
    for bits in (1, 5, 11, 17, 21, 27, 31):
        keys = _keys(rng, n, 32, "random")
        order = np.argsort(keys & np.uint32((1 << bits) - 1), kind="stable")
        for i, opt in enumerate(opts):
            ks, vs = opt.sortPairs(keys, vals, bits)
            assert np.array_equal(ks, keys[order]), (n, bits, i)
            assert np.array_equal(vs, order.astype(np.uint32)), (n, bits, i)


@pytest.mark.parametrize("n", SIZES + TILE_EDGES)
def test_radix_sort_is_the_stable_sort(hip, n):
    opt = hip.DmsaOptimizer()
    _check_sort32([opt], n)
    opt.close()


# the segmentation's tile frame and look-back (csrc/chained_scan.h): one tile +- 1 at 2 items; exactly 64 tiles (one full round of the look-back,
# every lane consumed) and the switch to 4 items behind it; 65 tiles of 2048 (a second round that consumes one lane); the switch 4 -> 16 items;
# 65 tiles of 8192
SEGMENT_EDGES = [1023, 1024, 1025, 65_535, 65_536, 65_537, 131_073, 262_144, 262_145, 524_289]


@pytest.mark.parametrize("n", SIZES + SEGMENT_EDGES)
def test_leaf_segments_match_run_lengths(hip, n):
    rng = np.random.default_rng(7 * n + 1)
    opt = hip.DmsaOptimizer()
    bits = 20
    invalid = np.uint32(1 << bits)
    for leaves_per_point, tail in ((0.1, 0), (1.0, 0), (0.001, 0), (0.1, min(n - 1, 37)), (0.1, n)):
        codes = np.sort(rng.integers(0, max(1, int(n * leaves_per_point)) + 1, n, dtype=np.uint64).astype(np.uint32))
        if tail:
            codes[n - tail:] = invalid  # non-finite points sort to the end and belong to no leaf
        of_pos, start = opt.leafSegments(codes, bits)
        valid = codes != invalid
        nv = int(valid.sum())
        if nv == 0:
            assert start.size == 1 or start.size == 0
            continue
        c = codes[:nv]
        head = np.ones(nv, bool)
        head[1:] = c[1:] != c[:-1]
        ref_of_pos = np.cumsum(head).astype(np.int32)
        ref_start = np.concatenate([np.flatnonzero(head), [nv]]).astype(np.int32)
        assert np.array_equal(of_pos[:nv], ref_of_pos)
        assert np.array_equal(start, ref_start)
    opt.close()


def _check_sort64(opts, n):
    rng = np.random.default_rng(3 * n + 5)
    for bits in (20, 32, 33, 40, 47, 63, 64):
        hi = (1 << bits) - 1
        keys = rng.integers(0, hi, n, dtype=np.uint64, endpoint=True)
        if n > 100:  # long runs of equal upper words, like leaf codes
            keys = (keys & np.uint64(0xFFFF_FFFF_FFFF_FFFF ^ 0x3FFF_FF00)) | (keys & np.uint64(0xFF))
        keys |= rng.integers(0, 1 << (64 - bits), n, dtype=np.uint64) << np.uint64(bits) if bits < 64 else np.uint64(0)  # bits above end_bit: ignored
        vals = rng.permutation(n).astype(np.uint32)
        order = np.argsort(keys & np.uint64(hi), kind="stable")
        for i, opt in enumerate(opts):
            ks, vs = opt.sortPairs64(keys, vals, bits)
            assert np.array_equal(ks, keys[order]), (n, bits, i)
            assert np.array_equal(vs, vals[order]), (n, bits, i)


@pytest.mark.parametrize("n", [1, 65, 8193, 100_003, 1_510_720, 1024, 1025, 2048, 2049, 4096, 4097, 8192])
def test_radix_sort_of_64_bit_keys_is_the_stable_sort(hip, n):
    """Leaf codes of trees deeper than ten levels: sorted as two stable 32-bit sorts that carry positions (csrc/radix_sort.hip)."""
    opt = hip.DmsaOptimizer()
    _check_sort64([opt], n)
    opt.close()


def test_sort_tile_size_belongs_to_the_context(hip):
    """Three contexts alive in one process -- 16 pairs per thread, 2, and the choice by size -- sort the same data in turn: a context's tile size
    is its own (debug switch sort_items), and the plan of a sort and its launches agree on it.  Sizes: one tile and one tile +- 1 at 2 and at
    16 pairs x 512 threads, and a size whose last tile is partial under both."""
    opts = [hip.DmsaOptimizer(debug={"sort_items": 16}), hip.DmsaOptimizer(debug={"sort_items": 2}), hip.DmsaOptimizer()]
    for n in (1023, 1024, 1025, 8191, 8192, 8193, 8193 + 1024):
        _check_sort32(opts, n)
        _check_sort64(opts, n)
    for opt in opts:
        opt.close()


@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 100_003, 64 * 4096, 64 * 4096 + 1, 3_021_440])
def test_prefix_scans(hip, n):
    """64 * 4096 (+ 1): 64 and 65 tiles, one full round of the look-back and a second one.  The hook promises int32, not counts: `signed` has
    negative entries, the running sum of `large` passes 2^30 and stays inside int32."""
    rng = np.random.default_rng(n)
    opt = hip.DmsaOptimizer()
    for kind in ("flags", "counts", "signed", "large"):
        if kind == "flags":
            x = (rng.random(n) < 0.3).astype(np.int32)
        elif kind == "counts":
            x = rng.integers(0, 700, n).astype(np.int32)
        elif kind == "signed":
            x = rng.integers(-700, 700, n).astype(np.int32)
        else:
            hi = (2**31 - 1) // n
            x = rng.integers(hi - hi // 4, hi, n, endpoint=True).astype(np.int32)
            assert 2**30 < int(x.sum(dtype=np.int64)) < 2**31
        incl = np.cumsum(x, dtype=np.int64).astype(np.int32)
        assert np.array_equal(opt.scan(x, True), incl), (n, kind)
        assert np.array_equal(opt.scan(x, False), incl - x), (n, kind)
    opt.close()
