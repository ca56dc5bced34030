"""CPU-side checks of include/dmsa_dense_carve.h: the model's walk (tests/dense_carve_model.py, the yardstick of the GPU tests) against exact
geometry in rationals, the two host-only calls against the model cell for cell and bit for bit, and the symbols, structs, defaults and the
refusals that need no device.

(a) Exact geometry.  In the doubled fixed-point units of T3 both ends of a ray are odd integers and cell planes lie at multiples of 2^11.  A
cell is traversed iff its OPEN box meets the segment: per axis the open interval of the segment's parameter t inside the cell's slab is
computed with fractions.Fraction, and the three are intersected with [0, 1].  A segment through a cell edge or corner touches the cells
diagonally across it only in that point, so they are not traversed: the tie rule of T4 decides exactly these cases."""
import ctypes as C
import itertools
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from dmsa_lidar_slam_amd import _capi as capi
from dmsa_lidar_slam_amd import dense_cloud as dcl

import dense_carve_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
W = 2048


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


# ---- the rays ----------------------------------------------------------------------------------------------------------------------------------
def _fixed(v, cell_size):
    return 2 * int(math.floor(np.float64(f32(v)) / np.float64(f32(cell_size)) * 1024.0)) + 1


def _rays():
    """(cell_size, o, g, tag) of every ray of (a) and (b)."""
    rng = np.random.default_rng(3)
    rays = []
    for cell in (0.2, 1.0, 0.37):  # 2 100 random rays of up to four cells per axis
        for _ in range(700):
            o = rng.uniform(-3, 3, 3) * cell
            rays.append((cell, o, o + rng.uniform(-1, 1, 3) * rng.choice([0.3, 1.5, 4.0]) * cell, "random"))
    for _ in range(40):  # long and thin
        o = rng.uniform(-2, 2, 3)
        g = o + rng.uniform(-0.4, 0.4, 3)
        g[rng.integers(3)] += rng.choice([-1, 1]) * rng.uniform(5, 12)
        rays.append((0.2, o, g, "long"))
    for axis in range(3):  # axis-parallel, both directions, also along a cell plane's neighbourhood
        for sign in (-1.0, 1.0):
            for off in (0.5, 0.0, 0.999):
                o = np.array([off, off, off])
                g = o.copy()
                g[axis] += sign * 5.3
                rays.append((1.0, o, g, "axis"))
    for _ in range(30):  # inside one cell
        o = np.floor(rng.uniform(-4, 4, 3)) + rng.uniform(0.05, 0.95, 3)
        rays.append((1.0, o, np.floor(o) + rng.uniform(0.05, 0.95, 3), "one cell"))
    for signs in itertools.product((-1.0, 1.0), repeat=3):  # the eight octants, from both sides of the origin
        s = np.array(signs)
        rays.append((0.2, -0.13 * s, s * np.array([0.71, 0.52, 0.93]), "octant"))
        rays.append((0.2, s * np.array([0.31, 0.12, 0.23]), s * np.array([1.71, 1.52, 0.93]), "octant"))
    # through cell edges and corners: with cell_size 1 a coordinate k / 1024 has F = k, and F = k and F = -(k + 1) mirror each other about the plane
    # at 0, so equal coordinates on two (three) axes cross their planes at the same parameter at every crossing
    def v(k):
        return k / 1024.0

    for a, b in ((5, 2047 + 2048), (-(5 + 1), 3000), (700, -(4000 + 1)), (-(100 + 1), -(6000 + 1)), (1023, 1024), (0, 2048 * 3 + 17)):
        rays.append((1.0, np.array([v(a), v(a), v(33)]), np.array([v(b), v(b), v(40)]), "edge"))           # x and y tie, z does not move a cell
        rays.append((1.0, np.array([v(33), v(a), v(a)]), np.array([v(4000), v(b), v(b)]), "edge"))        # y and z tie, x crosses on its own
        rays.append((1.0, np.array([v(a), v(a), v(a)]), np.array([v(b), v(b), v(b)]), "corner"))         # all three tie
        rays.append((1.0, np.array([v(a), v(-(a + 1)), v(a)]), np.array([v(b), v(-(b + 1)), v(b)]), "corner"))  # ... in mirrored directions
    # an edge hit once, between crossings of single planes: X runs from (1, 1) to (4 W - 1, 2 W - 1), so x crosses W and 3 W alone and 2 W together
    # with y's W, at t = 1 / 2
    rays.append((1.0, np.array([v(0), v(0), v(7)]), np.array([v(4095), v(2047), v(9)]), "edge"))
    return rays


RAYS = _rays()


def _exact_cells(cell_size, o, g):
    """The cells of the bounding box whose open box meets the segment, by rationals."""
    a = [_fixed(o[k], cell_size) for k in range(3)]
    b = [_fixed(g[k], cell_size) for k in range(3)]
    spans = []
    for k in range(3):
        lo, hi = sorted((a[k] // W, b[k] // W))
        inside = {}
        for c in range(lo, hi + 1):
            if a[k] == b[k]:
                inside[c] = (Fraction(-1), Fraction(2)) if c * W < a[k] < (c + 1) * W else None
            else:
                t0, t1 = sorted((Fraction(c * W - a[k], b[k] - a[k]), Fraction((c + 1) * W - a[k], b[k] - a[k])))
                inside[c] = (t0, t1)
        spans.append(inside)
    cells = set()
    for cx, ix in spans[0].items():
        for cy, iy in spans[1].items():
            for cz, iz in spans[2].items():
                if ix is None or iy is None or iz is None:
                    continue
                t0, t1 = max(ix[0], iy[0], iz[0]), min(ix[1], iy[1], iz[1])
                if t0 < t1 and t0 < 1 and t1 > 0:  # the open interval (t0, t1) meets [0, 1]
                    cells.add((cx, cy, cz))
    return cells


# ---- (a) the model's walk against exact geometry ---------------------------------------------------------------------------------------------
def test_model_walk_equals_the_cells_whose_open_box_meets_the_segment():
    ties = 0
    tags = set()
    for cell_size, o, g, tag in RAYS:
        o, g = o.astype(f32), g.astype(f32)
        path = cm.walk(cell_size, o, g)
        assert path is not None, (tag, o, g)
        assert len(set(path)) == len(path) and set(path) == _exact_cells(cell_size, o, g), (tag, o, g)
        assert path[0] == cm.cell_of(o, cell_size) and path[-1] == cm.cell_of(g, cell_size)
        steps = [sum(abs(p[k] - q[k]) for k in range(3)) for p, q in zip(path, path[1:])]
        assert all(max(abs(p[k] - q[k]) for k in range(3)) == 1 for p, q in zip(path, path[1:])), (tag, o, g)  # consecutive cells are neighbours
        ties += sum(1 for s in steps if s > 1)
        if tag in ("edge", "corner"):
            assert any(s == (3 if tag == "corner" else 2) for s in steps), (tag, o, g, path)
        if tag == "one cell":
            assert len(path) == 1
        tags.add(tag)
    assert sum(1 for r in RAYS if r[3] == "random") >= 2000 and tags == {"random", "long", "axis", "one cell", "octant", "edge", "corner"} and ties > 30


# ---- (b) dmsa_dense_carve_walk against the model -------------------------------------------------------------------------------------------------
def test_host_walk_equals_the_model_cell_for_cell():
    for cell_size, o, g, tag in RAYS:
        o, g = o.astype(f32), g.astype(f32)
        got = dcl.carve_walk(cell_size, o, g)
        want = cm.walk(cell_size, o, g)
        assert got is not None and got.dtype == np.int32 and [tuple(int(v) for v in c) for c in got] == want, (tag, o, g)


def test_host_walk_skips_what_t2_skips_and_walks_the_largest_extent(lib):
    half = np.array([0.5, 0.5, 0.5], f32)
    # L2 == 0
    assert cm.walk(1.0, half, half) is None and dcl.carve_walk(1.0, half, half) is None
    tiny, tinier = np.array([2e-30, 0, 0], f32), np.array([1e-30, 0, 0], f32)  # d * d underflows: L2 == 0 although the ends differ
    assert cm.walk(1.0, tinier, tiny) is None and dcl.carve_walk(1.0, tinier, tiny) is None
    # an extent of exactly 2^11 cells is walked, of 2^11 + 1 is not, on every axis and in both directions
    for axis in range(3):
        for sign in (-1.0, 1.0):
            g = half.copy()
            g[axis] += f32(sign * 2048.0)
            want = cm.walk(1.0, half, g)
            got = dcl.carve_walk(1.0, half, g)
            assert len(want) == 2049 and [tuple(int(v) for v in c) for c in got] == want
            g[axis] += f32(sign)
            assert cm.walk(1.0, half, g) is None and dcl.carve_walk(1.0, half, g) is None
    # the longest walk there is: 2^11 planes on each axis, never two at once
    o, g = np.array([0.1, 0.3, 0.7], f32), np.array([2048.9, 2048.2, 2048.4], f32)
    want = cm.walk(1.0, o, g)
    assert len(want) == 3 * 2048 + 1 and [tuple(int(v) for v in c) for c in dcl.carve_walk(1.0, o, g)] == want
    # an end beyond cell 2^31, and ends that are not finite
    for bad in (3e9, -3e9, np.inf, -np.inf, np.nan):
        g = half.copy()
        g[1] = bad
        assert cm.walk(1.0, half, g) is None and dcl.carve_walk(1.0, half, g) is None and dcl.carve_walk(1.0, g, half) is None
    assert cm.walk(1.0, half + f32(2.1e9), half + f32(2.1e9) + f32(512.0)) is not None  # (just inside)
    # the length limit is T2's second case: the model with a limit, the pair test on the host
    far = half + np.array([40.0, 0, 0], f32)
    assert cm.walk(1.0, half, far, max_length=30.0) is None and len(cm.walk(1.0, half, far, max_length=40.0)) == 41
    cfg = cm.Config(max_length=30.0)
    p = half + np.array([20.0, 0, 0], f32)
    assert not cm.sees_through(cfg, half, far, p) and not dcl.carve_sees_through(dcl.DenseCarveConfig(max_length=30.0), half, far, p)
    assert cm.sees_through(cm.Config(max_length=40.0), half, far, p) and dcl.carve_sees_through(dcl.DenseCarveConfig(max_length=40.0), half, far, p)
    # a short output buffer gets the first cells and the full count
    n, few = C.c_int64(0), np.full((2, 3), -7, np.int32)
    assert lib.dmsa_dense_carve_walk(1.0, capi.ptr(half, C.c_float), capi.ptr(far, C.c_float), capi.ptr(few, C.c_int32), 2, C.byref(n)) == capi.DMSA_OK
    assert n.value == 41 and few.tolist() == [[0, 0, 0], [1, 0, 0]]


def test_hash_is_the_stated_chain():
    assert cm.hash_of([]) == 0xCBF29CE484222325
    h = 0xCBF29CE484222325
    for v in (0 + 2**20, -1 + 2**20, 5 + 2**20):
        h = ((h ^ v) * 0x100000001B3) % 2**64
    assert cm.hash_of([(0, -1, 5)]) == h and cm.hash_of([(0, -1, 5), (1, -1, 5)]) != cm.hash_of([(1, -1, 5), (0, -1, 5)])
    assert cm.hash_of([(-(2**20) - 1, 0, 0)]) == cm.hash_of([(2**64 - 2**20 - 1, 0, 0)])  # a cell below the bias wraps modulo 2^64


# ---- (c) dmsa_dense_carve_sees_through against the model ----------------------------------------------------------------------------------------
def _as_c(cfg):
    return dcl.DenseCarveConfig(cfg.cell_size, cfg.rho, cfg.tan_half_angle, cfg.end_margin, cfg.start_margin, cfg.max_length, cfg.min_passes)


def _both(cfg, o, g, p):
    got, want = dcl.carve_sees_through(_as_c(cfg), o, g, p), cm.sees_through(cfg, o, g, p)
    assert got == want, (cfg, o, g, p)
    return want


def test_pair_test_equals_the_model_on_random_rays_and_points():
    rng = np.random.default_rng(5)
    seen = 0
    for i in range(3000):
        o = rng.uniform(-5, 5, 3).astype(f32)
        g = (o + rng.normal(0, 4, 3)).astype(f32)
        t = rng.uniform(-0.1, 1.1)
        p = (o + t * (g - o) + rng.normal(0, rng.choice([0.005, 0.05, 0.2]), 3)).astype(f32)
        cfg = cm.Config(tan_half_angle=float(rng.choice([0.052407779, 0.2, 1.0])), max_length=float(rng.choice([30.0, 5.0])))
        seen += _both(cfg, o, g, p)
    assert 300 < seen < 2700


def test_rows_at_once_equal_the_scalar_pair_test():
    rng = np.random.default_rng(6)
    cfg = cm.Config(tan_half_angle=0.2)
    o, g = np.array([0.5, -1.0, 0.3], f32), np.array([7.1, 2.2, 1.4], f32)
    pts = (o + rng.uniform(0, 1, (4000, 1)) * (g - o) + rng.normal(0, 0.06, (4000, 3))).astype(f32)
    d, _, length = cm.ray(o, g)
    many = cm._sees_through_rows(cfg, d, length, g, pts)
    assert many.tolist() == [cm.sees_through(cfg, o, g, p) for p in pts] and 400 < many.sum() < 3600


def test_each_comparison_at_equality_and_one_ulp_to_either_side():
    o, g = np.zeros(3, f32), np.array([8.0, 0.0, 0.0], f32)  # d = (8, 0, 0), L = 8: every term below is exact
    up, down = (lambda v: float(np.nextafter(f32(v), f32(np.inf)))), (lambda v: float(np.nextafter(f32(v), f32(-np.inf))))
    wide = dict(rho=4.0, tan_half_angle=1.0, end_margin=0.125, start_margin=0.0)
    # s >= start_margin: p at x = 0.5 has s = 0.5
    p = np.array([0.5, 0.25, 0.0], f32)
    t = cm.pair_terms(o, g, p)
    assert (t["L"], t["rem"], t["perp2"], t["s"]) == (8.0, 7.5, 0.0625, 0.5)
    assert _both(cm.Config(**{**wide, "start_margin": 0.5}), o, g, p) and _both(cm.Config(**{**wide, "start_margin": down(0.5)}), o, g, p)
    assert not _both(cm.Config(**{**wide, "start_margin": up(0.5)}), o, g, p)
    # rem >= end_margin: p at x = 7.5 has rem = 0.5
    p = np.array([7.5, 0.25, 0.0], f32)
    t = cm.pair_terms(o, g, p)
    assert (t["rem"], t["perp2"], t["s"]) == (0.5, 0.0625, 7.5)
    assert _both(cm.Config(**{**wide, "end_margin": 0.5}), o, g, p) and _both(cm.Config(**{**wide, "end_margin": down(0.5)}), o, g, p)
    assert not _both(cm.Config(**{**wide, "end_margin": up(0.5)}), o, g, p)
    # perp2 <= rho * rho: 0.0625 = 0.25^2
    assert _both(cm.Config(**{**wide, "rho": 0.25}), o, g, p) and _both(cm.Config(**{**wide, "rho": up(0.25)}), o, g, p)
    assert not _both(cm.Config(**{**wide, "rho": down(0.25)}), o, g, p)
    # perp2 <= w * w: rem = 0.5, tan = 0.5 gives w = 0.25
    assert _both(cm.Config(**{**wide, "tan_half_angle": 0.5}), o, g, p) and _both(cm.Config(**{**wide, "tan_half_angle": up(0.5)}), o, g, p)
    assert not _both(cm.Config(**{**wide, "tan_half_angle": down(0.5)}), o, g, p)
    # the point one ulp to either side instead of the bound
    tight = cm.Config(rho=0.25, tan_half_angle=0.5, end_margin=0.5, start_margin=0.0)
    assert _both(tight, o, g, p)  # all four at equality at once
    for q in (np.array([up(7.5), 0.25, 0.0], f32), np.array([down(7.5), 0.25, 0.0], f32), np.array([7.5, up(0.25), 0.0], f32), np.array([7.5, down(0.25), 0.0], f32)):
        _both(tight, o, g, q)
    assert not cm.sees_through(tight, o, g, [up(7.5), 0.25, 0.0])  # rem = 8 - x is exact: one ulp below end_margin


def test_nans_fail_every_comparison():
    cfg = cm.Config(rho=4.0, tan_half_angle=1.0, end_margin=0.125, start_margin=0.0)
    o, g, p = np.zeros(3, f32), np.array([8.0, 0.0, 0.0], f32), np.array([4.0, 0.25, 0.0], f32)
    assert _both(cfg, o, g, p)
    for which in range(3):
        for k in range(3):
            for bad in (np.nan, np.inf, -np.inf):
                v = [o.copy(), g.copy(), p.copy()]
                v[which][k] = bad
                assert not _both(cfg, *v)
    assert not _both(cfg, o, o, p)  # L2 == 0


# ---- (d) exports, defaults, refusals ---------------------------------------------------------------------------------------------------------
def test_symbol_tuple_equals_the_header_and_the_library_exports_it(lib):
    header = open(os.path.join(ROOT, "include", "dmsa_dense_carve.h")).read()
    declared = set(re.findall(r"\b(dmsa_[a-z_0-9]+)\s*\(", header))
    assert declared == set(capi.DENSE_CARVE_SYMBOLS) and len(capi.DENSE_CARVE_SYMBOLS) == len(declared) == 6
    assert not declared & (set(capi.EXPORTED_SYMBOLS) | set(capi.DENSE_CLOUD_SYMBOLS) | set(capi.DENSE_NORMALS_SYMBOLS) | set(capi.DENSE_OUTLIERS_SYMBOLS))
    for name in declared:
        assert hasattr(lib, name), name
    for rule in ("T1", "T2", "T3", "T4", "T5", "T6", "T7"):
        assert re.search(rf"\b{rule}\b", header)


def test_struct_layouts_and_defaults(lib):
    names = ("cell_size", "rho", "tan_half_angle", "end_margin", "start_margin", "max_length", "min_passes", "pad")
    assert C.sizeof(capi.DenseCarveConfig) == 32 and [getattr(capi.DenseCarveConfig, n).offset for n in names] == list(range(0, 32, 4))
    assert C.sizeof(capi.DenseCarveStats) == 64 and dcl.CARVE_STAT_NAMES == cm.STAT_NAMES
    c = capi.DenseCarveConfig()
    C.memset(C.byref(c), 0x5A, C.sizeof(c))
    lib.dmsa_default_dense_carve_config(C.byref(c))
    want = [float(f32(v)) for v in (0.2, 0.1, 0.052407779, 0.3, 0.5, 30.0)] + [2, 0]
    assert [getattr(c, n) for n in names] == want
    assert f32(0.052407779) == f32(math.tan(math.radians(3.0)))  # the literal is the float nearest tan 3 deg
    lib.dmsa_default_dense_carve_config(None)
    py, model = dcl.DenseCarveConfig().to_c(), cm.Config()
    assert [getattr(py, n) for n in names] == want and [float(f32(getattr(model, n))) for n in names[:6]] + [model.min_passes, 0] == want


def test_every_refusal_that_needs_no_device(lib):
    from dmsa_lidar_slam_amd.api import DmsaError

    o, g, p = np.zeros(3, f32), np.array([8.0, 0.0, 0.0], f32), np.array([4.0, 0.01, 0.0], f32)
    assert dcl.carve_sees_through(None, o, g, p)
    bad = [dict(rho=0.0), dict(rho=-1.0), dict(rho=np.nan), dict(rho=np.inf), dict(end_margin=0.0), dict(end_margin=-0.1), dict(end_margin=np.inf),
           dict(start_margin=-0.1), dict(start_margin=np.nan), dict(start_margin=np.inf), dict(max_length=0.0), dict(max_length=np.inf), dict(max_length=np.nan),
           dict(tan_half_angle=0.0), dict(tan_half_angle=float(np.nextafter(f32(1.0), f32(2.0)))), dict(tan_half_angle=np.nan), dict(tan_half_angle=-0.5),
           dict(min_passes=0), dict(min_passes=2**20 + 1), dict(min_passes=-1)]
    for kw in bad:
        assert cm.Config(**kw).refused(), kw
        with pytest.raises(DmsaError):
            dcl.carve_sees_through(dcl.DenseCarveConfig(**kw), o, g, p)
    for kw in (dict(start_margin=0.0), dict(tan_half_angle=1.0), dict(min_passes=1), dict(min_passes=2**20), dict(cell_size=np.nan)):  # the bounds are legal; cell_size is not looked at
        assert not cm.Config(**kw).refused()
        dcl.carve_sees_through(dcl.DenseCarveConfig(**kw), o, g, p)
    cfg = dcl.DenseCarveConfig().to_c()
    fp = lambda a: capi.ptr(a, C.c_float)  # noqa: E731
    null = capi.ptr(None, C.c_float)
    assert lib.dmsa_dense_carve_sees_through(None, fp(o), fp(g), fp(p)) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_carve_sees_through(C.byref(cfg), null, fp(g), fp(p)) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_carve_sees_through(C.byref(cfg), fp(o), fp(g), null) == capi.DMSA_ERR_INVALID
    n = C.c_int64(5)
    nocells = capi.ptr(None, C.c_int32)
    for cell in (0.0, -1.0, np.nan, np.inf):
        assert lib.dmsa_dense_carve_walk(cell, fp(o), fp(g), nocells, 0, C.byref(n)) == capi.DMSA_ERR_INVALID and n.value == 0
        with pytest.raises(DmsaError):
            dcl.carve_walk(cell, o, g)
    assert lib.dmsa_dense_carve_walk(1.0, null, fp(g), nocells, 0, C.byref(n)) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_carve_walk(1.0, fp(o), fp(g), nocells, 0, None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_carve_walk(1.0, fp(o), fp(g), nocells, -1, C.byref(n)) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_carve_walk(1.0, fp(o), fp(g), nocells, 3, C.byref(n)) == capi.DMSA_ERR_INVALID  # room promised, no buffer
    # the device calls refuse a null object before they touch anything
    assert lib.dmsa_dense_cloud_carve_walk_rows(None, C.byref(cfg), 0, 0, None, None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_count_passes(None, C.byref(cfg), None, None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_remove_transients(None, None) == capi.DMSA_ERR_INVALID
