"""CPU-side checks of include/dmsa_dense_normals.h: the symbol list, the struct, the header text, the numpy model of the neighbourhoods
(tests/dense_normals_model.py, the yardstick of the GPU tests) against scipy's cKDTree, and the host function of N4,
dmsa_dense_normal_from_moments -- the arithmetic the device kernel compiles from the same header -- against numpy.linalg.eigh.

The bounds of the eigh comparison come from the CPU yardstick the project already has, not from the new code: the oracle's
orc_update_normals (k = 8, PCL's float eigen33 restated) against eigh in float64 on its own neighbourhoods, over the same clouds and under
the same eigenvalue-gap condition.  Measured on the clouds below (seed 7, 120 patches within 2 m of the origin; 13 093 yardstick rows of
which 13 074 have lambda_1 >= 4 lambda_0):  A = 1.047e-2 rad,  curvature yardstick C = 3.462e-3.  The new function on the same clouds (120 of
120 rows qualify): largest angle 2.49e-7 rad, largest curvature difference 6.9e-8; the bounds are 2 A and 2 C.  (With the patches 20 m from
the origin the yardstick's own single-pass float covariance cancels and A reaches 1.56 rad, a bound that would say nothing: hence 2 m.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.spatial import cKDTree

from dmsa_lidar_slam_amd import _capi as capi
from dmsa_lidar_slam_amd import dense_cloud as dcl

import dense_normals_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


# ---- symbols, struct, header ---------------------------------------------------------------------------------------------------------------
def test_symbol_tuple_equals_the_header_and_the_library_exports_it(lib):
    header = open(os.path.join(ROOT, "include", "dmsa_dense_normals.h")).read()
    declared = set(re.findall(r"\b(dmsa_[a-z_0-9]+)\s*\(", header))
    assert declared == set(capi.DENSE_NORMALS_SYMBOLS) and len(capi.DENSE_NORMALS_SYMBOLS) == len(declared) == 8
    assert not declared & set(capi.EXPORTED_SYMBOLS) and not declared & set(capi.DENSE_CLOUD_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    # the header states the semantics it decides, and does not claim PCL's writer for its file
    for rule in ("N0", "N1", "N2", "N3", "N4", "N5"):
        assert re.search(rf"\b{rule}\b", header)
    assert "decided here, self-describing" in header


def test_struct_layout_and_defaults(lib):
    assert C.sizeof(capi.DenseNormalsConfig) == 8 and capi.DenseNormalsConfig.min_neighbours.offset == 4
    c = capi.DenseNormalsConfig()
    C.memset(C.byref(c), 0x5A, C.sizeof(c))
    lib.dmsa_default_dense_normals_config(C.byref(c))
    assert (c.radius, c.min_neighbours) == (float(f32(0.3)), 5)


def test_header_is_its_stated_text(lib):
    want = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z normal_x normal_y normal_z curvature\nSIZE 4 4 4 4 4 4 4\n"
            "TYPE F F F F F F F\nCOUNT 1 1 1 1 1 1 1\nWIDTH 000000012345\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 000000012345\nDATA binary\n")
    assert dcl.pcdHeaderNormalsBinary(12345) == want
    assert {len(dcl.pcdHeaderNormalsBinary(n)) for n in (0, 1, 999_999_999_999)} == {len(want)}
    buf = C.create_string_buffer(512)
    assert lib.dmsa_pcd_header_normals_binary(10**12, buf, 512) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_pcd_header_normals_binary(-1, buf, 512) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_pcd_header_normals_binary(5, buf, len(want)) == capi.DMSA_ERR_INVALID  # no room for the terminating zero
    assert lib.dmsa_pcd_header_normals_binary(5, buf, len(want) + 1) == len(want)


# ---- the model's neighbourhoods against scipy --------------------------------------------------------------------------------------------------
def test_model_neighbour_sets_equal_ckdtree_outside_the_rounding_band():
    rng = np.random.default_rng(3)
    r = 0.2
    g = rng.uniform(-0.6, 0.6, (1500, 3)).astype(f32) + f32([40.0, -25.0, 2.0])
    mask = nm.neighbour_mask(g, r)
    g64 = g.astype(np.float64)
    tree = cKDTree(g64)
    ball = np.zeros_like(mask)
    for i, js in enumerate(tree.query_ball_point(g64, r)):
        ball[i, js] = True
    dist = np.linalg.norm(g64[:, None, :] - g64[None, :, :], axis=2)
    band = np.abs(dist - r) <= 1e-5 * r
    near = dist <= 1.5 * r  # the pairs a search looks at
    share = band[near].mean()
    print("pairs within 1e-5 r of r:", int(band.sum()), "of", int(near.sum()), "share", share)
    assert share < 0.01
    assert np.array_equal(mask[~band], ball[~band])
    assert mask.diagonal().all() and np.array_equal(mask, mask.T)  # i is its own neighbour; d2 is symmetric in float
    assert 20 < mask.sum(axis=1).mean() < 40
    # the moments' count is the size of the set
    assert np.array_equal(nm.moments(g, r, rows=np.arange(0, 1500, 7))[:, 0], mask[::7].sum(axis=1))


# ---- N4 against eigh -------------------------------------------------------------------------------------------------------------------------
R = 0.3


def _patches(seed=7, count=120):
    """Noisy planar patches (sigma = 0.01 r, 20-200 points inside 0.9 r of their first point, random orientation) within 2 m of the origin."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(20, 201))
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        rad, phi = 0.9 * R * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
        local = np.stack([rad * np.cos(phi), rad * np.sin(phi), rng.normal(0, 0.01 * R, n)], axis=1)
        local[0] = 0.0
        out.append((local @ q.T + rng.uniform(-2, 2, 3)).astype(f32))
    return out


def _angle(a, b):
    """The angle between two directions, up to sign."""
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), abs(float(np.dot(a, b)))))


@pytest.fixture(scope="module")
def yardstick():
    """A and C: orc_update_normals (k = 8) against eigh on its own neighbourhoods, rows with lambda_1 >= 4 lambda_0."""
    from oracle import oracle_py as orc

    A = Cv = 0.0
    rows = used = 0
    for cloud in _patches():
        c4 = np.concatenate([cloud, np.zeros((cloud.shape[0], 1), f32)], axis=1)
        normal, nn = orc.update_normals(c4, k=8, neighbours=True)
        for i in range(cloud.shape[0]):
            p = cloud[nn[i][nn[i] >= 0]].astype(np.float64)
            w, v = np.linalg.eigh(np.cov(p.T, bias=True))
            rows += 1
            if not (w[1] >= 4.0 * w[0]) or not np.isfinite(normal[i]).all():
                continue
            used += 1
            A = max(A, _angle(normal[i, :3].astype(np.float64), v[:, 0]))
            Cv = max(Cv, abs(float(normal[i, 3]) - abs(w[0] / w.sum())))
    print(f"yardstick: {rows} rows, {used} with lambda_1 >= 4 lambda_0; A = {A:.3e} rad, curvature C = {Cv:.3e}")
    assert used > 0.5 * rows
    return A, Cv


def test_normal_from_moments_against_eigh_within_twice_the_yardstick(yardstick):
    A, Cv = yardstick
    worst_angle = worst_curv = 0.0
    rows = used = 0
    for cloud in _patches():
        m = nm.moments(cloud, R, rows=[0])  # the first point is the patch's centre: every point of the patch is its neighbour
        assert m[0, 0] == cloud.shape[0]
        got = dcl.normal_from_moments(m, np.array([[0.0, 0.0, 1.0]], f32), 5)[0]
        ref_n, ref_c, w = nm.eigh_normal(m[0])
        rows += 1
        if not w[1] >= 4.0 * w[0]:
            continue
        used += 1
        assert np.isfinite(got).all() and abs(float(np.linalg.norm(got[:3].astype(np.float64))) - 1.0) < 1e-6
        worst_angle = max(worst_angle, _angle(got[:3].astype(np.float64), ref_n))
        worst_curv = max(worst_curv, abs(float(got[3]) - ref_c))
    print(f"normal_from_moments vs eigh: {used} of {rows} rows; largest angle {worst_angle:.3e} rad (bound {2 * A:.3e}), "
          f"largest curvature difference {worst_curv:.3e} (bound {2 * Cv:.3e})")
    assert used >= 0.95 * rows
    assert worst_angle <= 2.0 * A
    assert worst_curv <= 2.0 * Cv


def test_normals_point_toward_the_view_vector():
    rng = np.random.default_rng(12)
    clouds = _patches(seed=8, count=40)
    m = np.concatenate([nm.moments(c, R, rows=[0]) for c in clouds])
    w = rng.normal(0, 5, (len(clouds), 3)).astype(f32)
    n = dcl.normal_from_moments(m, w, 5)
    assert np.isfinite(n).all()
    dot = (w[:, 0] * n[:, 0] + w[:, 1] * n[:, 1]) + w[:, 2] * n[:, 2]  # float32, in the stated order
    assert dot.dtype == f32 and (dot >= 0).all()
    flipped = dcl.normal_from_moments(m, -w, 5)  # the opposite view: the opposite normal, the same curvature
    assert np.array_equal(flipped[:, :3], -n[:, :3]) and np.array_equal(flipped[:, 3], n[:, 3])


def test_small_neighbourhoods(lib):
    cloud = _patches(seed=9, count=1)[0]
    view = np.array([[0.0, 0.0, 1.0]], f32)

    def first_rows(k):
        return nm.moments(cloud[:k], R, rows=[0])

    for k, min_nb, finite in ((1, 0, False), (2, 0, False), (3, 0, True), (3, 3, True), (4, 5, False), (5, 5, True), (9, 10, False), (10, 10, True)):
        m = first_rows(k)
        assert m[0, 0] == k
        out = dcl.normal_from_moments(m, view, min_nb)[0]
        if finite:
            assert np.isfinite(out).all(), (k, min_nb, out)
        else:
            assert np.isnan(out).all() and (out.view(np.uint32) == 0x7FC00000).all(), (k, min_nb, out)  # four quiet NaNs
    # three collinear points: no plane; whatever comes out is finite or NaN, never an exception, and the same every time
    line = np.array([[0, 0, 0], [0.05, 0.05, 0.05], [-0.1, -0.1, -0.1]], f32)
    m = nm.moments(line, R, rows=[0])
    assert m[0, 0] == 3
    a = dcl.normal_from_moments(m, view, 0)
    b = dcl.normal_from_moments(m, view, 0)
    assert a.tobytes() == b.tobytes()
    # arguments
    out = np.zeros(4, f32)
    assert lib.dmsa_dense_normal_from_moments(None, capi.ptr(view[0].copy(), C.c_float), 0, capi.ptr(out, C.c_float)) == capi.DMSA_ERR_INVALID
