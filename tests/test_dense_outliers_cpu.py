"""CPU-side checks of include/dmsa_dense_outliers.h: the numpy model of O2-O5 (tests/dense_outliers_model.py, the yardstick of the GPU tests)
against scipy's cKDTree in float64, the host function of O5 against the model bit for bit, and the symbols, structs, defaults and refusals of
the host-only calls.

(a) The bound of the m_i comparison is 4 (k + 4) 2^-24 relative: the k + 2 roundings of O3 (k square roots, k - 1 additions, one division)
plus those of d2, with a factor 4 of margin.  On the cloud below (two noisy planes and 150 strays, one point per 0.1 m voxel, radius 0.3) the
band of rows whose k-th float64 distance lies within 1e-5 radius of the radius held 0 rows when the issue was written, and the largest
relative difference was 2.2e-7 against 4.8e-6 at k = 16."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
from scipy.spatial import cKDTree

from dmsa_lidar_slam_amd import _capi as capi
from dmsa_lidar_slam_amd import dense_cloud as dcl

import dense_outliers_model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
RADIUS = 0.3


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


# ---- (a) the model against cKDTree -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planes():
    rng = np.random.default_rng(7)
    n = 6000
    a = np.c_[rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.normal(0, 0.01, n)]
    b = np.c_[rng.uniform(-4, 4, n // 2), np.full(n // 2, 3.0) + rng.normal(0, 0.01, n // 2), rng.uniform(0, 2.5, n // 2)]
    s = np.c_[rng.uniform(-4, 4, 150), rng.uniform(-3, 3, 150), rng.uniform(0.5, 2.5, 150)]
    p = np.concatenate([a, b, s]).astype(f32)
    cells = np.floor(p / f32(0.1)).astype(np.int64)
    _, first = np.unique(cells, axis=0, return_index=True)
    g = p[np.sort(first)]  # one point per voxel, in input order
    assert 6000 < g.shape[0] < 7500
    g64 = g.astype(np.float64)
    dist, _ = cKDTree(g64).query(g64, k=17)
    return g, dist[:, 1:]


@pytest.mark.parametrize("k", [1, 8, 16])
def test_model_mean_distance_equals_ckdtree_outside_the_rounding_band(planes, k):
    g, dist = planes
    r = float(f32(RADIUS))
    m = om.knn_mean_distance(g, RADIUS, k, chunk=512)
    iso = np.isnan(m)
    assert (m[iso].view(np.uint32) == om.QNAN_BITS).all()
    kth = dist[:, k - 1]
    band = np.abs(kth - r) <= 1e-5 * r
    iso64 = kth > r
    print(f"k = {k}: rows {g.shape[0]}, isolated {int(iso.sum())}, in the band {int(band.sum())}")
    assert band.mean() <= 0.01
    assert np.array_equal(iso[~band], iso64[~band])
    ok = ~iso & ~iso64 & ~band
    want = dist[ok, :k].mean(axis=1)
    rel = np.abs(m[ok].astype(np.float64) - want) / want
    bound = 4.0 * (k + 4) * 2.0**-24
    q = om.quantise(m, RADIUS)
    print(f"k = {k}: largest relative difference {rel.max():.3e} (bound {bound:.3e}); largest q {int(q.max())}")
    assert ok.sum() > 0.5 * g.shape[0] and rel.max() <= bound
    assert q.max() <= 2**18 and (q[iso] == -1).all() and (q[~iso] >= 0).all()
    if k == 8:  # the filter does what it is for: the strays between the surfaces go, the planes stay
        flags, stats, _ = om.classify(g, RADIUS, 8, 1.0, chunk=512)
        assert stats["rows"] == stats["isolated"] + stats["above_threshold"] + stats["inliers"] and 0.7 * g.shape[0] < stats["inliers"] < g.shape[0]
        stray = (g[:, 2] > 0.3) & (g[:, 1] < 2.7)
        assert flags[stray].mean() < 0.2 and flags[~stray].mean() > 0.8


def test_model_on_tiny_clouds_and_duplicates():
    g = np.array([[0, 0, 0], [0.1, 0, 0], [0.1, 0, 0], [5, 5, 5]], f32)
    m = om.knn_mean_distance(g, RADIUS, 1)
    assert m[0] == f32(0.1) and m[1] == 0 and m[2] == 0 and np.isnan(m[3])  # a second row at the same place is a candidate at distance 0
    m2 = om.knn_mean_distance(g, RADIUS, 2)
    assert m2[0] == f32(f32(f32(0.1) + f32(0.1)) / f32(2)) and m2[1] == f32(f32(0.1) / f32(2)) and np.isnan(m2[3])
    assert np.isnan(om.knn_mean_distance(g[:1], RADIUS, 3)).all() and np.isnan(om.knn_mean_distance(g[:3], RADIUS, 3)).all()
    assert float(om.scale_of(0.3)) == 2.0**19 and float(om.scale_of(0.5)) == 2.0**18 and float(om.scale_of(0.25)) == 2.0**19


# ---- (b) O5 on the host against the model, bit for bit ------------------------------------------------------------------------------------------
def _bits(x):
    return struct.pack("<d", x)


def _cases():
    rng = np.random.default_rng(11)
    cases = [(0, 0, 0), (1, 7, 49), (1, 2**18, 2**36), (2, 10, 50), (2, 3, 5), (2, 2**19, 2**37), (3, 30, 302)]
    # equal values: the exact variance is 0 and the rounded one may fall below it
    for n, q in ((3, 144523), (7, 99991), (1000, 262143), (123457, 77777), (2**26, 262143), (2**26 - 3, 181817)):
        cases.append((n, n * q, n * q * q))
    # the largest sums O1 admits: 2^26 rows of q = 2^18
    cases.append((2**26, 2**44, 2**62))
    cases.append((2**26, 2**44 - 2**20, 2**62 - 2**39))
    for _ in range(200):
        n = int(rng.integers(2, 5000))
        q = rng.integers(0, 2**18 + 1, n).astype(object)
        cases.append((n, int(q.sum()), int((q * q).sum())))
    for _ in range(50):  # nearly equal values: cancellation in S2 - S1^2 / n
        n = int(rng.integers(2, 100000))
        base = int(rng.integers(1000, 2**18 - 2))
        q = (base + rng.integers(0, 2, n)).astype(object)
        cases.append((n, int(q.sum()), int((q * q).sum())))
    return cases


def test_threshold_equals_the_model_bit_for_bit(lib):
    negative_seen = 0
    for n_s, s1, s2 in _cases():
        for mul in (0.0, 1.0, 2.5, 0.1, 1e6):
            got = dcl.outlier_threshold(n_s, s1, s2, mul)
            want = om.threshold(n_s, s1, s2, mul)
            assert [_bits(v) for v in got] == [_bits(v) for v in want], (n_s, s1, s2, mul, got, want)
        if n_s >= 2 and (float(s2) - (float(s1) * float(s1)) / float(n_s)) < 0.0:
            negative_seen += 1
            assert dcl.outlier_threshold(n_s, s1, s2, 3.0) == (float(s1) / float(n_s), 0.0, float(s1) / float(n_s))  # var < 0 from rounding: 0
    assert negative_seen > 0
    assert dcl.outlier_threshold(0, 0, 0, 5.0) == (0.0, 0.0, 0.0)
    assert dcl.outlier_threshold(1, 9, 81, 5.0) == (9.0, 0.0, 9.0)
    assert dcl.outlier_threshold(2, 10, 52, 1.0) == (5.0, 2.0**0.5, 5.0 + 2.0**0.5)
    mean, sd, t = dcl.outlier_threshold(2**26, 2**44, 2**62, 1.0)
    assert (mean, sd, t) == (2.0**18, 0.0, 2.0**18)


# ---- (c) exports, defaults, refusals ---------------------------------------------------------------------------------------------------------
def test_symbol_tuple_equals_the_header_and_the_library_exports_it(lib):
    header = open(os.path.join(ROOT, "include", "dmsa_dense_outliers.h")).read()
    declared = set(re.findall(r"\b(dmsa_[a-z_0-9]+)\s*\(", header))
    assert declared == set(capi.DENSE_OUTLIERS_SYMBOLS) and len(capi.DENSE_OUTLIERS_SYMBOLS) == len(declared) == 6
    assert not declared & (set(capi.EXPORTED_SYMBOLS) | set(capi.DENSE_CLOUD_SYMBOLS) | set(capi.DENSE_NORMALS_SYMBOLS))
    for name in declared:
        assert hasattr(lib, name), name
    for rule in ("O1", "O2", "O3", "O4", "O5", "O6"):
        assert re.search(rf"\b{rule}\b", header)


def test_struct_layouts_and_defaults(lib):
    assert C.sizeof(capi.DenseOutlierConfig) == 16 and [getattr(capi.DenseOutlierConfig, n).offset for n in ("radius", "k", "stddev_mul", "pad")] == [0, 4, 8, 12]
    assert C.sizeof(capi.DenseOutlierStats) == 80 and capi.DenseOutlierStats.mean_m.offset == 56
    assert dcl.OUTLIER_STAT_NAMES == ("rows", "isolated", "above_threshold", "inliers", "n_s", "s1", "s2", "mean_m", "stddev_m", "threshold_m")
    c = capi.DenseOutlierConfig()
    C.memset(C.byref(c), 0x5A, C.sizeof(c))
    lib.dmsa_default_dense_outlier_config(C.byref(c))
    assert (c.radius, c.k, c.stddev_mul, c.pad) == (float(f32(0.3)), 8, 1.0, 0)
    lib.dmsa_default_dense_outlier_config(None)


def test_host_only_calls_refuse_bad_arguments(lib):
    from dmsa_lidar_slam_amd.api import DmsaError

    for args in ((-1, 0, 0, 1.0), (3, -1, 5, 1.0), (3, 1, -5, 1.0), (3, 30, 302, -0.5), (3, 30, 302, np.nan), (3, 30, 302, np.inf)):
        with pytest.raises(DmsaError):
            dcl.outlier_threshold(*args)
        out = [C.c_double(7.0) for _ in range(3)]
        assert lib.dmsa_dense_outlier_threshold(args[0], args[1], args[2], float(args[3]), *[C.byref(v) for v in out]) == capi.DMSA_ERR_INVALID
        assert [v.value for v in out] == [0.0, 0.0, 0.0]
    # any of the three outputs may be NULL
    t = C.c_double(0)
    null = capi.ptr(None, C.c_double)
    assert lib.dmsa_dense_outlier_threshold(3, 30, 302, 1.0, null, null, C.byref(t)) == capi.DMSA_OK and t.value == 11.0
    assert lib.dmsa_dense_outlier_threshold(3, 30, 302, 1.0, null, null, null) == capi.DMSA_OK
    # the device calls refuse a null object before they touch anything
    cfg = capi.DenseOutlierConfig(0.3, 8, 1.0, 0)
    assert lib.dmsa_dense_cloud_classify_outliers(None, C.byref(cfg), None, None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_knn_mean_distance(None, C.byref(cfg), 0, 0, None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_remove_outliers(None, None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_save_pcd_retained(None, b"/nowhere", None, None) == capi.DMSA_ERR_INVALID
