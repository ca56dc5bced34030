"""CPU-side checks of include/dmsa_dense_clusters.h: the symbol list, the structs and defaults, the header text of C7, the null-object
refusals, and the model (tests/dense_clusters_model.py, the yardstick of the GPU tests): its adjacency is symmetric, its cKDTree candidates
lose no pair and admit none, its two variants agree, and the chain and the d2 == r2 rows come out as C2-C3 say."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.spatial import cKDTree

from dmsa_lidar_slam_amd import _capi as capi
from dmsa_lidar_slam_amd import dense_cloud as dcl

import dense_clusters_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def chain(n=3000, spacing=0.18, seed=3):
    """n rows along x, `spacing` apart, in shuffled store order: (xyz (n,3) float32, position of every row along the chain)."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n)
    xyz = np.zeros((n, 3), f32)
    xyz[:, 0] = (f32(spacing) * order.astype(f32)).astype(f32)
    xyz[:, 1], xyz[:, 2] = f32(0.3), f32(-0.2)
    return xyz, order


def test_symbol_tuple_equals_the_header_and_the_library_exports_it(lib):
    header = open(os.path.join(ROOT, "include", "dmsa_dense_clusters.h")).read()
    declared = set(re.findall(r"\b(dmsa_[a-z_0-9]+)\s*\(", header))
    assert declared == set(capi.DENSE_CLUSTERS_SYMBOLS) and len(capi.DENSE_CLUSTERS_SYMBOLS) == len(declared) == 6
    others = (set(capi.EXPORTED_SYMBOLS) | set(capi.DENSE_CLOUD_SYMBOLS) | set(capi.DENSE_NORMALS_SYMBOLS) | set(capi.DENSE_OUTLIERS_SYMBOLS) |
              set(capi.DENSE_CARVE_SYMBOLS) | set(capi.DENSE_INTENSITY_SYMBOLS))
    assert not declared & others
    for name in declared:
        assert hasattr(lib, name), name
    for rule in ("C1", "C2", "C3", "C4", "C5", "C6", "C7"):
        assert re.search(rf"\b{rule}\b", header)
    assert "DECIDED HERE" in header


def test_structs_and_defaults(lib):
    assert C.sizeof(capi.DenseClusterConfig) == 16 and C.sizeof(capi.DenseClusterStats) == 56
    assert [capi.DenseClusterConfig.radius.offset, capi.DenseClusterConfig.min_size.offset, capi.DenseClusterConfig.max_size.offset] == [0, 4, 8]
    cfg = capi.DenseClusterConfig(9.0, 9, 9, 9)
    lib.dmsa_default_dense_cluster_config(C.byref(cfg))
    assert (cfg.radius, cfg.min_size, cfg.max_size, cfg.pad) == (float(f32(0.3)), 50, 0, 0)
    lib.dmsa_default_dense_cluster_config(None)
    assert dcl.CLUSTER_STAT_NAMES == ("rows", "clusters", "largest", "kept_rows", "kept_clusters", "small_rows", "large_rows")


@pytest.mark.parametrize("intensity", [False, True])
def test_the_header_is_its_stated_text(lib, intensity):
    k = 5 if intensity else 4
    fields = "x y z intensity label" if intensity else "x y z label"
    lengths = set()
    for n in (0, 1, 10**12 - 1):
        want = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS " + fields + "\nSIZE" + " 4" * k + "\nTYPE" + " F" * (k - 1) + " U\nCOUNT" + " 1" * k +
                "\nWIDTH %012d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %012d\nDATA binary\n" % (n, n))
        assert dcl.pcdHeaderXyzLabelBinary(n, intensity) == want == cm.header(n, intensity)
        lengths.add(len(want))
    assert len(lengths) == 1  # the counts are twelve digits wide whatever n
    size = lengths.pop()
    buf = C.create_string_buffer(512)
    assert lib.dmsa_pcd_header_xyz_label_binary(5, int(intensity), buf, size) == -1  # no room for the terminating 0
    assert lib.dmsa_pcd_header_xyz_label_binary(5, int(intensity), buf, size + 1) == size
    assert lib.dmsa_pcd_header_xyz_label_binary(-1, int(intensity), buf, 512) == -1 and lib.dmsa_pcd_header_xyz_label_binary(10**12, int(intensity), buf, 512) == -1
    assert lib.dmsa_pcd_header_xyz_label_binary(5, int(intensity), None, 512) == -1
    assert cm.row_dtype(intensity).itemsize == 4 * k


def test_null_objects_are_refused(lib):
    cfg = capi.DenseClusterConfig(0.3, 50, 0, 0)
    st = capi.DenseClusterStats(*([7] * 7))
    kept, a, b = C.c_int64(5), C.c_int64(5), C.c_int64(5)
    assert lib.dmsa_dense_cloud_cluster_labels(None, C.byref(cfg), None, None) == -1
    assert lib.dmsa_dense_cloud_classify_clusters(None, C.byref(cfg), None, C.byref(st)) == -1 and st.rows == 0 and st.large_rows == 0
    assert lib.dmsa_dense_cloud_remove_clusters(None, C.byref(kept)) == -1 and kept.value == 0
    assert lib.dmsa_dense_cloud_save_pcd_labels(None, b"/nonexistent/x.pcd", C.byref(a), C.byref(b)) == -1 and (a.value, b.value) == (0, 0)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
def test_the_models_adjacency_is_symmetric_bit_for_bit():
    rng = np.random.default_rng(1)
    g = rng.uniform(-1, 1, (500, 3)).astype(f32)
    i, j = np.triu_indices(500, 1)
    a, b = cm._d2(g, i, j), cm._d2(g, j, i)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_ckdtree_candidates_lose_no_pair_and_admit_none():
    rng = np.random.default_rng(2)
    g = rng.uniform(0, 1.5, (4000, 3)).astype(f32)
    r = 0.2
    got = {tuple(p) for p in cm.adjacent_pairs(g, r)}
    tree = cKDTree(g.astype(np.float64))
    inner = {tuple(sorted(p)) for p in tree.query_pairs(float(f32(r)) * (1 - 1e-6))}
    outer = {tuple(sorted(p)) for p in tree.query_pairs(float(f32(r)) * (1 + 1e-6))}
    assert len(got) > 50000 and inner <= got <= outer
    assert got == {tuple(p) for p in cm.adjacent_pairs_brute(g, r)}


@pytest.mark.parametrize("n,side,r", [(1, 1.0, 0.2), (2, 0.1, 0.2), (300, 1.0, 0.12), (1500, 2.0, 0.15)])
def test_brute_force_and_ckdtree_variants_agree(n, side, r):
    g = np.random.default_rng(n).uniform(0, side, (n, 3)).astype(f32)
    assert np.array_equal(cm.adjacent_pairs(g, r), cm.adjacent_pairs_brute(g, r))
    a, b = cm.classify(g, r, 3, 40), cm.classify(g, r, 3, 40, brute=True)
    assert a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip((a[0], a[2], a[3]), (b[0], b[2], b[3])))
    label, size = a[2], a[3]
    assert (label <= np.arange(n)).all() and (label[label] == label).all() and np.array_equal(size, np.bincount(label, minlength=n)[label])
    st = a[1]
    assert st["rows"] == n == st["kept_rows"] + st["small_rows"] + st["large_rows"] and st["clusters"] == len(np.unique(label)) and st["largest"] == size.max()


def test_a_shuffled_chain_is_one_cluster_with_label_zero():
    xyz, order = chain()
    label, size = cm.labels(xyz, 0.2)
    assert (label == 0).all() and (size == 3000).all() and order[0] != 0  # row 0 lies somewhere along the chain
    pairs = cm.adjacent_pairs(xyz, 0.2)
    assert pairs.shape[0] == 2999  # a path: the graph's diameter is 2999


def test_rows_at_exactly_r_link_and_one_ulp_beyond_does_not():
    r = f32(0.2)
    beyond = f32(2.0) * r + np.nextafter(r, f32(1))
    xyz = np.array([[0, 0, 0], [r, 0, 0], [f32(2.0) * r, 0, 0], [beyond, 0, 0]], f32)
    assert cm._d2(xyz, np.array([0, 1]), np.array([1, 2])).tolist() == [cm.r2_of(r)] * 2 and cm._d2(xyz, np.array([2]), np.array([3]))[0] > cm.r2_of(r)
    label, size = cm.labels(xyz, r)
    assert label.tolist() == [0, 0, 0, 3] and size.tolist() == [3, 3, 3, 1]
    flags, st, _, _ = cm.classify(xyz, r, 2)
    assert flags.tolist() == [1, 1, 1, 0] and st == dict(rows=4, clusters=2, largest=3, kept_rows=3, kept_clusters=1, small_rows=1, large_rows=0)
    flags, st, _, _ = cm.classify(xyz, r, 1, 2)
    assert flags.tolist() == [0, 0, 0, 1] and st["large_rows"] == 3 and st["kept_clusters"] == 1


def test_the_models_file_bytes():
    g = np.array([[1, 2, 3, 0.5], [4, 5, 6, 0.25]], f32)
    for intensity in (False, True):
        raw = cm.file_bytes(g, [0, 1], intensity)
        head = cm.header(2, intensity).encode()
        body = np.frombuffer(raw[len(head):], "<u4").reshape(2, -1)
        assert raw.startswith(head) and body.shape[1] == (5 if intensity else 4) and body[:, -1].tolist() == [0, 1]
        assert np.array_equal(body[:, :3].view(f32), g[:, :3]) and (not intensity or np.array_equal(body[:, 3].view(f32), g[:, 3]))
