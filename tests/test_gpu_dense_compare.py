"""GPU tests of include/dmsa_dense_compare.h against the model of D0-D7 (tests/dense_compare_model.py: cKDTree candidates re-tested in
float32, the winner by (d2, row), Python-int sums).  Every comparison is array_equal on bits, the NaN pattern included: a nearest row is a
minimum over 64-bit keys, so a candidate missed at a cell face or a tile seam, a tie resolved by arrival order or a row number taken from the
sorted order changes an integer.

k_nearest_across walks one set's grid with the other set's queries (csrc/dense_grid_walk.h), so the shapes are those of
tests/test_gpu_dense_outliers.py and the cloud builders of tests/test_gpu_dense_normals.py are reused: the store is one scan on the identity
trajectory, one row per voxel; the reference is any set of rows.

Not tested here: the bounds of 2^26 rows of either set (clouds of gigabytes); the refusal of the reference bound is tested, it reads no row."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dense_compare_model as dm
import test_gpu_dense_cloud as base
import test_gpu_dense_normals as ng

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL, REACH, TOL = ng.VOXEL, ng.RADIUS, 0.0625  # 0.05, 0.2 and a tolerance between them
_bits = ng._bits


@pytest.fixture(scope="module")
def opt():
    from dmsa_lidar_slam_amd.api import DmsaOptimizer

    o = DmsaOptimizer(device=0)
    yield o
    o.close()


def _refused(call, text, status=-1):
    from dmsa_lidar_slam_amd.api import DmsaError

    with pytest.raises(DmsaError) as e:
        call()
    assert e.value.status == status and text in e.value.args[0], e.value.args[0]


def _same(got, want):
    """(dist, index) of a stage call against the model's (d2, index)."""
    dist, index = got
    d2, want_index = want
    assert dist.dtype == f32 and index.dtype == np.int32
    assert np.array_equal(index, want_index), (np.flatnonzero(index != want_index)[:10], index[:10], want_index[:10])
    assert np.array_equal(_bits(dist), _bits(dm.dist_of(d2))), np.flatnonzero(_bits(dist) != _bits(dm.dist_of(d2)))[:10]


def _stats_equal(got, want):
    assert list(got) == list(want)
    for name in want:
        if isinstance(want[name], dict):
            assert list(got[name]) == list(want[name])
            for k in want[name]:
                a, b = got[name][k], want[name][k]
                assert (np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)) if isinstance(b, float) else a == b, (name, k, a, b)
        else:
            a, b = got[name], want[name]
            assert (np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)) if isinstance(b, float) else a == b, (name, a, b)


def _check_all(dc, g, ref, valid=None, reach=REACH, tol=TOL, cuts=True):
    """Both directions, a range call cut inside a wave in each, and compare() against the model; returns the model's (stats, arrays)."""
    valid = np.ones(ref.shape[0], np.uint8) if valid is None else valid
    want, (a_d2, a_idx, c_d2, c_idx) = dm.compare(g, ref, valid, reach, tol)
    _same(dc.nearest_in_reference(reach), (a_d2, a_idx))
    _same(dc.nearest_in_store(reach), (c_d2, c_idx))
    n, m = g.shape[0], ref.shape[0]
    if cuts:
        for first, count in ((n // 3, n - n // 3 - n // 5), (n - 1, 1), (n, 0)):
            _same(dc.nearest_in_reference(reach, first, count), (a_d2[first : first + count], a_idx[first : first + count]))
        for first, count in ((m // 3, m - m // 3 - m // 5), (0, 1), (m, 0)):
            _same(dc.nearest_in_store(reach, first, count), (c_d2[first : first + count], c_idx[first : first + count]))
    _stats_equal(dc.compare(reach, tol), want)
    return want, (a_d2, a_idx, c_d2, c_idx)


def _cloud_near(rng, g, m, spread=0.08):
    """m reference rows, each a store row displaced by up to `spread` per axis, some of them twice."""
    pick = rng.integers(0, g.shape[0], m)
    return (g[pick, :3] + rng.uniform(-spread, spread, (m, 3))).astype(f32)


# ---- 1. every total -------------------------------------------------------------------------------------------------------------------------------
TOTALS = [1, 2, 63, 64, 65, 257, 4097]


@pytest.mark.parametrize("rows,ref_rows", [(t, t) for t in TOTALS] + [(1, 4097), (4097, 1)])
def test_both_directions_at_every_total(opt, rows, ref_rows):
    rng = np.random.default_rng(rows + 7 * ref_rows)
    side = 3 if rows < 3 else 8 if rows < 100 else 12 if rows < 300 else 32
    xyz = ng._one_per_voxel(rng, rows, VOXEL, side, corner=(-0.3, -0.3, -0.3))
    dc, kept = ng._still_cloud(opt, xyz, VOXEL)
    assert kept.shape[0] == rows == dc.retained_count()
    g, _ = dc.retained()
    ref = _cloud_near(rng, g, ref_rows, 0.12)
    dc.set_reference(ref)
    assert dc.reference_count() == ref_rows
    want, _ = _check_all(dc, g, ref)
    dc.close()
    if min(rows, ref_rows) >= 63:
        acc, com = want["accuracy"], want["completeness"]
        assert acc["matched"] > rows // 2 and 0 < acc["within"] < acc["matched"] and com["matched"] > ref_rows // 2
        assert sum(1 for b in acc["histogram"] if b) > 20


# ---- 2. ties, duplicates, the bound ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap", [False, True])
def test_a_query_midway_between_two_reference_rows_takes_the_lower_row(opt, swap):
    """Coordinates that are multiples of 2^-4: both d2 are exactly 2^-4 whatever the order of the operations."""
    rng = np.random.default_rng(3)
    fill = ng._one_per_voxel(rng, 200, VOXEL, 10, corner=(2.0, 2.0, 2.0))
    xyz = np.concatenate([fill[:77], np.array([[0.25, 0.25, 0.0]], f32), fill[77:]]).astype(f32)
    if swap:
        xyz = xyz[::-1].copy()
    q = 123 if swap else 77
    ref = np.array([[9.0, 9.0, 9.0], [0.5, 0.25, 0.0], [0.0, 0.25, 0.0], [0.25, 0.5, 0.0], [0.25, 0.25, -0.25]], f32)
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
        dc, _ = ng._still_cloud(opt, xyz, VOXEL)
        g, _ = dc.retained()
        assert np.array_equal(_bits(g[q, :3]), _bits(f32([0.25, 0.25, 0.0])))
        dc.set_reference(ref[order])
        dist, index = dc.nearest_in_reference(0.5)
        lowest = min(k for k, r in enumerate(order) if r != 0)
        assert index[q] == lowest and dist[q] == f32(0.25)
        _check_all(dc, g, ref[order], reach=0.5, tol=0.25, cuts=False)
        dc.close()


def test_two_hundred_identical_reference_rows_and_a_cell_of_1500(opt):
    rng = np.random.default_rng(8)
    xyz = ng._one_per_voxel(rng, 400, VOXEL, 8, corner=(0.0, 0.0, 0.0))
    dc, _ = ng._still_cloud(opt, xyz, VOXEL)
    g, _ = dc.retained()
    # 30 other rows, then 200 copies of one point: row 30 wins wherever it wins at all
    twin = np.array([0.21, 0.17, 0.19], f32)
    ref = np.concatenate([rng.uniform(0.0, 0.4, (30, 3)), np.tile(twin, (200, 1))]).astype(f32)
    dc.set_reference(ref)
    _, (a_d2, a_idx, _, _) = _check_all(dc, g, ref)
    assert (a_idx >= 30).sum() >= 5 and set(a_idx[a_idx >= 30]) == {30}
    # one cell of the grid (edge 1.001 * 0.2) with 1 500 reference rows: 24 tiles of 64 with a seam inside the cell's run
    ref = rng.uniform(0.005, 0.195, (1500, 3)).astype(f32)
    inside = int(np.flatnonzero(((g[:, :3] > 0.005) & (g[:, :3] < 0.195)).all(axis=1))[0])
    ref[640] = ref[700:900] = g[inside, :3]  # duplicates across the seams, on a store row
    dc.set_reference(ref)
    _, (a_d2, a_idx, c_d2, c_idx) = _check_all(dc, g, ref)
    dc.close()
    assert not np.isin(a_idx, np.arange(700, 900)).any() and a_idx[inside] == 640 and a_d2[inside] == 0 and (~np.isnan(c_d2)).all()


@pytest.mark.parametrize("which", ["max_distance", "tolerance"])
def test_a_lone_candidate_at_exactly_the_bound_and_one_step_beyond(opt, which):
    reach, tol = f32(0.2), f32(0.0625)
    bound = reach if which == "max_distance" else tol
    dc, _ = ng._still_cloud(opt, np.array([[0.0, 0.5, 0.5]], f32), VOXEL)  # x = 0: the difference along x is the reference's x itself
    g, _ = dc.retained()
    for x, inside in ((bound, True), (np.nextafter(bound, f32(1)), False)):
        ref = np.array([[x, 0.5, 0.5]], f32)
        assert (dm.d2_to(ref, g[0, :3])[0] <= dm.r2_of(bound)) == inside  # the construction: d2 is the float product itself, or above it
        dc.set_reference(ref)
        want, (a_d2, a_idx, c_d2, c_idx) = _check_all(dc, g, ref, reach=reach, tol=tol, cuts=False)
        matched, confirmed = inside or which == "tolerance", inside and which == "tolerance"  # (at max_distance the row is beyond the tolerance)
        assert (a_idx[0], c_idx[0]) == ((0, 0) if matched else (-1, -1)) and want["accuracy"]["matched"] == int(matched) and want["accuracy"]["within"] == int(confirmed)
        if not matched:
            dist, _ = dc.nearest_in_reference(reach)
            assert _bits(dist)[0] == dm.NAN_BITS
        for keep in ("near", "far"):
            want_c, flags, _ = dm.classify(g, ref, np.ones(1, np.uint8), reach, tol, keep)
            got, got_flags = dc.classify_by_reference(reach, tol, keep, download=True)
            _stats_equal(got, want_c)
            assert got_flags.tolist() == flags.tolist() == [int(confirmed == (keep == "near"))]
    dc.close()


# ---- 3. cell faces, corners and the per-cell path of the walker ------------------------------------------------------------------------------------
def test_pairs_a_hair_apart_across_a_cell_face_and_a_cell_corner(opt):
    rng = np.random.default_rng(17)
    edge = 1.001 * float(f32(REACH))
    fill = ng._one_per_voxel(rng, 300, VOXEL, 10, corner=(2.0, 2.0, 2.0))
    face, corner = 2 * edge, 3 * edge
    pairs_store = np.array([[face - 1e-4, 0.31, 0.33], [corner - 1e-4, corner - 1e-4, corner - 1e-4], [5 * edge + 1e-4, 0.1, 0.1]])
    pairs_ref = np.array([[face + 1e-4, 0.31, 0.33], [corner + 1e-4, corner + 1e-4, corner + 1e-4], [5 * edge - 1e-4, 0.1, 0.1]])
    xyz = np.concatenate([fill, pairs_store]).astype(f32)
    ref = np.concatenate([_cloud_near(rng, fill, 200), pairs_ref]).astype(f32)
    cells = lambda p: np.floor(p.astype(f32).astype(np.float64) / edge)
    assert (np.abs(cells(pairs_store) - cells(pairs_ref)).sum(axis=1) == [1, 3, 1]).all()
    dc, kept = ng._still_cloud(opt, xyz, VOXEL)
    assert kept.shape[0] == 303
    g, _ = dc.retained()
    dc.set_reference(ref)
    _, (a_d2, a_idx, c_d2, c_idx) = _check_all(dc, g, ref)
    dc.close()
    assert a_idx[300:].tolist() == [200, 201, 202] and c_idx[200:].tolist() == [300, 301, 302] and (a_d2[300:] < 1e-6).all()


def test_sorted_order_that_jumps_between_distant_surfaces(opt):
    """120 small blobs and 150 lone rows scattered over 10 m, in the store and -- displaced -- in the reference: 64 consecutive sorted rows of
    either set lie in blobs far apart, the box of a wave exceeds kGridBoxCells and the wave goes through its distinct cells one by one."""
    import test_gpu_dense_outliers as og

    rng = np.random.default_rng(12)
    centres = rng.uniform(-5, 5, (120, 3))
    xyz = np.concatenate([c + ng._one_per_voxel(rng, 30, VOXEL, 4) for c in centres] + [rng.uniform(-5, 5, (150, 3))]).astype(f32)
    xyz = xyz[rng.permutation(xyz.shape[0])]
    dc, kept = ng._still_cloud(opt, xyz, VOXEL)
    g, _ = dc.retained()
    ref = (g[rng.permutation(g.shape[0])[:3000], :3] + rng.uniform(-0.04, 0.04, (3000, 3))).astype(f32)
    assert g.shape[0] > 3000 and (og._wave_box_cells(g, REACH) > 512).mean() > 0.9 and (og._wave_box_cells(ref, REACH) > 512).mean() > 0.9
    dc.set_reference(ref)
    want, _ = _check_all(dc, g, ref)
    dc.close()
    assert want["completeness"]["matched"] == 3000 and want["accuracy"]["unmatched"] > 0


# ---- 4. disjoint, identical ---------------------------------------------------------------------------------------------------------------------------
def test_disjoint_clouds_match_nothing_and_identical_clouds_match_themselves(opt):
    rng = np.random.default_rng(21)
    xyz = ng._one_per_voxel(rng, 700, VOXEL, 12)
    dc, _ = ng._still_cloud(opt, xyz, VOXEL)
    g, _ = dc.retained()
    ref = (g[:500, :3] + f32(10.0)).astype(f32)
    dc.set_reference(ref)
    want, _ = _check_all(dc, g, ref)
    for got in (dc.nearest_in_reference(REACH), dc.nearest_in_store(REACH)):
        assert (_bits(got[0]) == dm.NAN_BITS).all() and (got[1] == -1).all()
    st = dc.compare(REACH, TOL)
    for d, queries in ((st["accuracy"], 700), (st["completeness"], 500)):
        assert (d["queries"], d["matched"], d["unmatched"], d["within"], d["s1"], d["s2"]) == (queries, 0, queries, 0, 0, 0) and not any(d["histogram"])
        assert (d["mean_m"], d["rms_m"], d["fraction_within"]) == (0.0, 0.0, 0.0)
    assert (st["precision"], st["recall"], st["f_score"]) == (0.0, 0.0, 0.0)
    # the store itself as the reference
    dc.set_reference(g[:, :3])
    want, _ = _check_all(dc, g, g[:, :3])
    for dist, index in (dc.nearest_in_reference(REACH), dc.nearest_in_store(REACH)):
        assert (_bits(dist) == 0).all() and np.array_equal(index, np.arange(700))
    assert (want["precision"], want["recall"], want["f_score"]) == (1.0, 1.0, 1.0) and want["accuracy"]["histogram"][0] == 700
    dc.close()


# ---- 5. D0: invalid rows, the transform ------------------------------------------------------------------------------------------------------------
def test_invalid_reference_rows_keep_their_numbers_and_are_never_matched(opt):
    rng = np.random.default_rng(31)
    xyz = ng._one_per_voxel(rng, 500, VOXEL, 10)
    dc, _ = ng._still_cloud(opt, xyz, VOXEL)
    g, _ = dc.retained()
    ref = np.zeros((400, 5), f32)  # stride 5: two floats per row are not coordinates
    ref[:, :3], ref[:, 3:] = _cloud_near(rng, g, 400), np.nan
    limit = f32(VOXEL) * f32(2**20)
    bad = {0: [np.nan, 0.1, 0.1], 5: [0.1, np.inf, 0.1], 63: [0.1, 0.1, -np.inf], 64: [limit, 0.1, 0.1], 200: [0.1, -2 * limit, 0.1], 399: [1e30, 1e30, 1e30]}
    for row, v in bad.items():
        ref[row, :3] = v
    ref[7, :3] = g[3, :3]  # a valid row next to them, on a store row
    dc.set_reference(ref)
    back, valid = dc.reference()
    want_valid = dm.valid_rows(ref[:, :3], VOXEL)
    assert np.array_equal(_bits(back), _bits(ref[:, :3])) and np.array_equal(valid, want_valid) and np.flatnonzero(valid == 0).tolist() == sorted(bad)
    part, pv = dc.reference(60, 10)
    assert np.array_equal(_bits(part), _bits(ref[60:70, :3])) and np.array_equal(pv, want_valid[60:70])
    want, (a_d2, a_idx, c_d2, c_idx) = _check_all(dc, g, ref[:, :3], want_valid)
    dc.close()
    assert want["ref_invalid"] == 6 and want["completeness"]["queries"] == 394 and not np.isin(a_idx, sorted(bad)).any() and a_idx[3] == 7
    assert (c_idx[sorted(bad)] == -1).all() and np.isnan(c_d2[sorted(bad)]).all()


def test_the_transform_is_rule_5_in_float(opt):
    rng = np.random.default_rng(41)
    xyz = ng._one_per_voxel(rng, 600, VOXEL, 12, corner=(1.0, -0.5, 0.2))
    dc, _ = ng._still_cloud(opt, xyz, VOXEL)
    g, _ = dc.retained()
    a = 0.5235987755982988
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    t = np.array([0.37, -1.21, 0.05])
    T = np.concatenate([R, t[:, None]], axis=1)
    raw = ((_cloud_near(rng, g, 500, 0.05).astype(np.float64) - t) @ R).astype(f32)  # the reference in a frame of its own
    dc.set_reference(raw, T)
    want_ref = dm.transform(raw, T)
    back, valid = dc.reference()
    assert np.array_equal(_bits(back), _bits(want_ref)) and valid.all() and not np.array_equal(_bits(back), _bits(raw))
    want, _ = _check_all(dc, g, want_ref)
    assert want["accuracy"]["matched"] > 300
    T4 = np.eye(4)
    T4[:3] = T
    dc.set_reference(raw, T4)  # a 4x4: its upper rows
    assert np.array_equal(_bits(dc.reference()[0]), _bits(want_ref))
    dc.close()


# ---- 6. classify, remove, staleness --------------------------------------------------------------------------------------------------------------------
def test_remove_by_reference_compacts_the_store_and_everything_else_goes_stale(opt, tmp_path):
    import test_gpu_dense_outliers as og
    from dmsa_lidar_slam_amd.dense_cloud import DenseCarveConfig

    no_mask, no_dist = "no classification of the store as it stands", "no distances of the store as it stands"
    reach, tol = 0.5, 0.1
    dc, _ = ng._creator(opt, lidar_to_imu=base.L2I, voxel_size=0.1, min_range=0.5)
    for xyz, t in og._wall_scans(np.random.default_rng(9)):
        dc.add_scan(xyz, t)
    g, o = dc.retained()
    from scipy.spatial import cKDTree

    crowd = np.array([len(v) for v in cKDTree(g[:, :3]).query_ball_point(g[:, :3], 0.3)])
    wall = g[crowd >= 12, :3]
    ref = (wall[::2] + np.random.default_rng(2).uniform(-0.03, 0.03, (wall[::2].shape[0], 3))).astype(f32)  # half of the wall, none of the strays
    _refused(dc.remove_by_reference, no_mask)
    _refused(lambda: dc.compare(reach, tol), "no reference cloud")
    dc.set_reference(ref)
    _refused(dc.remove_by_reference, no_mask)
    _refused(lambda: dc.save_pcd_distance(tmp_path / "no.pcd"), no_dist)
    valid = np.ones(ref.shape[0], np.uint8)
    for keep in ("far", "near"):
        want, want_flags, d2 = dm.classify(g, ref, valid, reach, tol, keep)
        got, flags = dc.classify_by_reference(reach, tol, keep, download=True)
        _stats_equal(got, want)
        assert flags.dtype == np.uint8 and np.array_equal(flags, want_flags)
        _stats_equal(dc.classify_by_reference(reach, tol, keep), want)
    assert 50 < want["kept"] < g.shape[0] - 50
    assert dc.save_pcd_distance(tmp_path / "d.pcd")[0] == g.shape[0]
    assert open(tmp_path / "d.pcd", "rb").read() == dm.file_bytes(g, dm.dist_of(d2))
    # a scan added after classify: the reference stays, distances and mask are stale
    far = np.zeros((50, 4), f32)
    far[:, 0], far[:, 1:3] = 6.0, np.random.default_rng(1).uniform(3.0, 4.0, (50, 2))
    extra, _ = dc.add_scan(far, np.linspace(base.S[4], base.S[5], 50))
    assert extra.shape[0] > 10
    _refused(dc.remove_by_reference, no_mask)
    _refused(lambda: dc.save_pcd_distance(tmp_path / "no.pcd"), no_dist)
    assert not (tmp_path / "no.pcd").exists() and dc.reference_count() == ref.shape[0] and np.array_equal(_bits(dc.reference()[0]), _bits(ref))
    g, o = dc.retained()
    _stats_equal(dc.compare(reach, tol), dm.compare(g, ref, valid, reach, tol)[0])
    # everything the other stages keep of the store, then this stage's classification and removal
    dc.compute_normals(radius=0.3, download=False)
    dc.cluster_labels(0.3)
    dc.classify_clusters(0.3, 5)
    dc.classify_outliers(0.4, 8, 1.0)
    dc.count_passes(DenseCarveConfig())
    want, want_flags, d2 = dm.classify(g, ref, valid, reach, tol, "near")
    _stats_equal(dc.classify_by_reference(reach, tol, "near"), want)
    slots, occupied = dc.table_info()
    before = dc.stats()
    keep = want_flags.astype(bool)
    assert dc.remove_by_reference() == want["kept"] == int(keep.sum()) == dc.retained_count() < g.shape[0]
    g2, o2 = dc.retained()
    assert np.array_equal(_bits(g2), _bits(g[keep])) and np.array_equal(_bits(o2), _bits(o[keep]))
    assert dc.table_info() == (slots, occupied) and dc.stats() == before  # D6: the voxel set and the scan statistics are untouched
    _refused(lambda: dc.save_pcd_distance(tmp_path / "no.pcd"), no_dist)
    _refused(dc.remove_by_reference, no_mask)
    _refused(lambda: dc.save_pcd_normals(tmp_path / "no.pcd"), "no normals since the last added scan")
    _refused(lambda: dc.save_pcd_labels(tmp_path / "no.pcd"), "no labels of the store as it stands")
    _refused(dc.remove_clusters, no_mask)
    _refused(dc.remove_outliers, no_mask)
    _refused(dc.remove_transients, "no pass counts of the store as it stands")
    assert not (tmp_path / "no.pcd").exists()
    # the reference survived, and the grid is rebuilt over the smaller store: a second compare() equals the model on it
    assert dc.reference_count() == ref.shape[0] and np.array_equal(_bits(dc.reference()[0]), _bits(ref))
    want2, _ = _check_all(dc, g2, ref, reach=reach, tol=tol)
    assert want2["precision"] == 1.0 and want2["rows"] == want["kept"]
    # a new reference makes the distances stale as well; an empty one drops it
    dc.set_reference(ref[:10])
    _refused(lambda: dc.save_pcd_distance(tmp_path / "no.pcd"), no_dist)
    dc.set_reference(np.zeros((0, 3), f32))
    assert dc.reference_count() == 0
    _refused(lambda: dc.compare(reach, tol), "no reference cloud")
    dc.close()


def test_the_intensity_travels_and_the_file_is_the_same_bytes_on_every_run(opt, tmp_path):
    from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator

    rng = np.random.default_rng(27)
    xyz = ng._one_per_voxel(rng, 900, VOXEL, 24, corner=(-0.6, -0.6, 0.2))
    rows = np.concatenate([xyz, np.arange(900, dtype=f32)[:, None] + f32(0.5)], axis=1).astype(f32)
    ref = _cloud_near(rng, rows[rows[:, 0] < 0.0], 700, 0.1)  # one half of the cube: the rows deep in the other half match nothing
    valid = np.ones(700, np.uint8)
    s, p, q = base._still_trajectory()
    files = []
    for intensity in (True, False):
        for reserve in (0, 5000):
            dc = DenseCloudCreator(s, p, q, DenseCloudConfig(voxelSize=VOXEL), optimizer=opt, retain=True, intensity=intensity)
            if reserve:
                dc.reserve(reserve)
            kept, _ = dc.add_scan(rows if intensity else rows[:, :3], ng._stamps(900))
            g, o = dc.retained()
            assert kept.shape[0] == 900
            dc.set_reference(ref)
            want, want_flags, d2 = dm.classify(g, ref, valid, REACH, TOL, "far")
            _stats_equal(dc.classify_by_reference(REACH, TOL, "far"), want)
            path = tmp_path / f"d{int(intensity)}{reserve}.pcd"
            points, nbytes = dc.save_pcd_distance(path)
            raw = open(path, "rb").read()
            assert raw == dm.file_bytes(g, dm.dist_of(d2), intensity) and (points, nbytes) == (900, len(raw)) and np.isnan(d2).any()
            files.append(raw)
            assert dc.remove_by_reference() == want["kept"] and 0 < want["kept"] < 900
            g2, o2 = dc.retained()
            keep = want_flags.astype(bool)
            assert np.array_equal(_bits(g2), _bits(g[keep])) and (not intensity or np.array_equal(g2[:, 3], rows[keep, 3])) and (o2[:, 3] == 1).all()
            dc.close()
    assert files[0] == files[1] and files[2] == files[3] and len(files[0]) > len(files[2])
    # the library reads its own file back
    from dmsa_lidar_slam_amd.dense_cloud import read_pcd_xyz

    assert np.array_equal(_bits(read_pcd_xyz(tmp_path / "d10.pcd")), _bits(rows[:, :3]))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_every_breach_of_d0_d1_and_d7_is_refused_with_its_reason(opt, tmp_path):
    from dmsa_lidar_slam_amd import _capi as capi

    rng = np.random.default_rng(51)
    ref = rng.uniform(0, 0.5, (50, 3)).astype(f32)
    off, _ = ng._creator(opt, retain=False, still=True, voxel_size=VOXEL)
    off.add_scan(np.full((1, 3), 0.5, f32), ng._stamps(1))
    off.set_reference(ref)  # a reference needs no store
    for call in (lambda: off.compare(REACH, TOL), lambda: off.nearest_in_reference(REACH), lambda: off.nearest_in_store(REACH), lambda: off.classify_by_reference(REACH, TOL),
                 off.remove_by_reference, lambda: off.save_pcd_distance(tmp_path / "x.pcd")):
        _refused(call, "retention is off" if call != off.remove_by_reference else "no classification of the store as it stands")
    off.close()
    empty, _ = ng._creator(opt, still=True, voxel_size=VOXEL)
    empty.set_reference(ref)
    _refused(lambda: empty.compare(REACH, TOL), "no retained point")
    _refused(lambda: empty.save_pcd_distance(tmp_path / "x.pcd"), "no retained point to write")
    empty.close()
    unthinned, _ = ng._creator(opt, still=True, voxel_size=0.0)
    unthinned.add_scan(np.full((1, 3), 0.5, f32), ng._stamps(1))
    _refused(lambda: unthinned.set_reference(ref), "voxel_size must be > 0")
    unthinned.close()
    dc, _ = ng._still_cloud(opt, ng._one_per_voxel(rng, 100, VOXEL, 8), VOXEL)
    lib, handle = dc._lib, dc._dc
    # D0
    assert lib.dmsa_dense_cloud_set_reference(handle, capi.ptr(ref, C.c_float), 50, 2, None) == -1
    assert b"stride_floats must be at least 3" in lib.dmsa_last_error(opt._ctx)
    assert lib.dmsa_dense_cloud_set_reference(handle, capi.ptr(ref, C.c_float), 2**26 + 1, 3, None) == -1
    assert b"more than 2^26 reference rows" in lib.dmsa_last_error(opt._ctx)
    assert lib.dmsa_dense_cloud_set_reference(handle, None, 5, 3, None) == -1 and lib.dmsa_dense_cloud_set_reference(handle, capi.ptr(ref, C.c_float), -1, 3, None) == -1
    T = np.eye(4)[:3].copy()
    T[1, 3] = np.inf
    _refused(lambda: dc.set_reference(ref, T), "the transform is not finite")
    _refused(lambda: dc.compare(REACH, TOL), "no reference cloud")
    _refused(lambda: dc.reference(0, 1), "rows beyond the reference cloud")
    dc.set_reference(np.full((4, 3), np.nan, f32))
    assert dc.reference_count() == 4
    _refused(lambda: dc.compare(REACH, TOL), "the reference cloud has no valid row")
    dc.set_reference(ref)
    # D1
    for reach, text in ((np.nan, "max_distance is not finite"), (np.inf, "max_distance is not finite"), (0.04, "max_distance must lie in [voxel_size, 64 * voxel_size]"),
                        (3.3, "max_distance must lie in [voxel_size, 64 * voxel_size]")):
        _refused(lambda: dc.compare(reach, 0.04), text)
        _refused(lambda: dc.nearest_in_reference(reach), text)
    for tol, text in ((0.0, "tolerance must lie in (0, max_distance]"), (-0.1, "tolerance must lie in (0, max_distance]"), (0.3, "tolerance must lie in (0, max_distance]"),
                      (np.nan, "tolerance is not finite"), (np.inf, "tolerance is not finite")):
        _refused(lambda: dc.compare(REACH, tol), text)
        _refused(lambda: dc.classify_by_reference(REACH, tol), text)
    assert dc.compare(REACH, REACH)["rows"] == 100  # tolerance == max_distance is legal
    _refused(lambda: dc.nearest_in_reference(REACH, 50, 51), "rows beyond the retained store")
    _refused(lambda: dc.nearest_in_store(REACH, 50, 1), "rows beyond the reference cloud")
    cfg = capi.DenseCompareConfig(0.2, 0.05, 2, 0)
    assert lib.dmsa_dense_cloud_classify_by_reference(handle, C.byref(cfg), None, None) == -1 and b"keep must be DMSA_COMPARE_KEEP_NEAR" in lib.dmsa_last_error(opt._ctx)
    with pytest.raises(ValueError):
        dc.classify_by_reference(REACH, TOL, keep="both")
    # D7: a stage call over a part of the rows leaves no distances of the store; a path that cannot be written leaves no file
    dc.nearest_in_reference(REACH, 0, 50)
    _refused(lambda: dc.save_pcd_distance(tmp_path / "y.pcd"), "no distances of the store as it stands")
    dc.nearest_in_reference(REACH)
    assert dc.save_pcd_distance(tmp_path / "y.pcd")[0] == 100
    before = sorted(os.listdir(tmp_path))
    _refused(lambda: dc.save_pcd_distance(tmp_path), "cannot open")
    _refused(lambda: dc.save_pcd_distance(tmp_path / "no" / "such" / "dir.pcd"), "cannot open")
    assert sorted(os.listdir(tmp_path)) == before and not (tmp_path / "x.pcd").exists()
    dc.close()


# ---- 8. the programs ----------------------------------------------------------------------------------------------------------------------------------
def test_the_cpp_example_compares_a_cloud_with_the_file_it_wrote_a_moment_earlier(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import dense_cloud_demo

    r = dense_cloud_demo.run(scans=6, workdir=str(tmp_path), clusters=(0.3, 20))
    exe = os.path.join(ROOT, "examples", "dense_cloud_from_raw")
    first, out, dist = tmp_path / "first.pcd", tmp_path / "second.pcd", tmp_path / "dist.pcd"
    args = [exe, r["dump"], r["poses_file"], "ouster", "OUT", "--voxel", "0.1", "--min-range", "0.5", "--cluster-min", "20", "--cluster-radius", "0.3"]
    p = subprocess.run([str(first) if a == "OUT" else a for a in args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
    p = subprocess.run([str(out) if a == "OUT" else a for a in args] + ["--compare", str(first), "--compare-out", str(dist)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
    line = re.search(r"^compare: .*$", p.stdout, re.M).group(0)
    num = lambda name: float(re.search(rf"\b{name} ([0-9.]+)", line).group(1))
    rows = int(num("rows"))
    assert rows == r["clusters_points"] > 1000 and num("ref_rows") == rows and num("ref_invalid") == 0 and num("matched") == num("ref_matched") == num("within") == rows
    assert num("unmatched") == 0 and (num("mean"), num("rms"), num("ref_mean"), num("ref_rms")) == (0, 0, 0, 0) and (num("precision"), num("recall"), num("f_score")) == (1, 1, 1)
    assert open(first, "rb").read() == open(out, "rb").read()
    raw = open(dist, "rb").read()
    xyz = np.frombuffer(open(first, "rb").read()[-12 * rows :], "<f4").reshape(rows, 3)
    assert raw == dm.file_bytes(xyz, np.zeros(rows, f32))
    # the near side of a self-comparison is everything; a reference that is no PCD is refused by the reader's own reason
    p = subprocess.run([str(out) if a == "OUT" else a for a in args] + ["--compare", str(first), "--compare-keep", "near"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and f"keep near: {rows} rows left" in p.stdout
    p = subprocess.run([str(tmp_path / "no.pcd") if a == "OUT" else a for a in args] + ["--compare", r["poses_file"]], capture_output=True, text=True, timeout=300)
    assert p.returncode == 1 and "pcd read: " in p.stderr and not (tmp_path / "no.pcd").exists()


def test_the_demo_compares_with_a_reference_file(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import dense_cloud_demo

    r = dense_cloud_demo.run(scans=6, workdir=str(tmp_path))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dense_cloud_demo.py"), "--scans", "6", "--compare", r["pcd"], "--compare-out", str(tmp_path / "Dist.pcd"),
                        "--out", str(tmp_path / "Dense2.pcd")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = re.search(r"^compare .*$", p.stdout, re.M).group(0)
    assert f"rows {r['points']} " in line and f"matched {r['points']} " in line and "f_score 1.000000" in line
    raw = open(tmp_path / "Dist.pcd", "rb").read()
    assert raw.startswith(dm.header(r["points"]).encode()) and not np.frombuffer(raw[-16 * r["points"] :], "<f4").reshape(-1, 4)[:, 3].any()
