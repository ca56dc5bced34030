"""GPU tests of include/dmsa_dense_outliers.h against the numpy model of O2-O5 (tests/dense_outliers_model.py).

Mean distances: k_knn_mean_distance against the brute-force model BIT FOR BIT, NaNs included -- a candidate missed at a cell face or a tile
seam, the row itself taken as its own neighbour, or a list that loses an entry at a tie changes a float.  Classification: the flags and all
ten statistics fields equal the model's (the sums are integers, O5 is the same double arithmetic on both sides).  Removal: the store and the
origins afterwards are the model's inliers bit for bit and in order, and the normals afterwards are those of the filtered cloud.

The kernel walks the search grid like k_neighbour_moments (tiles of 64 candidates, a wave of 64 queries; csrc/dense_grid_walk.h), so the shapes
are those of tests/test_gpu_dense_normals.py, whose cloud builders are reused; it is instantiated for list capacities 4, 8 and 16, and
k = 1, 5, 16 takes each of them.

The files of the store are written in chunks of 2^20 rows through two slots (csrc/copy_back.h): stores of 2^20 + 1 and of 2 * 2^20 + 3 rows
reach the second chunk and the first reuse of a slot with real rows, and one object has all three writers of the library at work at once.

Not tested here: the O1 bound of 2^26 retained rows (a store of 2 GiB)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dense_normals_model as nm
import dense_outliers_model as om
import test_gpu_dense_cloud as base
import test_gpu_dense_normals as ng

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL, RADIUS = ng.VOXEL, ng.RADIUS
KS = (1, 5, 16)
_bits = ng._bits


@pytest.fixture(scope="module")
def opt():
    from dmsa_lidar_slam_amd.api import DmsaOptimizer

    o = DmsaOptimizer(device=0)
    yield o
    o.close()


def _same_floats(got, ref):
    bad = np.flatnonzero(_bits(got) != _bits(ref))
    assert got.shape == ref.shape and bad.size == 0, (bad[:10], got[bad[:5]], ref[bad[:5]])


def _check_knn(dc, g, radius, ks=KS):
    """knn_mean_distance for every k against the model; returns the model's values per k."""
    out = {}
    for k in ks:
        ref = om.knn_mean_distance(g, radius, k)
        got = dc.knn_mean_distance(radius, k)
        assert got.dtype == f32
        _same_floats(got, ref)
        out[k] = ref
    return out


# ---- 1. every total, every capacity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [1, 2, 5, 6, 16, 17])
def test_knn_in_a_cluster_of_k_and_of_k_plus_one_rows(opt, total):
    """All rows within reach of each other (a cube of three voxels, radius five voxels): with `total` rows every row has total - 1 candidates,
    so k = total isolates every row and k = total - 1 none."""
    rng = np.random.default_rng(100 + total)
    radius = 0.25
    xyz = ng._one_per_voxel(rng, total, VOXEL, 3, corner=(0.4, -0.2, 1.0))
    dc, kept = ng._still_cloud(opt, xyz, VOXEL)
    g, _ = dc.retained()
    assert kept.shape[0] == total
    ref = _check_knn(dc, g, radius)
    dc.close()
    for k in KS:
        assert np.isnan(ref[k]).all() if k >= total else (ref[k] > 0).all(), (k, total)


@pytest.mark.parametrize("total", [63, 64, 65, 257, 4097])
def test_knn_at_every_total(opt, total):
    rng = np.random.default_rng(total)
    side = 12 if total < 300 else 32
    xyz = ng._one_per_voxel(rng, total, VOXEL, side, corner=(-0.3, -0.3, -0.3))
    dc, kept = ng._still_cloud(opt, xyz, VOXEL)
    assert kept.shape[0] == total == dc.retained_count()
    g, _ = dc.retained()
    ref = _check_knn(dc, g, RADIUS)
    dc.close()
    assert not np.isnan(ref[1]).all() and (total < 257 or not np.isnan(ref[16]).all())


# ---- 2. hand-placed rows, windows -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(opt):
    """The cloud of the normals' tests: random rows (about 30 candidates each) with the hand-placed rows of ng._hand_placed mixed in."""
    rng = np.random.default_rng(31)
    hand, tags = ng._hand_placed()
    rand = ng._one_per_voxel(rng, 2600, VOXEL, 30, corner=(-0.75, -0.75, -0.75))
    xyz = np.concatenate([rand, hand])
    order = rng.permutation(xyz.shape[0])
    dc, kept = ng._still_cloud(opt, xyz[order], VOXEL)
    g, o = dc.retained()
    where = np.empty(xyz.shape[0], np.int64)
    where[order] = np.arange(xyz.shape[0])
    assert g.shape[0] == xyz.shape[0]

    def rows(name):
        a, k = tags[name]
        return where[rand.shape[0] + a : rand.shape[0] + a + k]

    yield dict(dc=dc, g=g, o=o, rows=rows, n_rand=rand.shape[0])
    dc.close()


def test_hand_placed_rows_equal_the_model(mixed):
    dc, g, rows = mixed["dc"], mixed["g"], mixed["rows"]
    r = f32(RADIUS)
    ref = _check_knn(dc, g, RADIUS, ks=(1, 2, 3, 4, 5, 16))
    # a candidate at d2 == r2 is one, a candidate one ulp of r further is none
    e0, e1, e2 = rows("edge")
    assert ref[1][e0] == r and ref[1][e1] == r and np.isnan(ref[1][e2]) and np.isnan(ref[2][e0])
    assert np.isnan(ref[1][rows("isolated")[0]])
    # exactly k - 1 and exactly k candidates
    assert np.isnan(ref[4][rows("four")]).all() and not np.isnan(ref[3][rows("four")]).any()
    assert not np.isnan(ref[4][rows("five")]).any() and np.isnan(ref[5][rows("five")]).all()
    # the query with a neighbour in each of the 27 cells: 26 candidates, all at most 0.55 sqrt(3) r away
    q27 = rows("all27")[0]
    assert not np.isnan(ref[16][q27]) and ref[16][q27] < r
    # rows on cell faces
    assert not np.isnan(ref[1][rows("faces")]).any()
    assert 0.0 < np.isnan(ref[16]).mean() < 0.5


def test_row_ranges_that_cut_a_wave(mixed):
    dc, g = mixed["dc"], mixed["g"]
    n = g.shape[0]
    ref = om.knn_mean_distance(g, RADIUS, 5)
    for first, count in ((0, 1), (1, 1), (n - 1, 1), (n // 3, 700), (n - 65, 65), (63, 130), (31, 64), (0, 0)):
        win = dc.knn_mean_distance(RADIUS, 5, first, count)
        assert win.shape == (count,)
        _same_floats(win, ref[first : first + count])
    # another radius on the same object: the grid is rebuilt
    _same_floats(dc.knn_mean_distance(0.11, 1, 100, 300), om.knn_mean_distance(g, 0.11, 1, rows=np.arange(100, 400)))


# ---- 3. shapes of the grid -----------------------------------------------------------------------------------------------------------------------------
def test_a_lattice_with_equal_distances_at_the_kth_place(opt):
    """Points on exact voxel centres (voxel 2^-4: every coordinate and every d2 is exact): 6 candidates at distance 1 voxel, 12 at sqrt 2, 8 at
    sqrt 3: the 5-th and the 16-th smallest are tied with their successors."""
    rng = np.random.default_rng(8)
    voxel, radius = 0.0625, 0.2
    idx = np.stack(np.meshgrid(*[np.arange(-5, 5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    idx = idx[rng.permutation(idx.shape[0])[:880]]
    xyz = ((idx + 0.5) * voxel).astype(f32)
    dc, kept = ng._still_cloud(opt, xyz, voxel)
    g, _ = dc.retained()
    assert kept.shape[0] == 880
    ref = _check_knn(dc, g, radius)
    dc.close()
    inner = (np.abs(idx + 0.5) < 3).all(axis=1)
    assert len(np.unique(ref[5][inner & ~np.isnan(ref[5])])) < 40  # a handful of distinct means: the distances repeat
    assert not np.isnan(ref[16][inner]).all()


def test_one_cell_with_more_rows_than_a_wave_and_many_tiles(opt):
    rng = np.random.default_rng(5)
    voxel, radius = 0.01, f32(0.01) * f32(64.0)
    n = 1500
    xyz = ng._one_per_voxel(rng, n, voxel, 60, corner=(0.02, 0.02, 0.02))
    assert len({tuple(c) for c in np.floor(xyz / radius).astype(int)}) == 1
    dc, kept = ng._still_cloud(opt, xyz, voxel)
    assert kept.shape[0] == n
    g, _ = dc.retained()
    ref = _check_knn(dc, g, float(radius))
    dc.close()
    assert not np.isnan(ref[16]).any()


def _sparse_cells(rng):
    r = f32(RADIUS)
    cells = np.stack(np.meshgrid(np.arange(-3, 3), np.arange(-3, 3), np.arange(-3, 3), indexing="ij"), axis=-1).reshape(-1, 3)[:200] * 2
    first = (cells + rng.uniform(0.1, 0.4, (200, 3))) * float(r)
    second = first[::2] + rng.uniform(0.3, 0.5, (100, 3)) * float(r)
    xyz = np.concatenate([first, second]).astype(f32)
    return xyz[rng.permutation(xyz.shape[0])]


def test_two_hundred_cells_of_one_or_two_rows(opt):
    """Cells two apart, a second row in every other one: a third of the rows is isolated at k = 1, and all of them at k = 2, where n_s and T
    are 0 and every row is an outlier."""
    xyz = _sparse_cells(np.random.default_rng(6))
    dc, kept = ng._still_cloud(opt, xyz, VOXEL)
    assert kept.shape[0] == 300
    g, _ = dc.retained()
    ref = _check_knn(dc, g, RADIUS, ks=(1, 2))
    for k in (1, 2):
        want_flags, want, _ = om.classify(g, RADIUS, k, 1.0)
        got, flags = dc.classify_outliers(RADIUS, k, 1.0, download=True)
        assert got == want and np.array_equal(flags, want_flags)
    assert 0 < want["rows"] == want["isolated"] and want["n_s"] == 0 and want["threshold_m"] == 0.0 and not want_flags.any()
    assert 0 < (~np.isnan(ref[1])).sum() <= 200
    assert dc.remove_outliers() == 0 and dc.retained_count() == 0  # every row was an outlier: the store is empty
    dc.close()


def _wave_box_cells(g, radius):
    """Cells of the box around every 64 consecutive rows of the sorted order (cells of edge 1.001 radius cut in double, rows sorted by cell)."""
    c = np.floor(g[:, :3].astype(np.float64) / (1.001 * float(f32(radius)))).astype(np.int64)
    order = np.lexsort((c[:, 2], c[:, 1], c[:, 0]))
    c = c[order]
    return np.array([np.prod(c[a : a + 64].max(axis=0) - c[a : a + 64].min(axis=0) + 3) for a in range(0, c.shape[0], 64)])


def test_sorted_order_that_jumps_between_distant_surfaces(opt):
    """120 small clusters and 150 lone rows scattered over 10 m: 64 consecutive sorted rows lie in clusters far apart, the box of a wave exceeds
    kGridBoxCells and the wave goes through its distinct cells one by one."""
    rng = np.random.default_rng(12)
    centres = rng.uniform(-5, 5, (120, 3))
    xyz = np.concatenate([c + ng._one_per_voxel(rng, 30, VOXEL, 4) for c in centres] + [rng.uniform(-5, 5, (150, 3))]).astype(f32)
    xyz = xyz[rng.permutation(xyz.shape[0])]
    dc, kept = ng._still_cloud(opt, xyz, VOXEL)
    g, _ = dc.retained()
    boxes = _wave_box_cells(g, RADIUS)
    assert g.shape[0] > 3000 and (boxes > 512).mean() > 0.9
    ref = _check_knn(dc, g, RADIUS)
    dc.close()
    assert 0.02 < np.isnan(ref[5]).mean() < 0.2 and not np.isnan(ref[16]).all()


# ---- 4. classification ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,mul", [(8, 1.0), (8, 0.0), (5, 1e6), (16, 2.5), (1, 0.5)])
def test_classify_equals_the_model_in_flags_and_all_ten_fields(mixed, k, mul):
    dc, g = mixed["dc"], mixed["g"]
    want_flags, want, _ = om.classify(g, RADIUS, k, mul)
    got, flags = dc.classify_outliers(RADIUS, k, mul, download=True)
    assert list(got) == list(want) and len(got) == 10
    assert got == want, [(n, got[n], want[n]) for n in got if got[n] != want[n]]
    assert flags.dtype == np.uint8 and np.array_equal(flags, want_flags)
    assert dc.classify_outliers(RADIUS, k, mul) == want  # without the flags: the dict alone
    assert got["rows"] == g.shape[0] == got["isolated"] + got["above_threshold"] + got["inliers"] and got["n_s"] == got["rows"] - got["isolated"]
    if mul == 1e6:
        assert got["above_threshold"] == 0 and got["inliers"] == got["n_s"]
    else:
        assert got["above_threshold"] > 0 and got["inliers"] > 0


def test_a_row_with_q_equal_to_the_threshold_is_an_inlier(opt):
    """stddev_mul = 0: T is the mean.  (a) k = 2, rectangles of 2 x 3 voxels: every corner's two nearest rows are one at each of the two side
    lengths, every m_i is their mean, every q_i equals T.  (b) k = 1, pairs at 2, 4 and 3 voxels in equal numbers: T is q of the pairs at 3."""
    voxel, radius = 0.0625, 0.25  # exact coordinates, exact d2, exact square roots
    scale = float(om.scale_of(radius))
    rect = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0], [2, 3, 0]], np.float64)
    xyz = np.concatenate([(rect + [20 * i, 0, 7]) * voxel for i in range(5)]).astype(f32)
    dc, kept = ng._still_cloud(opt, xyz, voxel)
    g, _ = dc.retained()
    assert kept.shape[0] == 20
    want_flags, want, m = om.classify(g, radius, 2, 0.0)
    assert (m == f32(2.5 * voxel)).all() and want["stddev_m"] == 0.0 and want["threshold_m"] * scale == 2.5 * voxel * scale and want_flags.all()
    got, flags = dc.classify_outliers(radius, 2, 0.0, download=True)
    dc.close()
    assert got == want and flags.all() and got["inliers"] == 20

    pairs = []
    for i, d in enumerate((2, 4, 3, 2, 4, 3)):
        pairs += [[20 * i, 5, 7], [20 * i + d, 5, 7]]  # (away from the origin: a point at range 0 does not pass rule 2)
    xyz = (np.array(pairs, np.float64) * voxel).astype(f32)
    dc, kept = ng._still_cloud(opt, xyz, voxel)
    g, _ = dc.retained()
    assert kept.shape[0] == 12
    want_flags, want, m = om.classify(g, radius, 1, 0.0)
    q = om.quantise(m, radius)
    assert want["threshold_m"] * scale == 3 * voxel * scale and sorted(set(q)) == [int(2 * voxel * scale), int(3 * voxel * scale), int(4 * voxel * scale)]
    assert np.array_equal(want_flags, (q <= int(3 * voxel * scale)).astype(np.uint8)) and want["inliers"] == 8 and want["above_threshold"] == 4
    got, flags = dc.classify_outliers(radius, 1, 0.0, download=True)
    dc.close()
    assert got == want and np.array_equal(flags, want_flags)


# ---- 5. removal ---------------------------------------------------------------------------------------------------------------------------------------------
def _wall_scans(rng, scans=3, n=1500, strays=60):
    """A wall 6 m in front of a moving sensor (segment 4 of the trajectory) and strays between the sensor and the wall."""
    out = []
    for _ in range(scans):
        xyz = np.zeros((n + strays, 4), f32)
        xyz[:n, 0], xyz[:n, 1:3] = 6.0 + rng.normal(0, 0.01, n), rng.uniform(-1.5, 1.5, (n, 2))
        xyz[n:, 0], xyz[n:, 1:3] = rng.uniform(3.0, 5.5, strays), rng.uniform(-1.5, 1.5, (strays, 2))
        xyz = xyz[rng.permutation(n + strays)]
        out.append((xyz, np.sort(rng.uniform(base.S[4], base.S[5], n + strays))))
    return out


def test_remove_outliers_compacts_points_and_origins_and_the_normals_follow(opt):
    from dmsa_lidar_slam_amd.api import DmsaError
    from dmsa_lidar_slam_amd.dense_cloud import normal_from_moments

    def refused(call):
        with pytest.raises(DmsaError) as e:
            call()
        assert e.value.status == -1 and "no classification of the store as it stands" in e.value.args[0], e.value.args[0]

    radius, k, mul = 0.4, 8, 1.0
    dc, _ = ng._creator(opt, lidar_to_imu=base.L2I, voxel_size=0.1, min_range=0.5)
    scans = _wall_scans(np.random.default_rng(9))
    for xyz, t in scans:
        dc.add_scan(xyz, t)
    refused(dc.remove_outliers)  # nothing classified yet
    g, o = dc.retained()
    want_flags, want, _ = om.classify(g, radius, k, mul)
    assert g.shape[0] > 1000 and 20 < want["isolated"] + want["above_threshold"] < 0.5 * g.shape[0]
    got, flags = dc.classify_outliers(radius, k, mul, download=True)
    assert got == want and np.array_equal(flags, want_flags)
    # a scan added after classify: remove is refused until classify runs again
    far = np.zeros((50, 4), f32)
    far[:, 0], far[:, 1:3] = 6.0, np.random.default_rng(1).uniform(3.0, 4.0, (50, 2))
    t_far = np.linspace(base.S[4], base.S[5], 50)
    extra, _ = dc.add_scan(far, t_far)
    assert extra.shape[0] > 10
    refused(dc.remove_outliers)
    g, o = dc.retained()
    want_flags, want, _ = om.classify(g, radius, k, mul)
    assert dc.classify_outliers(radius, k, mul) == want
    slots, occupied = dc.table_info()
    before = dc.stats()
    # the removal
    keep = want_flags.astype(bool)
    assert dc.remove_outliers() == want["inliers"] == int(keep.sum()) == dc.retained_count()
    g2, o2 = dc.retained()
    assert np.array_equal(_bits(g2), _bits(g[keep])) and np.array_equal(_bits(o2), _bits(o[keep]))
    assert len(np.unique(o2[:, :3], axis=0)) > 500  # an origin per stamp: the origins moved with their points
    assert dc.table_info() == (slots, occupied) and dc.stats() == before  # O6: the voxel set and the scan statistics are untouched
    refused(dc.remove_outliers)  # the classification was of the store before
    # normals of the cleaned store
    normals, without = dc.compute_normals(radius, 5)
    ref_n = normal_from_moments(nm.moments(g2, radius), nm.view_vectors(g2, o2), 5)
    assert np.array_equal(_bits(normals), _bits(ref_n)) and without == int(np.isnan(ref_n[:, 0]).sum())
    # the first scan again: every point falls in a voxel that is taken, those of the removed rows included
    again, st = dc.add_scan(*scans[0])
    assert again.shape[0] == 0 and st["thinned"] > 1000 and dc.retained_count() == g2.shape[0]
    # a scan elsewhere is appended behind the cleaned rows
    far2 = far.copy()
    far2[:, 1] -= 8.0
    more, _ = dc.add_scan(far2, t_far)
    g3, o3 = dc.retained()
    assert more.shape[0] > 10 and g3.shape[0] == g2.shape[0] + more.shape[0]
    assert np.array_equal(_bits(g3[: g2.shape[0]]), _bits(g2)) and np.array_equal(_bits(g3[g2.shape[0] :]), _bits(more)) and np.array_equal(_bits(o3[: g2.shape[0]]), _bits(o2))
    # ... and the grown store classifies like any other
    want_flags, want, _ = om.classify(g3, radius, k, mul)
    got, flags = dc.classify_outliers(radius, k, mul, download=True)
    assert got == want and np.array_equal(flags, want_flags)
    dc.close()


def _read_xyz(path):
    raw = open(path, "rb").read()
    end = raw.index(b"DATA binary\n") + len(b"DATA binary\n")
    return raw[:end].decode(), np.frombuffer(raw[end:], "<f4").reshape(-1, 3), len(raw)


def test_two_fresh_objects_give_the_same_flags_and_file_bytes_whatever_the_table_size(opt, tmp_path):
    rng = np.random.default_rng(41)
    xyz = ng._one_per_voxel(rng, 3000, VOXEL, 32)
    out = []
    for reserve in (0, 30000):
        dc, _ = ng._still_cloud(opt, xyz, VOXEL, reserve=reserve)
        stats, flags = dc.classify_outliers(RADIUS, 8, 1.0, download=True)
        mean = dc.knn_mean_distance(RADIUS, 8)
        left = dc.remove_outliers()
        path = tmp_path / f"clean{reserve}.pcd"
        points, size = dc.save_pcd_retained(path)
        assert points == left == stats["inliers"] < 3000
        out.append((stats, flags.tobytes(), mean.tobytes(), open(path, "rb").read()))
        dc.close()
    assert out[0] == out[1]


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_breach_of_o1_is_refused_with_its_reason(opt, tmp_path):
    from dmsa_lidar_slam_amd.api import DmsaError

    def refused(call, text):
        with pytest.raises(DmsaError) as e:
            call()
        assert e.value.status == -1 and text in e.value.args[0], e.value.args[0]

    rng = np.random.default_rng(44)
    xyz = ng._one_per_voxel(rng, 100, VOXEL, 8)
    off, _ = ng._creator(opt, retain=False, still=True, voxel_size=VOXEL)
    off.add_scan(xyz, ng._stamps(100))
    for call in (off.classify_outliers, off.knn_mean_distance, off.remove_outliers, lambda: off.save_pcd_retained(tmp_path / "x.pcd")):
        with pytest.raises(DmsaError) as e:
            call()
        assert e.value.status == -1
    refused(off.classify_outliers, "retention is off")
    off.close()
    empty, _ = ng._creator(opt, still=True, voxel_size=VOXEL)
    refused(lambda: empty.classify_outliers(RADIUS), "no retained point")
    refused(lambda: empty.knn_mean_distance(RADIUS), "no retained point")
    refused(lambda: empty.save_pcd_retained(tmp_path / "empty.pcd"), "no retained point")
    assert not (tmp_path / "empty.pcd").exists() and not (tmp_path / "x.pcd").exists()
    empty.close()
    no_voxel, _ = ng._creator(opt, still=True, voxel_size=0.0)
    no_voxel.add_scan(xyz, ng._stamps(100))
    refused(lambda: no_voxel.classify_outliers(RADIUS), "voxel_size must be > 0")
    no_voxel.close()
    dc, _ = ng._still_cloud(opt, xyz, VOXEL)
    for call in (dc.classify_outliers, dc.knn_mean_distance):
        refused(lambda: call(np.inf), "radius is not finite")
        refused(lambda: call(np.nan), "radius is not finite")
        refused(lambda: call(np.nextafter(f32(VOXEL), f32(0))), "[voxel_size, 64 * voxel_size]")
        refused(lambda: call(np.nextafter(f32(64.0) * f32(VOXEL), f32(10))), "[voxel_size, 64 * voxel_size]")
        refused(lambda: call(-1.0), "[voxel_size, 64 * voxel_size]")
        refused(lambda: call(RADIUS, 0), "k must lie in [1, 16]")
        refused(lambda: call(RADIUS, 17), "k must lie in [1, 16]")
        refused(lambda: call(RADIUS, -3), "k must lie in [1, 16]")
    for mul in (-0.5, np.nan, np.inf):
        refused(lambda: dc.classify_outliers(RADIUS, 8, mul), "stddev_mul must be finite and >= 0")
    refused(lambda: dc.knn_mean_distance(RADIUS, 8, 90, 11), "beyond the retained store")
    # a refused call is no classification; the bounds themselves are legal
    refused(dc.remove_outliers, "no classification")
    assert dc.knn_mean_distance(VOXEL, 1).shape == (100,) and dc.classify_outliers(64.0 * VOXEL, 16, 0.0)["rows"] == 100
    dc.close()


# ---- 7. the file ------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_file_of_the_store_is_its_header_and_12_byte_rows(mixed, tmp_path):
    from dmsa_lidar_slam_amd.api import DmsaError
    from dmsa_lidar_slam_amd.dense_cloud import pcdHeaderXyzBinary

    dc, g = mixed["dc"], mixed["g"]
    path = tmp_path / "Retained.pcd"
    points, size = dc.save_pcd_retained(path)
    head, body, file_size = _read_xyz(path)
    assert head == pcdHeaderXyzBinary(g.shape[0])
    assert points == g.shape[0] == body.shape[0] and size == file_size == len(head) + 12 * points
    assert np.array_equal(_bits(body), _bits(g[:, :3]))
    # the path of a directory: refused, nothing left behind
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(DmsaError) as e:
        dc.save_pcd_retained(tmp_path)
    assert e.value.status == -1 and "cannot open" in e.value.args[0] and sorted(os.listdir(tmp_path)) == before
    with pytest.raises(DmsaError):
        dc.save_pcd_retained(tmp_path / "no" / "such" / "dir.pcd")
    assert sorted(os.listdir(tmp_path)) == before
    # the seven-field file of the same object shares the pinned buffers: one after the other, both right
    normals, _ = dc.compute_normals(RADIUS, 5)
    dc.save_pcd_normals(tmp_path / "n.pcd")
    assert dc.save_pcd_retained(path) == (points, size) and np.array_equal(_bits(_read_xyz(path)[1]), _bits(g[:, :3]))
    _, body7, _ = ng._read_pcd7(tmp_path / "n.pcd")
    assert np.array_equal(_bits(body7[:, 3:]), _bits(normals))


FILE_CHUNK = 1 << 20  # kFileChunkRows of csrc/dense_store.cpp


@pytest.mark.parametrize("n,side", [(2 * FILE_CHUNK + 3, 160), (FILE_CHUNK + 1, 128)])
def test_the_files_of_a_store_of_more_than_one_chunk(opt, tmp_path, n, side):
    """Three chunks is the smallest count at which a slot of the copy-back is used again, and its last chunk of 3 rows has a byte count (36, 84)
    that is no multiple of 16; two chunks with a last one of a single row.  The radius is the smallest N1 admits: a row has two other rows in
    reach on average, so with min_neighbours = 3 both kinds of rows, with a normal and without, go through the file."""
    from dmsa_lidar_slam_amd.dense_cloud import pcdHeaderNormalsBinary, pcdHeaderXyzBinary

    dc, kept = ng._still_cloud(opt, ng._one_per_voxel(np.random.default_rng(n), n, VOXEL, side), VOXEL)
    g, _ = dc.retained()
    assert kept.shape[0] == n == g.shape[0] == dc.retained_count()
    path = tmp_path / "Retained.pcd"
    points, size = dc.save_pcd_retained(path)
    head, body, file_size = _read_xyz(path)
    assert head == pcdHeaderXyzBinary(n)
    assert points == n == body.shape[0] and size == file_size == len(head) + 12 * n
    assert np.array_equal(_bits(body), _bits(g[:, :3]))
    normals, without = dc.compute_normals(VOXEL, 3)
    assert normals.shape == (n, 4) and 0 < without < n
    path7 = tmp_path / "Normals.pcd"
    points, size = dc.save_pcd_normals(path7)
    head, body7, file_size = ng._read_pcd7(path7)
    dc.close()
    assert head == pcdHeaderNormalsBinary(n)
    assert points == n == body7.shape[0] and size == file_size == len(head) + 28 * n
    assert np.array_equal(_bits(body7[:, :3]), _bits(g[:, :3])) and np.array_equal(_bits(body7[:, 3:]), _bits(normals))


def test_one_object_with_all_three_writers_interleaved(opt, tmp_path):
    """The streaming file has a scan on its way back while the store is saved and while the context's ASCII writer runs on the same two
    streams: each writer has slots of its own, and every file is what it is when written alone."""
    import ctypes as C

    from dmsa_lidar_slam_amd import _capi as capi
    from dmsa_lidar_slam_amd.dense_cloud import pcdHeaderXyzBinary

    def ascii_file(path, xyz, nrm):
        written = C.c_int64(0)
        rc = opt._lib.dmsa_save_pcd_ascii_ex(opt._ctx, str(path).encode(), capi.ptr(xyz, C.c_float), capi.ptr(nrm, C.c_float), capi.ptr(None, C.c_float), xyz.shape[0], 700,
                                             C.byref(written))
        assert rc == 0 and written.value == os.path.getsize(path) > 0
        return open(path, "rb").read()

    rng = np.random.default_rng(19)
    scans = _wall_scans(rng)
    cloud = np.ascontiguousarray(rng.normal(0, 3, (2500, 4)), f32)  # four chunks of text, the last one short
    nrm = np.ascontiguousarray(rng.normal(0, 1, (2500, 4)), f32)
    dc, _ = ng._creator(opt, lidar_to_imu=base.L2I, voxel_size=0.1, min_range=0.5)
    dc.open_pcd(tmp_path / "Stream.pcd")
    kept = [dc.add_scan(*scans[0])[0], dc.add_scan(*scans[1])[0]]
    # the rows of the second scan are pending
    store_points, store_size = dc.save_pcd_retained(tmp_path / "Store.pcd")
    text_between = ascii_file(tmp_path / "between.pcd", cloud, nrm)
    g2, _ = dc.retained()
    kept.append(dc.add_scan(*scans[2])[0])
    points, size = dc.close_pcd()
    dc.close()
    assert all(k.shape[0] > 0 for k in kept) and sum(k.shape[0] for k in kept) > 1000
    rows = np.concatenate(kept)[:, :3]
    head, body, file_size = _read_xyz(tmp_path / "Stream.pcd")
    assert head == pcdHeaderXyzBinary(rows.shape[0]) and points == rows.shape[0] and size == file_size == len(head) + 12 * points
    assert np.array_equal(_bits(body), _bits(rows))
    head, body, file_size = _read_xyz(tmp_path / "Store.pcd")
    assert head == pcdHeaderXyzBinary(g2.shape[0]) and store_points == g2.shape[0] and store_size == file_size == len(head) + 12 * store_points
    assert np.array_equal(_bits(body), _bits(g2[:, :3])) and np.array_equal(_bits(g2[:, :3]), _bits(rows[: g2.shape[0]]))
    assert text_between == ascii_file(tmp_path / "alone.pcd", cloud, nrm)


# ---- 8. the demo ------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_demo_removes_outliers_then_writes_normals_of_the_inliers(tmp_path):
    out, clean = tmp_path / "Normals.pcd", tmp_path / "Clean.pcd"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dense_cloud_demo.py"), "--scans", "6", "--outliers", "8", "1.0", "--normals", "0.3",
                        "--normals-out", str(out), "--clean-out", str(clean), "--out", str(tmp_path / "Dense.pcd")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    kept = int(re.search(r"\bkept (\d+)", p.stdout).group(1))
    rows, inliers = int(re.search(r"\brows (\d+)", p.stdout).group(1)), int(re.search(r"\binliers (\d+)", p.stdout).group(1))
    head, body, _ = ng._read_pcd7(out)
    fields = dict(line.split(" ", 1) for line in head.splitlines()[1:])
    assert fields["FIELDS"] == "x y z normal_x normal_y normal_z curvature" and int(fields["POINTS"]) == inliers == body.shape[0]
    assert rows == kept > 2000 and 0 < inliers < kept
    _, xyz, _ = _read_xyz(clean)
    assert np.array_equal(_bits(xyz), _bits(body[:, :3]))


def test_the_cpp_example_removes_outliers_like_the_demo(tmp_path):
    """examples/dense_cloud_from_raw on the demo's recording: without a radius argument the x y z file of the cleaned store, byte for byte the
    demo's; with one, seven fields and as many rows."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import dense_cloud_demo

    r = dense_cloud_demo.run(scans=6, workdir=str(tmp_path), outliers=(8, 1.0), outlier_radius=0.3)
    exe = os.path.join(ROOT, "examples", "dense_cloud_from_raw")
    flags = ["--voxel", "0.1", "--min-range", "0.5", "--outlier-k", "8", "--outlier-mul", "1.0", "--outlier-radius", "0.3"]
    out = tmp_path / "cpp_clean.pcd"
    p = subprocess.run([exe, r["dump"], r["poses_file"], "ouster", str(out)] + flags, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
    assert int(re.search(r"\binliers (\d+)", p.stdout).group(1)) == r["outliers"]["inliers"] == r["clean_points"] > 1000
    assert open(out, "rb").read() == open(r["clean_pcd"], "rb").read()
    out7 = tmp_path / "cpp_normals.pcd"
    p = subprocess.run([exe, r["dump"], r["poses_file"], "ouster", str(out7), "0.3"] + flags, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
    head, body, _ = ng._read_pcd7(out7)
    assert body.shape[0] == r["clean_points"] and np.array_equal(_bits(body[:, :3]), _bits(_read_xyz(out)[1]))
    # a k out of range is refused with O1's reason
    p = subprocess.run([exe, r["dump"], r["poses_file"], "ouster", str(tmp_path / "no.pcd"), "--voxel", "0.1", "--outlier-k", "17"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 1 and "k must lie in [1, 16]" in p.stderr and not (tmp_path / "no.pcd").exists()
