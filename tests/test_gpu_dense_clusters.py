"""GPU tests of include/dmsa_dense_clusters.h against the model of C2-C7 (tests/dense_clusters_model.py: cKDTree candidates re-tested in
float32, scipy's connected components).  Every comparison is array_equal: a label is the smallest row of a component and a size its number
of rows, so a pair missed at a cell face or a tile seam, a hook lost in a race or a root that is not the smallest row changes an integer.

k_cluster_link walks the search grid like k_knn_mean_distance (csrc/dense_grid_walk.h), so the shapes are those of
tests/test_gpu_dense_outliers.py and the cloud builders of tests/test_gpu_dense_normals.py are reused.  What is new is the union-find: the
chain (graph diameter 2 999, the longest paths a find can meet), the single cell of 1 500 rows (every lane hooks at one root) and the corner
pair (one edge decides between one cluster and two) aim at it.

Not tested here: the C1 bound of 2^26 retained rows (a store of 2 GiB), and the give-up word of the bounded loops, which no correct build
sets."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dense_carve_model as tm
import dense_clusters_model as cm
import dense_normals_model as nm
import dense_outliers_model as om
import test_gpu_dense_cloud as base
import test_gpu_dense_normals as ng

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL, RADIUS = ng.VOXEL, ng.RADIUS
_bits = ng._bits


@pytest.fixture(scope="module")
def opt():
    from dmsa_lidar_slam_amd.api import DmsaOptimizer

    o = DmsaOptimizer(device=0)
    yield o
    o.close()


def _check_labels(dc, g, radius):
    """cluster_labels against the model; returns the model's (label, size)."""
    want_label, want_size = cm.labels(g, radius)
    label, size = dc.cluster_labels(radius)
    assert label.dtype == np.int32 and size.dtype == np.int32
    assert np.array_equal(label, want_label), (np.flatnonzero(label != want_label)[:10], label[:10], want_label[:10])
    assert np.array_equal(size, want_size), np.flatnonzero(size != want_size)[:10]
    return want_label, want_size


def _check_classify(dc, g, radius, min_size, max_size=0):
    want_flags, want, label, size = cm.classify(g, radius, min_size, max_size)
    got, flags = dc.classify_clusters(radius, min_size, max_size, download=True)
    assert list(got) == list(want) and len(got) == 7
    assert got == want, [(n, got[n], want[n]) for n in got if got[n] != want[n]]
    assert flags.dtype == np.uint8 and np.array_equal(flags, want_flags)
    assert dc.classify_clusters(radius, min_size, max_size) == want  # without the flags: the dict alone
    assert got["rows"] == g.shape[0] == got["kept_rows"] + got["small_rows"] + got["large_rows"]
    return want_flags, want, label, size


def _refused(call, text, status=-1):
    from dmsa_lidar_slam_amd.api import DmsaError

    with pytest.raises(DmsaError) as e:
        call()
    assert e.value.status == status and text in e.value.args[0], e.value.args[0]


# ---- 1. every total -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [1, 2, 63, 64, 65, 257, 4097])
def test_labels_and_sizes_at_every_total(opt, total):
    """At the radius of the other stages' tests most rows join one cluster; at 1.2 voxels a row has about one adjacent row, and the cloud falls
    into clusters of every small size."""
    rng = np.random.default_rng(total)
    side = 3 if total < 3 else 8 if total < 100 else 12 if total < 300 else 32
    xyz = ng._one_per_voxel(rng, total, VOXEL, side, corner=(-0.3, -0.3, -0.3))
    dc, kept = ng._still_cloud(opt, xyz, VOXEL)
    assert kept.shape[0] == total == dc.retained_count()
    g, _ = dc.retained()
    _, size = _check_labels(dc, g, RADIUS)
    label, small = _check_labels(dc, g, 0.06)
    _check_classify(dc, g, 0.06, 3, 6)
    dc.close()
    if total >= 63:
        assert size.max() > total // 2 and len(np.unique(label)) > total // 8 and small.max() >= 3


# ---- 2. the chain -----------------------------------------------------------------------------------------------------------------------------------
def _chain(gap, n=3000, seed=3):
    """n rows along x in shuffled store order: 3/16 m apart (exact in float32 left of x = 0) but for the link in the middle, between x = 0 and
    x = gap.  Returns (xyz, the position of every row along the chain)."""
    rng = np.random.default_rng(seed)
    pos = np.arange(n) - n // 2  # -1500 .. 1499
    x = np.where(pos < 0, f32(0.1875) * (pos + 1).astype(f32), f32(gap) + f32(0.1875) * pos.astype(f32)).astype(f32)
    order = rng.permutation(n)
    xyz = np.zeros((n, 3), f32)
    xyz[:, 0], xyz[:, 1], xyz[:, 2] = x[order], f32(0.3), f32(-0.2)
    return xyz, pos[order]


@pytest.mark.parametrize("link", ["plain", "at_r", "beyond_r"])
def test_a_shuffled_chain_of_3000_rows(opt, link):
    r = f32(RADIUS)
    gap = {"plain": f32(0.1875), "at_r": r, "beyond_r": np.nextafter(r, f32(1))}[link]
    xyz, pos = _chain(gap)
    dc, kept = ng._still_cloud(opt, xyz, VOXEL)
    assert kept.shape[0] == 3000
    g, _ = dc.retained()
    assert np.array_equal(_bits(g[:, :3]), _bits(xyz))
    label, size = _check_labels(dc, g, RADIUS)
    dc.close()
    left = pos < 0
    if link == "beyond_r":  # d2 is one step above r2: two clusters, each labelled by its own smallest row, which lies mid-chain
        assert sorted(set(label)) == sorted({int(np.flatnonzero(left)[0]), int(np.flatnonzero(~left)[0])}) and (size == 1500).all()
        assert len(set(label[left])) == 1 and len(set(label[~left])) == 1
    else:  # at_r: d2 == r2 exactly, which is adjacent
        assert (label == 0).all() and (size == 3000).all() and abs(int(pos[0])) < 1499


# ---- 3. one pair between two blobs -------------------------------------------------------------------------------------------------------------------
def test_two_blobs_joined_by_one_pair_across_a_cell_corner(opt):
    rng = np.random.default_rng(17)
    edge = 1.001 * float(f32(RADIUS))
    c = 3 * edge  # the corner shared by cells (2,2,2) and (3,3,3)
    a, b = np.full(3, c - 0.05), np.full(3, c + 0.05)
    blob_a = ng._one_per_voxel(rng, 300, VOXEL, 8, corner=(0.10, 0.10, 0.10))
    blob_b = ng._one_per_voxel(rng, 300, VOXEL, 8, corner=(0.70, 0.70, 0.70))
    for pair, clusters in ((True, 1), (False, 2)):
        xyz = np.concatenate([blob_a, blob_b] + ([np.array([a, b])] if pair else [])).astype(f32)
        xyz = xyz[np.random.default_rng(5).permutation(xyz.shape[0])]
        dc, kept = ng._still_cloud(opt, xyz, VOXEL)
        assert kept.shape[0] == xyz.shape[0]
        g, _ = dc.retained()
        label, size = _check_labels(dc, g, RADIUS)
        dc.close()
        assert len(set(label)) == clusters and set(size) == ({602} if pair else {300})
    cells = np.floor(np.array([a, b], f32).astype(np.float64) / edge).astype(int)
    assert (cells[0] == 2).all() and (cells[1] == 3).all()
    # the pair is the only edge between the blobs
    pairs = cm.adjacent_pairs(np.concatenate([blob_a, blob_b, [a, b]]).astype(f32), RADIUS)
    crossing = pairs[(pairs[:, 0] < 300) & (pairs[:, 1] >= 300) & (pairs[:, 1] != 600)]
    assert crossing.shape[0] == 0 and ((pairs == [600, 601]).all(axis=1)).sum() == 1


# ---- 4. hand-placed rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(opt):
    """The cloud of the normals' tests: random rows (about 30 adjacent rows each) with the hand-placed rows of ng._hand_placed mixed in."""
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
    label, size = _check_labels(dc, g, RADIUS)
    e0, e1, e2 = rows("edge")
    assert label[e0] == label[e1] == min(e0, e1) and size[e0] == 2  # d2 == r2: adjacent
    assert label[e2] == e2 and size[e2] == 1  # one ulp of r further: not
    iso = rows("isolated")[0]
    assert label[iso] == iso and size[iso] == 1
    q27 = rows("all27")
    assert (label[q27] == q27.min()).all() and (size[q27] == 27).all()
    assert (size[rows("four")] == 4).all() and (size[rows("five")] == 5).all()
    # rows on cell faces, a rounded multiple of r apart: fl(3 r) - fl(2 r) is above r, so the outer columns stand alone
    assert sorted(set(size[rows("faces")])) == [3, 15] and len(set(label[rows("faces")])) == 3
    assert size.max() == mixed["n_rand"]
    # another radius on the same object: the grid is rebuilt and the labels follow
    _check_labels(dc, g, 0.06)
    _check_labels(dc, g, RADIUS)


# ---- 5. shapes of the grid -----------------------------------------------------------------------------------------------------------------------------
def test_one_cell_of_1500_rows_is_one_cluster(opt):
    rng = np.random.default_rng(5)
    voxel, radius = 0.01, f32(0.01) * f32(64.0)
    n = 1500
    xyz = ng._one_per_voxel(rng, n, voxel, 60, corner=(0.02, 0.02, 0.02))
    assert len({tuple(c) for c in np.floor(xyz / radius).astype(int)}) == 1
    dc, kept = ng._still_cloud(opt, xyz, voxel)
    assert kept.shape[0] == n
    g, _ = dc.retained()
    label, size = _check_labels(dc, g, float(radius))
    assert (label == 0).all() and (size == n).all()
    _, few = _check_labels(dc, g, 0.025)  # the same rows, many cells, clusters of a few rows
    assert 3 < few.max() < 20
    dc.close()


def _sparse_cells(rng):
    r = f32(RADIUS)
    cells = np.stack(np.meshgrid(np.arange(-3, 3), np.arange(-3, 3), np.arange(-3, 3), indexing="ij"), axis=-1).reshape(-1, 3)[:200] * 2
    first = (cells + rng.uniform(0.1, 0.4, (200, 3))) * float(r)
    second = first[::2] + rng.uniform(0.3, 0.5, (100, 3)) * float(r)
    xyz = np.concatenate([first, second]).astype(f32)
    return xyz[rng.permutation(xyz.shape[0])]


def test_two_hundred_cells_of_one_or_two_rows(opt):
    xyz = _sparse_cells(np.random.default_rng(6))
    dc, kept = ng._still_cloud(opt, xyz, VOXEL)
    assert kept.shape[0] == 300
    g, _ = dc.retained()
    label, size = _check_labels(dc, g, RADIUS)
    assert sorted(np.bincount(size)[1:].tolist()) == [100, 200]  # 100 lone rows, 100 pairs
    flags, stats, _, _ = _check_classify(dc, g, RADIUS, 2)
    assert stats == dict(rows=300, clusters=200, largest=2, kept_rows=200, kept_clusters=100, small_rows=100, large_rows=0) and np.array_equal(flags, (size == 2).astype(np.uint8))
    assert dc.remove_clusters() == 200
    g2, _ = dc.retained()
    assert np.array_equal(_bits(g2), _bits(g[size == 2]))
    dc.close()


def test_sorted_order_that_jumps_between_distant_surfaces(opt):
    """120 small blobs and 150 lone rows scattered over 10 m: 64 consecutive sorted rows lie in blobs far apart, the box of a wave exceeds
    kGridBoxCells and the wave goes through its distinct cells one by one."""
    import test_gpu_dense_outliers as og

    rng = np.random.default_rng(12)
    centres = rng.uniform(-5, 5, (120, 3))
    xyz = np.concatenate([c + ng._one_per_voxel(rng, 30, VOXEL, 4) for c in centres] + [rng.uniform(-5, 5, (150, 3))]).astype(f32)
    xyz = xyz[rng.permutation(xyz.shape[0])]
    dc, kept = ng._still_cloud(opt, xyz, VOXEL)
    g, _ = dc.retained()
    boxes = og._wave_box_cells(g, RADIUS)
    assert g.shape[0] > 3000 and (boxes > 512).mean() > 0.9
    label, size = _check_labels(dc, g, RADIUS)
    _, stats, _, _ = _check_classify(dc, g, RADIUS, 10)
    dc.close()
    assert 100 <= stats["kept_clusters"] <= 120 and stats["small_rows"] > 50


# ---- 8. classification --------------------------------------------------------------------------------------------------------------------------------
def test_clusters_of_exactly_min_and_max_size_are_kept(opt):
    """Blobs of 4, 5, 9, 10, 1 and 7 rows, two metres apart, every blob inside a cube of three voxels whose diagonal is below the radius."""
    rng = np.random.default_rng(23)
    sizes = [4, 5, 9, 10, 1, 7]
    radius = 0.3
    xyz = np.concatenate([ng._one_per_voxel(rng, m, VOXEL, 3, corner=(2.0 * k, 1.0, -1.0)) for k, m in enumerate(sizes)])
    group = np.repeat(np.arange(len(sizes)), sizes)
    order = rng.permutation(xyz.shape[0])
    dc, kept = ng._still_cloud(opt, xyz[order], VOXEL)
    assert kept.shape[0] == sum(sizes)
    g, _ = dc.retained()
    flags, stats, label, size = _check_classify(dc, g, radius, 5, 9)
    assert np.array_equal(size, np.array(sizes)[group[order]])
    assert np.array_equal(flags, np.isin(size, (5, 7, 9)).astype(np.uint8))
    assert stats == dict(rows=36, clusters=6, largest=10, kept_rows=21, kept_clusters=3, small_rows=5, large_rows=10)
    _, stats, _, _ = _check_classify(dc, g, radius, 5)  # no upper bound
    assert stats["kept_rows"] == 31 and stats["large_rows"] == 0
    _, stats, _, _ = _check_classify(dc, g, radius, 10, 10)
    assert stats["kept_rows"] == 10 and stats["kept_clusters"] == 1 and stats["small_rows"] == 26
    _, stats, _, _ = _check_classify(dc, g, radius, 1, 1)
    assert stats["kept_rows"] == 1 and stats["large_rows"] == 35
    dc.close()


@pytest.mark.parametrize("radius,min_size,max_size", [(RADIUS, 50, 0), (RADIUS, 5, 100), (0.06, 2, 3), (0.06, 1, 0)])
def test_classify_equals_the_model_in_flags_and_all_seven_fields(mixed, radius, min_size, max_size):
    _, stats, _, _ = _check_classify(mixed["dc"], mixed["g"], radius, min_size, max_size)
    assert stats["kept_rows"] > 0 and (min_size == 1 or stats["small_rows"] > 0)


# ---- 9. removal ---------------------------------------------------------------------------------------------------------------------------------------
def test_remove_clusters_compacts_points_and_origins_and_later_calls_follow(opt, tmp_path):
    import test_gpu_dense_outliers as og

    no_mask, no_labels = "no classification of the store as it stands", "no labels of the store as it stands"
    radius, min_size = 0.25, 20
    dc, _ = ng._creator(opt, lidar_to_imu=base.L2I, voxel_size=0.1, min_range=0.5)
    scans = og._wall_scans(np.random.default_rng(9))
    for xyz, t in scans:
        dc.add_scan(xyz, t)
    _refused(dc.remove_clusters, no_mask)  # nothing classified yet
    _refused(lambda: dc.save_pcd_labels(tmp_path / "no.pcd"), no_labels)
    g, o = dc.retained()
    flags, stats, label, size = _check_classify(dc, g, radius, min_size)
    assert g.shape[0] > 1000 and 20 < stats["small_rows"] < 0.5 * g.shape[0] and stats["kept_clusters"] >= 1
    assert dc.save_pcd_labels(tmp_path / "a.pcd")[0] == g.shape[0]
    # a scan added after classify: labels and mask are stale
    far = np.zeros((50, 4), f32)
    far[:, 0], far[:, 1:3] = 6.0, np.random.default_rng(1).uniform(3.0, 4.0, (50, 2))
    extra, _ = dc.add_scan(far, np.linspace(base.S[4], base.S[5], 50))
    assert extra.shape[0] > 10
    _refused(dc.remove_clusters, no_mask)
    _refused(lambda: dc.save_pcd_labels(tmp_path / "no.pcd"), no_labels)
    assert not (tmp_path / "no.pcd").exists()
    g, o = dc.retained()
    flags, stats, label, size = _check_classify(dc, g, radius, min_size)
    # the outlier stage's removal in between (k = 1 and a threshold far out: only the rows with nothing within 0.4 m leave, the strays that
    # stand in twos and threes stay): this stage's classification was of the store before
    o_flags, o_stats, _ = om.classify(g, 0.4, 1, 1e6)
    assert dc.classify_outliers(0.4, 1, 1e6) == o_stats and dc.remove_outliers() == o_stats["inliers"] < g.shape[0]
    _refused(dc.remove_clusters, no_mask)
    _refused(lambda: dc.save_pcd_labels(tmp_path / "no.pcd"), no_labels)
    g, o = g[o_flags.astype(bool)], o[o_flags.astype(bool)]
    flags, stats, label, size = _check_classify(dc, g, radius, min_size)
    assert dc.classify_outliers(0.4, 8, 1.0)["rows"] == g.shape[0]
    slots, occupied = dc.table_info()
    before = dc.stats()
    # the removal
    keep = flags.astype(bool)
    assert dc.remove_clusters() == stats["kept_rows"] == int(keep.sum()) == dc.retained_count() < g.shape[0]
    g2, o2 = dc.retained()
    assert np.array_equal(_bits(g2), _bits(g[keep])) and np.array_equal(_bits(o2), _bits(o[keep]))
    assert len(np.unique(o2[:, :3], axis=0)) > 500  # an origin per stamp: the origins moved with their points
    assert dc.table_info() == (slots, occupied) and dc.stats() == before  # C6: the voxel set and the scan statistics are untouched
    _refused(dc.remove_clusters, no_mask)  # the classification was of the store before
    _refused(dc.remove_outliers, no_mask)
    _refused(lambda: dc.save_pcd_labels(tmp_path / "no.pcd"), no_labels)
    # the cleaned store labels like any other, and every cluster left has min_size rows
    label2, size2 = _check_labels(dc, g2, radius)
    assert size2.min() >= min_size
    dc.close()


def test_the_intensity_travels_with_the_kept_rows(opt, tmp_path):
    from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator

    rng = np.random.default_rng(27)
    xyz = ng._one_per_voxel(rng, 900, VOXEL, 24, corner=(-0.6, -0.6, 0.2))
    rows = np.concatenate([xyz, np.arange(900, dtype=f32)[:, None] + f32(0.5)], axis=1).astype(f32)
    s, p, q = base._still_trajectory()
    dc = DenseCloudCreator(s, p, q, DenseCloudConfig(voxelSize=VOXEL), optimizer=opt, retain=True, intensity=True)
    kept, _ = dc.add_scan(rows, ng._stamps(900))
    g, o = dc.retained()
    assert kept.shape[0] == 900 and np.array_equal(_bits(g), _bits(rows))
    flags, stats, label, size = _check_classify(dc, g, 0.08, 4)
    assert 0 < stats["kept_rows"] < 900
    # the 20-byte rows of the whole store, then the removal
    points, nbytes = dc.save_pcd_labels(tmp_path / "i.pcd")
    raw = open(tmp_path / "i.pcd", "rb").read()
    assert raw == cm.file_bytes(g, label, intensity=True) and (points, nbytes) == (900, len(raw))
    assert dc.remove_clusters() == stats["kept_rows"]
    g2, o2 = dc.retained()
    keep = flags.astype(bool)
    assert np.array_equal(_bits(g2), _bits(g[keep])) and np.array_equal(g2[:, 3], rows[keep, 3]) and (o2[:, 3] == 1).all()
    dc.close()


def test_carve_then_clusters_then_outliers_then_normals_equal_the_models_chained(opt):
    import test_gpu_dense_carve as tg
    from dmsa_lidar_slam_amd.dense_cloud import DenseCarveConfig, normal_from_moments

    rng = np.random.default_rng(11)
    scans = []
    for k in range(3):
        wall = np.c_[6.05 + 0.1 * k + rng.normal(0, 0.01, 700), rng.uniform(-1.5, 1.5, 700), rng.uniform(-1.0, 1.5, 700)]
        scans.append(wall if k else np.concatenate([np.c_[3.0 + rng.normal(0, 0.08, 300), rng.uniform(-0.3, 0.3, 300), rng.uniform(-0.2, 0.9, 300)], wall]))
    origins = np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.25], [0.0, -0.5, 0.125]])
    dc, g, o = tg._store(opt, scans, origins=origins)
    # carve
    want, t_stats = tm.count_passes(g, o, tm.Config())
    assert dc.count_passes(DenseCarveConfig()) == t_stats and 0 < t_stats["transient"]
    assert dc.remove_transients() == t_stats["kept"]
    keep = want < 2
    g, o = g[keep], o[keep]
    # clusters: what the carving left of the blob is smaller than the wall
    flags, k_stats, label, size = _check_classify(dc, g, 0.3, 40)
    left_of_blob = g[:, 0] < 4.0
    assert 0 < left_of_blob.sum() and k_stats["small_rows"] >= left_of_blob.sum() and not flags[left_of_blob].any() and k_stats["kept_rows"] > 1000
    assert dc.remove_clusters() == k_stats["kept_rows"]
    g, o = g[flags.astype(bool)], o[flags.astype(bool)]
    # outliers
    o_flags, o_stats, _ = om.classify(g, 0.4, 8, 1.0)
    got, got_flags = dc.classify_outliers(0.4, 8, 1.0, download=True)
    assert got == o_stats and np.array_equal(got_flags, o_flags)
    assert dc.remove_outliers() == o_stats["inliers"]
    g, o = g[o_flags.astype(bool)], o[o_flags.astype(bool)]
    # normals
    g3, o3 = dc.retained()
    assert np.array_equal(_bits(g3), _bits(g)) and np.array_equal(_bits(o3), _bits(o))
    normals, without = dc.compute_normals(0.4, 5)
    ref_n = normal_from_moments(nm.moments(g, 0.4), nm.view_vectors(g, o), 5)
    assert np.array_equal(_bits(normals), _bits(ref_n)) and without == int(np.isnan(ref_n[:, 0]).sum())
    dc.close()


# ---- 10. determinism ------------------------------------------------------------------------------------------------------------------------------------
def test_two_fresh_objects_give_the_same_bytes_and_a_shuffled_store_the_same_partition(opt, tmp_path):
    rng = np.random.default_rng(41)
    xyz = ng._one_per_voxel(rng, 3000, VOXEL, 32)
    radius = 0.07
    out = []
    for reserve in (0, 30000):
        dc, _ = ng._still_cloud(opt, xyz, VOXEL, reserve=reserve)
        label, size = dc.cluster_labels(radius)
        stats, flags = dc.classify_clusters(radius, 3, 8, download=True)
        path = tmp_path / f"labels{reserve}.pcd"
        dc.save_pcd_labels(path)
        left = dc.remove_clusters()
        assert left == stats["kept_rows"] < 3000 and stats["small_rows"] > 0 and stats["large_rows"] > 0
        out.append((label.tobytes(), size.tobytes(), stats, flags.tobytes(), open(path, "rb").read(), dc.retained()[0].tobytes()))
        dc.close()
    assert out[0] == out[1]
    label = np.frombuffer(out[0][0], np.int32)
    assert len(np.unique(label)) > 300
    # the same rows in another store order: the partition is the same, named by other rows
    perm = np.random.default_rng(42).permutation(3000)
    dc, kept = ng._still_cloud(opt, xyz[perm], VOXEL)
    assert np.array_equal(_bits(kept[:, :3]), _bits(xyz[perm]))
    label2, size2 = dc.cluster_labels(radius)
    dc.close()
    canon = np.full(3000, 3000, np.int64)
    np.minimum.at(canon, label2, perm)  # per cluster of the shuffled store, the smallest original row in it
    back = np.empty(3000, np.int64)
    back[perm] = canon[label2]
    assert np.array_equal(back, label)
    size_back = np.empty(3000, np.int32)
    size_back[perm] = size2
    assert np.array_equal(size_back, np.frombuffer(out[0][1], np.int32))


# ---- 11. the file -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_file_is_its_header_and_16_byte_rows(mixed, tmp_path):
    from dmsa_lidar_slam_amd.api import DmsaError
    from dmsa_lidar_slam_amd.dense_cloud import pcdHeaderXyzLabelBinary

    dc, g = mixed["dc"], mixed["g"]
    label, size = _check_labels(dc, g, RADIUS)
    path = tmp_path / "Labels.pcd"
    points, nbytes = dc.save_pcd_labels(path)
    raw = open(path, "rb").read()
    head, rows, file_size = cm.read_file(path)
    assert head == pcdHeaderXyzLabelBinary(g.shape[0]) == cm.header(g.shape[0])
    assert points == g.shape[0] == rows.shape[0] and nbytes == file_size == len(head) + 16 * points
    assert raw == cm.file_bytes(g, label)
    # the path of a directory: refused, nothing left behind
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(DmsaError) as e:
        dc.save_pcd_labels(tmp_path)
    assert e.value.status == -1 and "cannot open" in e.value.args[0] and sorted(os.listdir(tmp_path)) == before
    with pytest.raises(DmsaError):
        dc.save_pcd_labels(tmp_path / "no" / "such" / "dir.pcd")
    assert sorted(os.listdir(tmp_path)) == before
    # the x y z file of the same object shares the pinned buffers: one after the other, both right
    dc.save_pcd_retained(tmp_path / "xyz.pcd")
    assert dc.save_pcd_labels(path) == (points, nbytes) and open(path, "rb").read() == raw


FILE_CHUNK = 1 << 20  # kFileChunkRows of csrc/dense_store.cpp


def test_the_file_of_a_store_of_more_than_one_chunk(opt, tmp_path):
    """2^20 + 1 rows: the second chunk of the copy-back holds one row.  At a radius of one voxel a row has about two adjacent rows."""
    n = FILE_CHUNK + 1
    dc, kept = ng._still_cloud(opt, ng._one_per_voxel(np.random.default_rng(n), n, VOXEL, 128), VOXEL)
    g, _ = dc.retained()
    assert kept.shape[0] == n == g.shape[0]
    label, size = dc.cluster_labels(VOXEL)
    want_label, want_size = cm.labels(g, VOXEL)
    assert np.array_equal(label, want_label) and np.array_equal(size, want_size)
    path = tmp_path / "Labels.pcd"
    points, nbytes = dc.save_pcd_labels(path)
    dc.close()
    head, rows, file_size = cm.read_file(path)
    assert head == cm.header(n) and points == n == rows.shape[0] and nbytes == file_size == len(head) + 16 * n
    xyz = np.stack([rows["x"], rows["y"], rows["z"]], axis=1)
    assert np.array_equal(_bits(xyz), _bits(g[:, :3])) and np.array_equal(rows["label"], label.astype(np.uint32))
    assert len(np.unique(label)) > 1000 and size.max() > 100


# ---- 12. refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_every_breach_of_c1_is_refused_with_its_reason(opt, tmp_path):
    from dmsa_lidar_slam_amd.api import DmsaError

    rng = np.random.default_rng(44)
    xyz = ng._one_per_voxel(rng, 100, VOXEL, 8)
    off, _ = ng._creator(opt, retain=False, still=True, voxel_size=VOXEL)
    off.add_scan(xyz, ng._stamps(100))
    for call in (off.classify_clusters, off.cluster_labels, off.remove_clusters, lambda: off.save_pcd_labels(tmp_path / "x.pcd")):
        with pytest.raises(DmsaError) as e:
            call()
        assert e.value.status == -1
    _refused(off.classify_clusters, "retention is off")
    _refused(lambda: off.save_pcd_labels(tmp_path / "x.pcd"), "retention is off")
    off.close()
    empty, _ = ng._creator(opt, still=True, voxel_size=VOXEL)
    _refused(lambda: empty.classify_clusters(RADIUS), "no retained point")
    _refused(lambda: empty.cluster_labels(RADIUS), "no retained point")
    _refused(lambda: empty.save_pcd_labels(tmp_path / "empty.pcd"), "no retained point")
    _refused(empty.remove_clusters, "no classification")
    assert not (tmp_path / "empty.pcd").exists() and not (tmp_path / "x.pcd").exists()
    empty.close()
    no_voxel, _ = ng._creator(opt, still=True, voxel_size=0.0)
    no_voxel.add_scan(xyz, ng._stamps(100))
    _refused(lambda: no_voxel.classify_clusters(RADIUS), "voxel_size must be > 0")
    no_voxel.close()
    dc, _ = ng._still_cloud(opt, xyz, VOXEL)
    for call in (dc.classify_clusters, dc.cluster_labels):
        _refused(lambda: call(np.inf), "radius is not finite")
        _refused(lambda: call(np.nan), "radius is not finite")
        _refused(lambda: call(np.nextafter(f32(VOXEL), f32(0))), "[voxel_size, 64 * voxel_size]")
        _refused(lambda: call(np.nextafter(f32(64.0) * f32(VOXEL), f32(10))), "[voxel_size, 64 * voxel_size]")
        _refused(lambda: call(-1.0), "[voxel_size, 64 * voxel_size]")
    for m in (0, -1, (1 << 26) + 1):
        _refused(lambda: dc.classify_clusters(RADIUS, m), "min_size must lie in [1, 2^26]")
    for m in (4, -1, (1 << 26) + 1):
        _refused(lambda: dc.classify_clusters(RADIUS, 5, m), "max_size must be 0 or lie in [min_size, 2^26]")
    # a refused call leaves neither a classification nor labels; the bounds themselves are legal
    _refused(dc.remove_clusters, "no classification")
    _refused(lambda: dc.save_pcd_labels(tmp_path / "y.pcd"), "no labels of the store as it stands")
    assert not (tmp_path / "y.pcd").exists()
    assert dc.classify_clusters(VOXEL, 1 << 26, 1 << 26)["kept_rows"] == 0 and dc.classify_clusters(64.0 * VOXEL, 1, 0)["kept_rows"] == 100
    assert dc.classify_clusters(RADIUS, 5, 5)["rows"] == 100
    dc.close()


# ---- 13. the programs -------------------------------------------------------------------------------------------------------------------------------------
def test_the_demo_removes_small_clusters_and_writes_the_labels(tmp_path):
    out = tmp_path / "Clusters.pcd"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dense_cloud_demo.py"), "--scans", "6", "--clusters", "0.3", "20", "--clusters-out", str(out),
                        "--out", str(tmp_path / "Dense.pcd")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    kept = int(re.search(r"\bkept (\d+)", p.stdout).group(1))
    rows, kept_rows = int(re.search(r"\brows (\d+)", p.stdout).group(1)), int(re.search(r"\bkept_rows (\d+)", p.stdout).group(1))
    head, body, _ = cm.read_file(out)
    assert head == cm.header(kept_rows) and body.shape[0] == kept_rows and rows == kept > 2000 and 0 < kept_rows <= kept
    xyz = np.stack([body["x"], body["y"], body["z"]], axis=1)
    label, size = cm.labels(xyz, 0.3)
    assert np.array_equal(body["label"], label.astype(np.uint32)) and size.min() >= 20


def test_the_cpp_example_removes_small_clusters_like_the_demo(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import dense_cloud_demo

    r = dense_cloud_demo.run(scans=6, workdir=str(tmp_path), clusters=(0.3, 20))
    exe = os.path.join(ROOT, "examples", "dense_cloud_from_raw")
    out, labels = tmp_path / "cpp_kept.pcd", tmp_path / "cpp_labels.pcd"
    p = subprocess.run([exe, r["dump"], r["poses_file"], "ouster", str(out), "--voxel", "0.1", "--min-range", "0.5", "--cluster-min", "20", "--cluster-radius", "0.3",
                        "--cluster-labels", str(labels)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
    assert int(re.search(r"\bkept_rows (\d+)", p.stdout).group(1)) == r["clusters"]["kept_rows"] == r["clusters_points"] > 1000
    assert open(labels, "rb").read() == open(r["clusters_pcd"], "rb").read()
    _, body, _ = cm.read_file(labels)
    raw = open(out, "rb").read()
    xyz = np.frombuffer(raw[raw.index(b"DATA binary\n") + 12 :], "<f4").reshape(-1, 3)
    assert np.array_equal(_bits(xyz), _bits(np.stack([body["x"], body["y"], body["z"]], axis=1)))
    # a size out of range is refused with C1's reason
    p = subprocess.run([exe, r["dump"], r["poses_file"], "ouster", str(tmp_path / "no.pcd"), "--voxel", "0.1", "--cluster-min", "0"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 1 and "min_size must lie in [1, 2^26]" in p.stderr and not (tmp_path / "no.pcd").exists()
