"""GPU tests of include/dmsa_dense_carve.h against the model of T2-T7 (tests/dense_carve_model.py).

The walk: k_carve_walk_rows against the model in the number of cells and in the order-dependent hash of the cell sequence, bit for bit.  The
counts: k_carve_passes against the model in `passes` and in all eight statistics (integers throughout: T5 is the same float operations on both
sides).  The removal: store and origins afterwards are the model's non-transient rows bit for bit and in order.

Stores are built by add_scan on a trajectory that stands still at a different place for every scan (identity rotations, segments 0, 2, 4 and
6 of eight poses): g = p + t with one rounding, exact where the numbers are dyadic, and every scan has an origin of its own.  The model is fed
the store's own g and o, read back.

The kernel takes a ray per lane in the grid's sorted order, so the shapes are totals around the wave and the block (1 / 63 / 64 / 65 / 257 /
4 097), rays of one cell and of the largest extent in one wave, one cell of 1 500 rows, many cells of one or two rows, and coordinates at the
edge of the 21-bit cell range with origins beyond it.

Not tested here: the T1 bound of 2^26 retained rows (a store of 2 GiB)."""
import numpy as np
import pytest

import dense_carve_model as cm
import dense_normals_model as nm
import dense_outliers_model as om
import test_gpu_dense_cloud as base
import test_gpu_dense_normals as ng
import test_gpu_dense_outliers as og

pytestmark = pytest.mark.gpu

f32 = np.float32
VOXEL = 0.1
ORIGINS = np.array([[0.0, 0.0, 0.0], [0.5, 2.0, 0.25], [-1.0, -1.5, 0.5], [0.25, 0.5, 1.0]])
LIVELY = dict(rho=0.1, tan_half_angle=0.2, end_margin=0.1, start_margin=0.2)  # a wider cone than the default: more rows are seen through
_bits = ng._bits


@pytest.fixture(scope="module")
def opt():
    from dmsa_lidar_slam_amd.api import DmsaOptimizer

    o = DmsaOptimizer(device=0)
    yield o
    o.close()


def _cfg(**kw):
    from dmsa_lidar_slam_amd.dense_cloud import DenseCarveConfig

    return DenseCarveConfig(**kw), cm.Config(**kw)


def _store(opt, scans, voxel=VOXEL, origins=ORIGINS):
    """scans: a list of world points (m,3), one per origin; scan k is measured from origins[k] (its sensor-frame points are g - origin).  Returns
    (the object, g, o) with g and o read back from the store."""
    from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator

    pos = np.repeat(np.asarray(origins, np.float64)[:4], 2, axis=0)
    if pos.shape[0] < 8:
        pos = np.concatenate([pos, np.repeat(pos[-1:], 8 - pos.shape[0], axis=0)])
    quat = np.tile([0.0, 0.0, 0.0, 1.0], (8, 1))
    dc = DenseCloudCreator(base.S, pos, quat, DenseCloudConfig(voxelSize=voxel), optimizer=opt, retain=True)
    for k, world in enumerate(scans):
        world = np.asarray(world, np.float64).reshape(-1, 3)
        if world.shape[0] == 0:
            continue
        local = (world - np.asarray(origins, np.float64)[k]).astype(f32)
        a, b = base.S[2 * k], base.S[2 * k + 1]
        dc.add_scan(local, np.linspace(a + 0.25 * (b - a), a + 0.75 * (b - a), world.shape[0]))
    g, o = dc.retained()
    return dc, g, o


def _split(rng, xyz, parts):
    cut = np.sort(rng.choice(np.arange(1, xyz.shape[0]), parts - 1, replace=False)) if xyz.shape[0] >= parts else []
    return np.split(xyz, cut) if len(cut) else [xyz]


def _check_walk(dc, g, o, py, model, windows=((0, None),)):
    want_cells, want_hash = cm.walk_rows(g, o, model)
    for first, count in windows:
        cells, hashes = dc.carve_walk_rows(py, first, count)
        stop = g.shape[0] if count is None else first + count
        assert cells.dtype == np.int32 and hashes.dtype == np.uint64
        assert np.array_equal(cells, want_cells[first:stop]), (first, count, np.flatnonzero(cells != want_cells[first:stop])[:10])
        assert np.array_equal(hashes, want_hash[first:stop]), (first, count, np.flatnonzero(hashes != want_hash[first:stop])[:10])
    return want_cells


def _check_passes(dc, g, o, py, model):
    want, want_stats = cm.count_passes(g, o, model)
    stats, passes = dc.count_passes(py, download=True)
    assert list(stats) == list(cm.STAT_NAMES) and stats == want_stats, [(n, stats[n], want_stats[n]) for n in stats if stats[n] != want_stats[n]]
    assert passes.dtype == np.uint32 and np.array_equal(passes, want), np.flatnonzero(passes != want)[:10]
    assert dc.count_passes(py) == want_stats  # without the counts: the dict alone
    assert stats["rows"] == g.shape[0] == stats["rays_walked"] + stats["rays_skipped"] == stats["transient"] + stats["kept"] and stats["seen_through"] == int(want.sum())
    return want, want_stats


# ---- 1. every total -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [1, 63, 64, 65, 257, 4097])
def test_walk_and_passes_at_every_total(opt, total):
    """A cube of voxels two metres in front of four origins: the rays of one scan run through the rows of the others."""
    rng = np.random.default_rng(total)
    side = 8 if total < 300 else 20
    xyz = ng._one_per_voxel(rng, total, VOXEL, side, corner=(2.0, -0.4, -0.3))
    dc, g, o = _store(opt, _split(rng, xyz, 4))
    assert g.shape[0] == total == dc.retained_count() and (total < 4 or len(np.unique(o[:, :3], axis=0)) == 4)
    n = g.shape[0]
    windows = ((0, None), (0, 1), (n - 1, 1), (n // 3, min(70, n - n // 3)), (max(n - 65, 0), min(65, n)), (min(63, n - 1), min(130, n - min(63, n - 1))), (0, 0))
    py, model = _cfg(cell_size=0.2, **LIVELY)
    _check_walk(dc, g, o, py, model, windows)
    want, stats = _check_passes(dc, g, o, py, model)
    assert total < 257 or (stats["seen_through"] > 0 and 0 < stats["transient"] < total)
    if total < 4097:  # ... and the defaults
        py, model = _cfg()
        _check_walk(dc, g, o, py, model, windows[:2])
        _check_passes(dc, g, o, py, model)
    dc.close()


# ---- 2. the walk: skipped rays, one cell and the largest extent in one wave ------------------------------------------------------------------------
def test_walks_of_one_cell_of_the_largest_extent_and_skipped_rays_in_one_wave(opt):
    """Voxels of 1 cm, cells of 64 voxels.  Every 64 consecutive rows (a wave of the stage call) hold 10 rays that stay in the origin's cell, 50
    of a few cells, two whose ends are exactly 2^11 cells apart along x (2 049 traversed cells and more: they climb in y and z as well) and
    two of 2^11 + 1, which are skipped; with a max_length of 20 m the long ones are skipped for their length instead."""
    rng = np.random.default_rng(2)
    voxel = 0.01
    c = float(f32(0.01) * f32(64.0))
    scan = []
    for k in range(5):
        near = rng.uniform(0.02, 0.62, (10, 3))  # the origin's cell (0, 0, 0)
        mid = np.c_[rng.uniform(1.0, 6.0, 50), rng.uniform(-3, 3, 50), rng.uniform(-1, 2, 50)]
        far = np.array([[2048.5 * c, 3.0 + k, 1.0 + k], [2049.5 * c, -3.0 - k, 1.5 + k], [-2047.5 * c, 2.0 + k, 0.55], [-2048.5 * c, 2.0 + k, 0.7]])
        block = np.concatenate([near, mid, far])
        scan.append(block[rng.permutation(block.shape[0])])
    xyz = np.concatenate(scan)
    dc, g, o = _store(opt, [xyz], voxel=voxel, origins=ORIGINS[:1])
    assert g.shape[0] == 320 and (o[:, :3] == 0).all()
    py, model = _cfg(cell_size=c, max_length=5000.0)
    cells = _check_walk(dc, g, o, py, model, ((0, None), (17, 64), (64, 64), (5, 200)))
    for a in range(0, g.shape[0] - 63, 64):
        wave = cells[a : a + 64]
        assert (wave == -1).sum() == 2 and (wave == 1).sum() == 10 and (wave > 2048).sum() == 2 and ((wave > 3) & (wave < 60)).any(), a
    assert cells.max() <= 3 * 2048 + 1 and (cells == -1).sum() == 10 and (cells > 2048).sum() == 10
    py, model = _cfg(cell_size=c, max_length=20.0)
    cells = _check_walk(dc, g, o, py, model)
    assert (cells == -1).sum() == 20 and cells.max() < 60
    # the counts with both kinds of rays in the waves (the long rays run through two thousand empty cells)
    py, model = _cfg(cell_size=c, max_length=5000.0, **LIVELY)
    _, stats = _check_passes(dc, g, o, py, model)
    assert stats["rays_skipped"] == 10 and stats["cells_traversed"] > 10 * 2049
    dc.close()


def test_a_ray_exactly_as_long_as_max_length_is_walked(opt):
    """T2's L is the CORRECTLY ROUNDED square root: with max_length set to the model's L of ray i, ray i is walked (L > max_length is false)
    and every longer ray is skipped.  One call per ray, 2 048 lengths: a square root that is one ulp high for any of them skips its own ray."""
    from dmsa_lidar_slam_amd.dense_cloud import DenseCarveConfig

    rng = np.random.default_rng(21)
    xyz = ng._one_per_voxel(rng, 2048, VOXEL, 30, corner=(1.5, -1.2, -0.8))
    dc, g, o = _store(opt, _split(rng, xyz, 4))
    d = g[:, :3] - o[:, :3]
    length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    assert length.dtype == f32 and g.shape[0] == 2048 and all(length[i] == cm.ray(o[i, :3], g[i, :3])[2] for i in range(0, 2048, 97))
    bad = []
    for i in range(g.shape[0]):
        cells, _ = dc.carve_walk_rows(DenseCarveConfig(max_length=float(length[i])))
        if not np.array_equal(cells == -1, length > length[i]):
            bad.append(i)
    dc.close()
    assert not bad, (len(bad), bad[:10])


# ---- 3. shapes of the grid -------------------------------------------------------------------------------------------------------------------------
def test_one_cell_of_1500_rows_crossed_by_64_rays(opt):
    """Voxels of 1 cm and cells of 64 voxels: 1 500 rows in ONE cell, measured from its corner -- each of their rays stays in the cell, is offered
    the 1 499 others and is not offered itself (T5: j != r shows in pair_tests) -- and 64 rays of a second scan that enter the cell from the
    next one and end in the one behind it."""
    rng = np.random.default_rng(5)
    voxel = 0.01
    cell = float(f32(0.01) * f32(64.0))
    inside = ng._one_per_voxel(rng, 1500, voxel, 60, corner=(0.02, 0.02, 0.02))
    behind = np.c_[rng.uniform(0.7, 0.9, 64), rng.uniform(0.1, 0.5, 64), rng.uniform(0.1, 0.5, 64)]
    origins = np.array([[0.0, 0.0, 0.0], [-0.75, 0.25, 0.375]])
    dc, g, o = _store(opt, [inside, behind], voxel=voxel, origins=origins)
    assert g.shape[0] == 1564 and len({cm.cell_of(p, cell) for p in g[:1500]}) == 1 and all(cm.cell_of(p, cell)[0] == 1 for p in g[1500:])
    py, model = _cfg(cell_size=cell, rho=0.03, tan_half_angle=0.2, end_margin=0.05, start_margin=0.1, max_length=5.0)
    _check_walk(dc, g, o, py, model)
    want, stats = _check_passes(dc, g, o, py, model)
    assert stats["pair_tests"] >= 1500 * 1499 + 64 * 1500 and want[:1500].max() >= 3 and stats["seen_through"] > 1000
    dc.close()


def test_two_hundred_cells_of_one_or_two_rows(opt):
    xyz = og._sparse_cells(np.random.default_rng(6)) + np.array([3.0, 0.0, 0.0], f32)
    rng = np.random.default_rng(7)
    dc, g, o = _store(opt, _split(rng, xyz, 3))
    assert g.shape[0] == 300
    py, model = _cfg(cell_size=og.RADIUS, rho=0.2, tan_half_angle=0.5, end_margin=0.1, start_margin=0.2)
    assert 190 <= len({cm.cell_of(p, og.RADIUS) for p in g}) <= 200
    _check_walk(dc, g, o, py, model)
    want, stats = _check_passes(dc, g, o, py, model)
    assert stats["seen_through"] > 0 and stats["pair_tests"] > 300
    dc.close()


def test_coordinates_at_the_edge_of_the_cell_range_and_origins_beyond_it(opt):
    """Cells of one voxel: rows in cells up to +-(2^20 - 1), one scan measured from inside the range and two from beyond it in x and y, whose rays
    start in cells that hold no rows by definition and are not looked up."""
    rng = np.random.default_rng(9)
    edge = (2**20 - 2) * 0.1
    first = np.array([2**20 - 2 - 59, -(2**20), 2**20 - 100])  # the voxels first .. first + 59: up to 2^20 - 2 in x, down to -2^20 in y
    cellsv = rng.choice(60**3, 400, replace=False)
    idx = np.stack([cellsv // 3600, (cellsv // 60) % 60, cellsv % 60], axis=1)
    idx = np.concatenate([idx, [[59, 0, 30], [59, 30, 0], [0, 0, 59]]])  # (the corners for certain; a double is harmless: one point per voxel)
    xyz = (first + idx + 0.5) * 0.1  # voxel centres: float32 has steps of 2^-7 here
    origins = np.array([[edge - 8.0, -edge + 8.0, edge - 4.0], [edge + 2.0, -edge - 3.0, edge - 2.0], [edge + 0.75, -edge + 7.0, edge - 5.0]])
    dc, g, o = _store(opt, _split(rng, xyz, 3), origins=origins)
    cells = np.array([cm.cell_of(p, VOXEL) for p in g])
    assert g.shape[0] >= 400 and cells[:, 0].max() == 2**20 - 2 and cells[:, 1].min() == -(2**20) and len(np.unique(o[:, :3], axis=0)) == 3
    assert max(cm.cell_of(p, VOXEL)[0] for p in o) >= 2**20 and min(cm.cell_of(p, VOXEL)[1] for p in o) < -(2**20)
    py, model = _cfg(cell_size=VOXEL, rho=0.1, tan_half_angle=0.3, end_margin=0.1, start_margin=0.2)
    _check_walk(dc, g, o, py, model)
    want, stats = _check_passes(dc, g, o, py, model)
    assert stats["rays_skipped"] == 0 and stats["seen_through"] > 0
    dc.close()


# ---- 4. the pair test at its bounds, min_passes ----------------------------------------------------------------------------------------------------
def test_candidates_exactly_at_end_margin_and_at_rho(opt):
    """Dyadic numbers throughout (voxel 0.25, cells of 1): the ray (0, 0, 0) -> (8, 0, 0) and candidates measured from (0, 0.5, 0).  Row `at` has
    rem == end_margin, perp2 == rho * rho and perp2 == w * w at once and is seen through; a row whose rem is one ulp less is not, nor is `at` itself
    under bounds one ulp tighter."""
    up = lambda v: float(np.nextafter(f32(v), f32(np.inf)))  # noqa: E731
    target = np.array([[8.0, 0.0, 0.0]])
    cands = np.array([[7.5, 0.25, 0.0],      # at: every comparison at equality
                      [up(7.5), 0.125, 0.0],  # rem one ulp below end_margin
                      [6.5, 0.25 + 2.0**-12, 0.0],  # perp2 above rho * rho (by more than u2 - rem * rem rounds away)
                      [6.5, 0.125, 0.0],      # well inside
                      [7.0, 0.25, 0.0],       # rem = 1, perp2 == rho * rho, inside the cone
                      [7.5, -0.25, 0.0]])     # as `at`, but in the cell row below the ray's: not a candidate (T4 restricts them to traversed cells)
    dc, g, o = _store(opt, [target, cands], voxel=0.25, origins=np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.0]]))
    assert np.array_equal(g[:, :3], np.concatenate([target, cands]).astype(f32)) and np.array_equal(o[1:, :3], np.tile(f32([0, 0.5, 0]), (6, 1)))
    kw = dict(cell_size=1.0, rho=0.25, tan_half_angle=0.5, end_margin=0.5, start_margin=0.5, min_passes=1)
    py, model = _cfg(**kw)
    t = cm.pair_terms(o[0, :3], g[0, :3], g[1, :3])
    assert (t["rem"], t["perp2"], t["s"]) == (0.5, 0.0625, 7.5)
    assert [cm.sees_through(model, o[0, :3], g[0, :3], g[j, :3]) for j in range(1, 7)] == [True, False, False, True, True, True]
    want, stats = _check_passes(dc, g, o, py, model)
    assert want[1] >= 1 and want[6] == 0 and stats["transient"] == int((want >= 1).sum())  # (the last row passes the pair test and is never offered)
    # the bounds one ulp tighter: `at` is no longer seen through by that ray, by either of them
    for tighter in (dict(end_margin=up(0.5)), dict(rho=float(np.nextafter(f32(0.25), f32(0)))), dict(tan_half_angle=float(np.nextafter(f32(0.5), f32(0))))):
        py, model = _cfg(**{**kw, **tighter})
        assert not cm.sees_through(model, o[0, :3], g[0, :3], g[1, :3])
        less, _ = _check_passes(dc, g, o, py, model)
        assert less[1] < want[1]
    dc.close()


@pytest.fixture(scope="module")
def trail(opt):
    """A wall 6 m in front of three origins and, in the first scan only, a blob half way: the rays of the other two scans to the wall pass through
    where the blob stood."""
    rng = np.random.default_rng(11)
    scans = []
    for k in range(3):
        wall = np.c_[6.05 + 0.1 * k + rng.normal(0, 0.01, 700), rng.uniform(-1.5, 1.5, 700), rng.uniform(-1.0, 1.5, 700)]  # (a layer of voxels per scan)
        scans.append(wall if k else np.concatenate([np.c_[3.0 + rng.normal(0, 0.08, 300), rng.uniform(-0.3, 0.3, 300), rng.uniform(-0.2, 0.9, 300)], wall]))
    origins = np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.25], [0.0, -0.5, 0.125]])
    return scans, origins


def test_min_passes_exactly_met_and_missed_by_one(opt, trail):
    dc, g, o = _store(opt, trail[0], origins=trail[1])
    py, model = _cfg()
    want, stats = _check_passes(dc, g, o, py, model)
    top = int(want.max())
    assert top >= 3
    for m, transient in ((top, int((want == top).sum())), (top + 1, 0), (1, int((want > 0).sum()))):
        py, model = _cfg(min_passes=m)
        w2, s2 = _check_passes(dc, g, o, py, model)
        assert np.array_equal(w2, want) and s2["transient"] == transient and (m > top or transient > 0)
    dc.close()


def test_a_plane_seen_at_ten_degrees_grazing_is_not_carved(opt):
    """Ground at z = 0.05 seen from three origins one metre above it at 5 to 8 m: the rays land at 7 to 12 degrees.  From a ray's endpoint the
    ground lies at that angle from the ray, outside the default cone of 3 degrees: no ray sees through a single row."""
    rng = np.random.default_rng(13)
    origins = np.array([[0.0, 0.0, 1.05], [0.5, 1.0, 1.05], [-0.5, -1.0, 1.05]])
    scans = [np.c_[rng.uniform(5.0, 7.0, 600), rng.uniform(-1.5, 1.5, 600), np.full(600, 0.05)] for _ in range(3)]
    dc, g, o = _store(opt, scans, origins=origins)
    graze = np.degrees(np.arctan2(o[:, 2] - g[:, 2], np.linalg.norm(g[:, :2] - o[:, :2], axis=1)))
    assert g.shape[0] > 450 and 6.5 < graze.min() < 9.0 and 10.0 < graze.max() < 13.0
    py, model = _cfg()
    want, stats = _check_passes(dc, g, o, py, model)
    assert stats["transient"] == 0 and stats["seen_through"] == 0 and stats["pair_tests"] > 10 * g.shape[0]
    # the plain voxel-carving cone would erode it: at 10 degrees half-angle the same ground loses rows
    py, model = _cfg(tan_half_angle=0.3, min_passes=1)
    _, wide = _check_passes(dc, g, o, py, model)
    assert wide["transient"] > 100
    dc.close()


# ---- 5. removal ---------------------------------------------------------------------------------------------------------------------------------------
def test_remove_transients_compacts_points_and_origins_and_later_calls_follow(opt, trail, tmp_path):
    from dmsa_lidar_slam_amd.api import DmsaError
    from dmsa_lidar_slam_amd.dense_cloud import normal_from_moments, pcdHeaderXyzBinary

    def refused(call, text="no pass counts of the store as it stands"):
        with pytest.raises(DmsaError) as e:
            call()
        assert e.value.status == -1 and text in e.value.args[0], e.value.args[0]

    scans, origins = trail
    dc, g, o = _store(opt, scans, origins=origins)
    refused(dc.remove_transients)  # nothing counted yet
    py, model = _cfg()
    want, stats = _check_passes(dc, g, o, py, model)
    blob = g[:, 0] < 4.0
    assert 60 < blob.sum() and stats["transient"] > 0.5 * blob.sum() and (want[~blob] >= 2).sum() < 0.01 * (~blob).sum()
    # a scan added after the count: the removal is refused until the count runs again
    far = np.c_[np.full(40, 6.0), np.linspace(3.0, 4.0, 40), np.linspace(0.0, 1.0, 40)]
    dc.add_scan((far - origins[2]).astype(f32), np.linspace(base.S[4] + 0.01, base.S[5] - 0.01, 40))
    refused(dc.remove_transients)
    g, o = dc.retained()
    want, stats = _check_passes(dc, g, o, py, model)
    # O6 in between: its compaction makes the counts stale, and the counts' compaction the classification
    o_flags, o_stats, _ = om.classify(g, 0.4, 8, 1.0)
    assert dc.classify_outliers(0.4, 8, 1.0) == o_stats and dc.remove_outliers() == o_stats["inliers"]
    refused(dc.remove_transients)
    g, o = g[o_flags.astype(bool)], o[o_flags.astype(bool)]
    want, stats = _check_passes(dc, g, o, py, model)
    assert dc.classify_outliers(0.4, 8, 1.0)["rows"] == g.shape[0]
    slots, occupied = dc.table_info()
    before = dc.stats()
    # the removal
    keep = want < 2
    assert dc.remove_transients() == stats["kept"] == int(keep.sum()) == dc.retained_count() < g.shape[0]
    g2, o2 = dc.retained()
    assert np.array_equal(_bits(g2), _bits(g[keep])) and np.array_equal(_bits(o2), _bits(o[keep])) and len(np.unique(o2[:, :3], axis=0)) == 3
    assert dc.table_info() == (slots, occupied) and dc.stats() == before  # T7: the voxel set and the scan statistics are untouched
    refused(dc.remove_transients)  # a second removal: the counts were of the store before
    refused(dc.remove_outliers, "no classification of the store as it stands")
    # the file of the cleaned store, byte for byte
    path = tmp_path / "Carved.pcd"
    points, size = dc.save_pcd_retained(path)
    raw = open(path, "rb").read()
    assert raw == pcdHeaderXyzBinary(g2.shape[0]).encode() + np.ascontiguousarray(g2[:, :3]).tobytes() and (points, size) == (g2.shape[0], len(raw))
    # normals and the outlier classification of the cleaned store
    normals, without = dc.compute_normals(0.4, 5)
    ref_n = normal_from_moments(nm.moments(g2, 0.4), nm.view_vectors(g2, o2), 5)
    assert np.array_equal(_bits(normals), _bits(ref_n)) and without == int(np.isnan(ref_n[:, 0]).sum())
    want_flags, want_o, _ = om.classify(g2, 0.4, 8, 1.0)
    got_o, flags = dc.classify_outliers(0.4, 8, 1.0, download=True)
    assert got_o == want_o and np.array_equal(flags, want_flags)
    # ... and the cleaned store counts like any other: what is left of the trail has fewer rays through it
    want3, stats3 = _check_passes(dc, g2, o2, py, model)
    assert stats3["rows"] == g2.shape[0]
    dc.close()


def test_two_fresh_objects_give_the_same_passes_bytes(opt, trail):
    out = []
    for _ in range(2):
        dc, g, o = _store(opt, trail[0], origins=trail[1])
        stats, passes = dc.count_passes(download=True)
        cells, hashes = dc.carve_walk_rows()
        left = dc.remove_transients()
        g2, _ = dc.retained()
        out.append((stats, passes.tobytes(), cells.tobytes(), hashes.tobytes(), left, g2.tobytes()))
        dc.close()
    assert out[0] == out[1] and out[0][0]["seen_through"] > 0


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_every_breach_of_t1_is_refused_with_its_reason(opt):
    from dmsa_lidar_slam_amd.api import DmsaError
    from dmsa_lidar_slam_amd.dense_cloud import DenseCarveConfig as Cfg

    def refused(call, text):
        with pytest.raises(DmsaError) as e:
            call()
        assert e.value.status == -1 and text in e.value.args[0], e.value.args[0]

    rng = np.random.default_rng(44)
    xyz = ng._one_per_voxel(rng, 100, VOXEL, 8, corner=(1.0, 0.0, 0.0))
    off, _ = ng._creator(opt, retain=False, still=True, voxel_size=VOXEL)
    off.add_scan(xyz, ng._stamps(100))
    for call in (off.count_passes, off.carve_walk_rows):
        refused(call, "retention is off")
    refused(off.remove_transients, "no pass counts")
    off.close()
    empty, _ = ng._creator(opt, still=True, voxel_size=VOXEL)
    refused(empty.count_passes, "no retained point")
    refused(empty.carve_walk_rows, "no retained point")
    empty.close()
    no_voxel, _ = ng._creator(opt, still=True, voxel_size=0.0)
    no_voxel.add_scan(xyz, ng._stamps(100))
    refused(no_voxel.count_passes, "voxel_size must be > 0")
    no_voxel.close()
    dc, _ = ng._still_cloud(opt, xyz, VOXEL)
    for call in (dc.count_passes, dc.carve_walk_rows):
        refused(lambda: call(Cfg(cell_size=np.inf)), "cell_size is not finite")
        refused(lambda: call(Cfg(cell_size=np.nan)), "cell_size is not finite")
        refused(lambda: call(Cfg(cell_size=float(np.nextafter(f32(VOXEL), f32(0))))), "[voxel_size, 64 * voxel_size]")
        refused(lambda: call(Cfg(cell_size=float(np.nextafter(f32(64.0) * f32(VOXEL), f32(10))))), "[voxel_size, 64 * voxel_size]")
        refused(lambda: call(Cfg(rho=np.inf)), "must be finite")
        refused(lambda: call(Cfg(rho=0.0)), "rho must be > 0")
        refused(lambda: call(Cfg(end_margin=0.0)), "end_margin must be > 0")
        refused(lambda: call(Cfg(start_margin=-0.5)), "start_margin must be >= 0")
        refused(lambda: call(Cfg(max_length=0.0)), "max_length must be > 0")
        refused(lambda: call(Cfg(tan_half_angle=0.0)), "tan_half_angle must lie in (0, 1]")
        refused(lambda: call(Cfg(tan_half_angle=1.5)), "tan_half_angle must lie in (0, 1]")
        refused(lambda: call(Cfg(min_passes=0)), "min_passes must lie in [1, 2^20]")
        refused(lambda: call(Cfg(min_passes=2**20 + 1)), "min_passes must lie in [1, 2^20]")
    refused(lambda: dc.carve_walk_rows(None, 90, 11), "beyond the retained store")
    # a refused call is no count; the bounds themselves are legal
    refused(dc.remove_transients, "no pass counts")
    assert dc.count_passes(Cfg(cell_size=VOXEL, tan_half_angle=1.0, start_margin=0.0, min_passes=2**20))["rows"] == 100
    assert dc.count_passes(Cfg(cell_size=float(f32(64.0) * f32(VOXEL)), min_passes=1))["rows"] == 100 and dc.remove_transients() <= 100
    dc.close()


# ---- 7. the demo ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_demo_carves_then_removes_outliers_then_writes_normals(tmp_path):
    """The three stages in their order: the carved file holds what carving kept, the cleaned file the inliers among those, the seven-field file
    the same rows as the cleaned one."""
    import os
    import re
    import subprocess
    import sys

    out = {n: tmp_path / f"{n}.pcd" for n in ("Dense", "Carved", "Clean", "Normals")}
    p = subprocess.run([sys.executable, os.path.join(og.ROOT, "examples", "dense_cloud_demo.py"), "--scans", "6", "--carve", "0.2", "0.1", "1", "--outliers", "8", "1.0", "--normals",
                        "0.3", "--out", str(out["Dense"]), "--carved-out", str(out["Carved"]), "--clean-out", str(out["Clean"]), "--normals-out", str(out["Normals"])],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    carve = re.search(r"carve \(cell 0.2 m, rho 0.1 m, passes 1\): rows (\d+)  rays_walked (\d+)  rays_skipped (\d+) .* transient (\d+)  kept (\d+)", p.stdout)
    rows, walked, skipped, transient, kept = (int(v) for v in carve.groups())
    assert rows == int(re.search(r"\bkept (\d+)", p.stdout).group(1)) == walked + skipped == transient + kept > 2000 and walked > 0
    lines = p.stdout.splitlines()
    assert [i for i, l in enumerate(lines) if l.startswith("carve (")][0] < [i for i, l in enumerate(lines) if l.startswith("outliers (")][0]
    o_rows, inliers = int(re.search(r"outliers .*\brows (\d+)", p.stdout).group(1)), int(re.search(r"\binliers (\d+)", p.stdout).group(1))
    assert o_rows == kept and 0 < inliers < kept  # the outlier statistic saw the carved store
    _, carved, _ = og._read_xyz(out["Carved"])
    _, clean, _ = og._read_xyz(out["Clean"])
    _, body, _ = ng._read_pcd7(out["Normals"])
    assert carved.shape[0] == kept and clean.shape[0] == inliers == body.shape[0] and np.array_equal(_bits(clean), _bits(body[:, :3]))
