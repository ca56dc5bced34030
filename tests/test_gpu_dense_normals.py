"""GPU tests of include/dmsa_dense_normals.h against the numpy model of N0-N4 (tests/dense_normals_model.py).

Retention: the store against the add_scan outputs and the model's origins on the DEVICE's poses, bit for bit.  Moments: the ten int64 sums
against the brute-force model, bit for bit -- a neighbour missed at a cell face or a tile seam changes them.  Normals: the device against the
library's host function of N4 (checked against eigh in tests/test_dense_normals_cpu.py) on the model's moments, bit for bit.

k_neighbour_moments streams its candidates in tiles of 64 rows (kGridTile: one candidate per lane of a wave) and gives a wave 64 queries:
the one-cell cloud below holds 1 500 rows, more than twice the tile and more than one wave of queries."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dense_normals_model as nm
import test_gpu_dense_cloud as base
import wire_util

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 64


@pytest.fixture(scope="module")
def opt():
    from dmsa_lidar_slam_amd.api import DmsaOptimizer

    o = DmsaOptimizer(device=0)
    yield o
    o.close()


def _creator(opt, retain=True, still=False, lidar_to_imu=None, **gates):
    from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator

    s, p, q = base._still_trajectory() if still else (base.S, base.P, base.Q)
    g = dict(min_range=0.0, max_range=0.0, time_offset=0.0, max_pose_gap=0.0, voxel_size=0.0)
    g.update(gates)
    cfg = DenseCloudConfig(lidarToImu=np.eye(4, dtype=f32) if lidar_to_imu is None else lidar_to_imu, minRange=g["min_range"], maxRange=g["max_range"],
                           timeOffset=g["time_offset"], maxPoseGap=g["max_pose_gap"], voxelSize=g["voxel_size"])
    model = nm.RetainModel(s, p, q, lidar_to_imu, g["min_range"], g["max_range"], g["time_offset"], g["max_pose_gap"], g["voxel_size"])
    return DenseCloudCreator(s, p, q, cfg, optimizer=opt, retain=retain), model


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _stamps(n):
    return np.linspace(base.S[0], base.S[-1], n) if n > 1 else np.array([base.S[3]])


def _still_cloud(opt, xyz, voxel, reserve=0):
    """The rows of xyz (n,3) as one scan on the identity trajectory: g = the point itself, so cells and distances can be built by hand."""
    dc, _ = _creator(opt, still=True, voxel_size=voxel)
    if reserve:
        dc.reserve(reserve)
    kept, st = dc.add_scan(np.asarray(xyz, f32), _stamps(len(xyz)))
    return dc, kept


def _one_per_voxel(rng, n, voxel, side_voxels, corner=(0.0, 0.0, 0.0)):
    """n points in n distinct voxels of a cube of side_voxels^3 voxels, each well inside its voxel."""
    pick = rng.choice(side_voxels**3, n, replace=False)
    cells = np.stack([pick // side_voxels**2, (pick // side_voxels) % side_voxels, pick % side_voxels], axis=1)
    return ((cells + rng.uniform(0.2, 0.8, (n, 3))) * voxel + np.asarray(corner)).astype(f32)


# ---- 1. retention -----------------------------------------------------------------------------------------------------------------------------
def test_retained_store_equals_the_scans_and_the_models_origins(opt):
    from dmsa_lidar_slam_amd.api import DmsaError

    dc, model = _creator(opt, lidar_to_imu=base.L2I, voxel_size=0.25, **base.GATES)
    assert dc.retained_count() == 0
    kept = []
    for k in range(3):
        xyz, t = base._scan(1500, 200 + k)
        got, st = dc.add_scan(xyz, t)
        ref_g, ref_o, ref_st = model.add_scan_retained(xyz, t, interpolate=dc.interpolate)
        assert st == ref_st and np.array_equal(_bits(got), _bits(ref_g))
        kept.append(got)
    xyz, org = dc.retained()
    want = np.concatenate(kept)
    assert xyz.shape == org.shape == want.shape and want.shape[0] > 2000 and dc.retained_count() == want.shape[0]
    assert np.array_equal(_bits(xyz), _bits(want))
    assert np.array_equal(_bits(org), _bits(model.ret_o))  # rule 5 for (0, 0, 0) on the device's poses
    assert (org[:, 3] == 1).all() and np.abs(org[:, :3] - base.P.mean(axis=0).astype(f32)).max() < 5.0  # ... which lie along the trajectory
    # a window of the store, and rows beyond it
    a, b = dc.retained(700, 900)
    assert np.array_equal(_bits(a), _bits(want[700:1600])) and np.array_equal(_bits(b), _bits(model.ret_o[700:1600]))
    with pytest.raises(DmsaError) as e:
        dc.retained(want.shape[0] - 1, 2)
    assert e.value.status == -1 and "beyond the retained store" in e.value.args[0]
    # retain after a scan is refused (here: on an object that retains already, and on one that does not)
    with pytest.raises(DmsaError) as e:
        dc.retain()
    assert e.value.status == -1 and "before the first scan" in e.value.args[0]
    dc.close()


def test_a_capacity_refused_scan_leaves_the_store_unchanged(opt):
    from dmsa_lidar_slam_amd.api import DmsaError

    dc, _ = _creator(opt, lidar_to_imu=base.L2I, voxel_size=0.5, **base.GATES)
    first, second = base._scan(2000, 61), base._scan(2500, 62)
    k1, _ = dc.add_scan(*first)
    before = [a.copy() for a in dc.retained()]
    with pytest.raises(DmsaError) as e:
        dc.add_scan(*second, capacity=10)
    assert e.value.status == -1 and dc.lastKept > 10
    after = dc.retained()
    assert dc.retained_count() == k1.shape[0] and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, after))
    k2, _ = dc.add_scan(*second)
    xyz, _ = dc.retained()
    assert np.array_equal(_bits(xyz), _bits(np.concatenate([k1, k2])))
    dc.close()


def test_add_pointcloud2_retains_like_add_scan(opt):
    from dmsa_lidar_slam_amd import wire_formats as wf

    args = dict(lidar_to_imu=base.L2I, min_range=1.5, max_range=60.0, voxel_size=0.5)
    a, _ = _creator(opt, **args)
    b, _ = _creator(opt, **args)
    dec = wf.PointCloud2Decoder("ouster")
    for k in range(2):
        msg, _ = wire_util.make_msg("ouster", 4000 + k, seed=k, stamp=base.T0 + 0.3 + 0.12 * k)
        xyz, st, _ = dec.decode(msg)
        a.add_scan(xyz, st)
        b.add_pointcloud2(msg, "ouster", download=False)
    (ga, oa), (gb, ob) = a.retained(), b.retained()
    assert ga.shape[0] > 2000 and ga.tobytes() == gb.tobytes() and oa.tobytes() == ob.tobytes()
    dec.close(), a.close(), b.close()


def test_an_object_without_retain_is_what_it_was(opt):
    from dmsa_lidar_slam_amd.api import DmsaError

    dc, model = _creator(opt, retain=False, lidar_to_imu=base.L2I, voxel_size=0.25, **base.GATES)
    xyz, t = base._scan(3000, 77)
    kept, st = dc.add_scan(xyz, t)
    ref, ref_st = model.add_scan(xyz, t, interpolate=dc.interpolate)
    assert st == ref_st and np.array_equal(_bits(kept), _bits(ref))  # the bytes the existing tests expect
    for call in (lambda: dc.compute_normals(0.5), lambda: dc.neighbour_moments(0.5), lambda: dc.retained(), lambda: dc.retain()):
        with pytest.raises(DmsaError) as e:
            call()
        assert e.value.status == -1
    with pytest.raises(DmsaError) as e:
        dc.compute_normals(0.5)
    assert "retention is off" in e.value.args[0]
    dc.close()


# ---- 2. moments, bit for bit ---------------------------------------------------------------------------------------------------------------------
VOXEL, RADIUS, MIN_NB = 0.05, 0.2, 5


def _hand_placed():
    """Rows for the cases the kernel can get wrong, each group far from every other group and from the random rows."""
    r, rows, tags = f32(RADIUS), [], {}

    def group(name, pts):
        tags[name] = (len(rows), len(pts))
        rows.extend(pts)

    # coordinates exactly on cell faces, k * r and -k * r (floorf below zero), and between them
    group("faces", [[f32(kx) * r, f32(ky) * r, f32(30.0)] for kx in (-3, -2, -1, 0, 1, 2, 3) for ky in (-1, 0, 1)])
    # a query in the middle of a cell with a neighbour in each of the 27 cells around it (0.55 r per axis: inside the ball, beyond the face)
    # (the centre sits mid-cell on every axis both for a grid of edge r and for one of edge 1.001 r: a few cells from the origin)
    cx, cy, cz = f32(-10.5) * r, f32(10.5) * r, f32(20.5) * r
    s = f32(0.55) * r
    group("all27", [[cx + f32(dx) * s, cy + f32(dy) * s, cz + f32(dz) * s] for dx in (0, -1, 1) for dy in (0, -1, 1) for dz in (0, -1, 1)])
    # d2 == r * r exactly (inside) and one ulp of r further (outside)
    group("edge", [[0.0, 50.0, 50.0], [r, 50.0, 50.0], [-np.nextafter(r, f32(1)), 50.0, 50.0]])
    group("isolated", [[60.0, 60.0, 60.0]])
    # MIN_NB - 1 and MIN_NB rows within reach of each other and of nothing else
    group("four", [[70.0 + 0.055 * k, 70.0 + 0.005 * k * k, 70.0] for k in range(MIN_NB - 1)])
    group("five", [[80.0 + 0.045 * k, 80.0 + 0.004 * k * k, 80.0 - 0.06 * (k % 2)] for k in range(MIN_NB)])
    return np.array(rows, f32), tags


@pytest.fixture(scope="module")
def mixed(opt):
    """Random rows (about 30 neighbours each) with the hand-placed rows mixed in: the object, what it retained, and the model's moments."""
    rng = np.random.default_rng(31)
    hand, tags = _hand_placed()
    rand = _one_per_voxel(rng, 2600, VOXEL, 30, corner=(-0.75, -0.75, -0.75))  # a cube around the origin: negative and positive cells
    xyz = np.concatenate([rand, hand])
    order = rng.permutation(xyz.shape[0])
    dc, kept = _still_cloud(opt, xyz[order], VOXEL)
    g, o = dc.retained()
    where = np.empty(xyz.shape[0], np.int64)
    where[order] = np.arange(xyz.shape[0])  # row of xyz[k] in the store
    ref = nm.moments(g, RADIUS)
    yield dict(dc=dc, g=g, o=o, ref=ref, where=where, n_rand=rand.shape[0], tags=tags, hand=hand)
    dc.close()


def test_the_hand_placed_rows_are_what_they_are_meant_to_be(mixed):
    g, ref, tags, where, n_rand = mixed["g"], mixed["ref"], mixed["tags"], mixed["where"], mixed["n_rand"]
    assert g.shape[0] == n_rand + mixed["hand"].shape[0]  # nothing was thinned: every row has a voxel of its own
    assert np.array_equal(_bits(g[where[n_rand:], :3]), _bits(mixed["hand"]))  # the identity pose places a point where it is

    def rows(name):
        a, k = tags[name]
        return where[n_rand + a : n_rand + a + k]

    r = f32(RADIUS)
    assert 20 < ref[where[:n_rand], 0].mean() < 45
    # the 27 cells of the grid of edge r around the query (and of any grid with an edge a little above r)
    q27 = rows("all27")
    assert ref[q27[0], 0] == 27 and len({tuple(c) for c in np.floor(g[q27, :3] / r).astype(int)}) == 27
    assert len({tuple(c) for c in np.floor(g[q27, :3].astype(np.float64) / (1.001 * float(r))).astype(int)}) == 27
    e0, e1, e2 = g[rows("edge"), :3]
    d_in, d_out = (e1 - e0)[0], (e2 - e0)[0]
    assert f32(d_in * d_in) == f32(r * r) and f32(d_out * d_out) > f32(r * r)
    assert list(ref[rows("edge"), 0]) == [2, 2, 1]
    assert list(ref[rows("isolated")[0]]) == [1] + [0] * 9
    assert (ref[rows("four"), 0] == MIN_NB - 1).all() and (ref[rows("five"), 0] == MIN_NB).all()
    faces = g[rows("faces"), :3]
    assert (faces[:, 0] == np.repeat(f32([-3, -2, -1, 0, 1, 2, 3]) * r, 3)).all() and (ref[rows("faces"), 0] >= 1).all()


def test_moments_equal_the_model_bit_for_bit(mixed):
    dc, ref = mixed["dc"], mixed["ref"]
    n = ref.shape[0]
    got = dc.neighbour_moments(RADIUS)
    assert got.dtype == np.int64 and got.shape == (n, 10)
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert bad.size == 0, (bad[:10], got[bad[:3]], ref[bad[:3]])
    # windows that start and end inside cells (rows are in file order: every window cuts through cells of the sorted order)
    for first, count in ((0, 1), (1, 1), (n - 1, 1), (n // 3, 700), (n - 65, 65), (63, 130), (0, 0)):
        win = dc.neighbour_moments(RADIUS, first, count)
        assert win.shape == (count, 10) and np.array_equal(win, ref[first : first + count]), (first, count)
    # another radius on the same object: the grid is rebuilt
    other = dc.neighbour_moments(0.11, 100, 300)
    assert np.array_equal(other, nm.moments(mixed["g"], 0.11, rows=np.arange(100, 400)))


# ---- 3. kernel boundaries --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [1, 63, 64, 65, 257, 4097])
def test_moments_at_every_total(opt, total):
    rng = np.random.default_rng(total)
    side = 12 if total < 300 else 32
    xyz = _one_per_voxel(rng, total, VOXEL, side, corner=(-0.3, -0.3, -0.3))
    dc, kept = _still_cloud(opt, xyz, VOXEL)
    assert kept.shape[0] == total == dc.retained_count()
    g, _ = dc.retained()
    got, ref = dc.neighbour_moments(RADIUS), nm.moments(g, RADIUS)
    dc.close()
    assert np.array_equal(got, ref)
    if total > 1:
        assert ref[:, 0].max() > 3


def test_one_cell_with_more_rows_than_a_wave_and_two_tiles(opt):
    """radius = 64 voxels; 1 500 rows jittered inside one cell of the search grid: 24 waves of queries, every one of them streaming 24 tiles."""
    rng = np.random.default_rng(5)
    voxel, radius = 0.01, f32(0.01) * f32(64.0)
    n = 1500
    assert n >= 2 * TILE
    xyz = _one_per_voxel(rng, n, voxel, 60, corner=(0.02, 0.02, 0.02))  # inside (0, 0.62)^3: one cell for an edge of r and of 1.001 r
    assert len({tuple(c) for c in np.floor(xyz / radius).astype(int)}) == 1
    dc, kept = _still_cloud(opt, xyz, voxel)
    assert kept.shape[0] == n
    g, _ = dc.retained()
    got, ref = dc.neighbour_moments(float(radius)), nm.moments(g, radius)
    dc.close()
    assert np.array_equal(got, ref) and ref[:, 0].min() > 100 and ref[:, 0].min() < n


def test_two_hundred_cells_of_one_or_two_rows(opt):
    """Sparse cells: a wave packs the queries of dozens of cells; cells two apart along each axis, so most neighbourhoods are a row or two."""
    rng = np.random.default_rng(6)
    r = f32(RADIUS)
    cells = np.stack(np.meshgrid(np.arange(-3, 3), np.arange(-3, 3), np.arange(-3, 3), indexing="ij"), axis=-1).reshape(-1, 3)[:200] * 2
    first = (cells + rng.uniform(0.1, 0.4, (200, 3))) * float(r)
    second = first[::2] + rng.uniform(0.3, 0.5, (100, 3)) * float(r)  # a second row in every other cell
    xyz = np.concatenate([first, second]).astype(f32)
    xyz = xyz[rng.permutation(xyz.shape[0])]
    dc, kept = _still_cloud(opt, xyz, VOXEL)
    assert kept.shape[0] == 300
    g, _ = dc.retained()
    per_cell = np.unique(np.floor(g[:, :3] / r).astype(int), axis=0, return_counts=True)[1]
    assert per_cell.shape[0] == 200 and set(per_cell) == {1, 2}
    got, ref = dc.neighbour_moments(RADIUS), nm.moments(g, RADIUS)
    dc.close()
    assert np.array_equal(got, ref) and set(ref[:, 0]) >= {1, 2}


# ---- 4. normals ----------------------------------------------------------------------------------------------------------------------------------
def test_normals_equal_normal_from_moments_on_the_models_moments(mixed):
    from dmsa_lidar_slam_amd.dense_cloud import normal_from_moments

    dc, g, o, ref = mixed["dc"], mixed["g"], mixed["o"], mixed["ref"]
    got, without = dc.compute_normals(RADIUS, MIN_NB)
    want = normal_from_moments(ref, nm.view_vectors(g, o), MIN_NB)
    assert got.shape == want.shape == (g.shape[0], 4)
    assert np.array_equal(_bits(got), _bits(want))  # NaN rows in the same places, with the same bits
    nan = np.isnan(got).any(axis=1)  # (a neighbourhood on a line has enough rows and no plane: eigen33's NaNs, not counted)
    few = ref[:, 0] < MIN_NB
    assert without == int(few.sum()) and 0 < without < 0.1 * g.shape[0]
    assert (_bits(got[few]) == 0x7FC00000).all() and nan[few].all() and int(nan.sum()) - without < 10
    a, k = mixed["tags"]["four"]
    assert nan[mixed["where"][mixed["n_rand"] + a : mixed["n_rand"] + a + k]].all()
    a, k = mixed["tags"]["five"]
    assert not nan[mixed["where"][mixed["n_rand"] + a : mixed["n_rand"] + a + k]].any()
    ok = ~nan
    assert np.abs(np.linalg.norm(got[ok, :3].astype(np.float64), axis=1) - 1.0).max() < 1e-6 and (got[ok, 3] >= 0).all() and (got[ok, 3] <= 0.34).all()
    w = nm.view_vectors(g, o)[ok]
    assert ((w[:, 0] * got[ok, 0] + w[:, 1] * got[ok, 1]) + w[:, 2] * got[ok, 2] >= 0).all()  # toward the sensor
    # another threshold: only the NaN rows change
    got3, without3 = dc.compute_normals(RADIUS, 0)
    assert without3 == int((ref[:, 0] < 3).sum()) < without
    assert np.array_equal(_bits(got3[~few]), _bits(got[~few]))


def test_normals_on_a_moving_trajectory_point_at_the_sensor(opt):
    """Three scans of a wall seen while the sensor moves (segment 4 of the trajectory: one rotation, the position moving): origins differ per
    point, every normal faces its own origin."""
    from dmsa_lidar_slam_amd.dense_cloud import normal_from_moments

    dc, model = _creator(opt, lidar_to_imu=base.L2I, voxel_size=0.1, min_range=0.5)
    rng = np.random.default_rng(9)
    for k in range(3):
        n = 1500
        xyz = np.zeros((n, 4), f32)
        xyz[:, 0], xyz[:, 1:3] = 6.0 + rng.normal(0, 0.01, n), rng.uniform(-1.5, 1.5, (n, 2))  # a wall 6 m in front of the sensor
        t = np.sort(rng.uniform(base.S[4], base.S[5], n))
        dc.add_scan(xyz, t)
    g, o = dc.retained()
    got, without = dc.compute_normals(0.4, 5)
    want = normal_from_moments(nm.moments(g, 0.4), nm.view_vectors(g, o), 5)
    dc.close()
    assert g.shape[0] > 1000 and np.array_equal(_bits(got), _bits(want))
    ok = ~np.isnan(got).any(axis=1)
    w = nm.view_vectors(g, o)[ok]
    assert ok.mean() > 0.5 and ((w[:, 0] * got[ok, 0] + w[:, 1] * got[ok, 1]) + w[:, 2] * got[ok, 2] >= 0).all()
    assert len(np.unique(o[:, :3], axis=0)) > 800  # an origin per stamp


# ---- 5. repeatability, staleness, refusals ------------------------------------------------------------------------------------------------------------
def test_two_fresh_objects_give_the_same_bytes_whatever_the_table_size(opt):
    rng = np.random.default_rng(41)
    xyz = _one_per_voxel(rng, 3000, VOXEL, 32)
    out = []
    for reserve in (0, 30000):
        dc, _ = _still_cloud(opt, xyz, VOXEL, reserve=reserve)
        normals, without = dc.compute_normals(RADIUS, MIN_NB)
        out.append((dc.neighbour_moments(RADIUS).tobytes(), normals.tobytes(), without, dc.retained()[0].tobytes()))
        dc.close()
    assert out[0] == out[1]


def _read_pcd7(path):
    raw = open(path, "rb").read()
    end = raw.index(b"DATA binary\n") + len(b"DATA binary\n")
    return raw[:end].decode(), np.frombuffer(raw[end:], "<f4").reshape(-1, 7), len(raw)


def test_a_scan_after_compute_makes_save_fail_until_compute_runs_again(opt, tmp_path):
    from dmsa_lidar_slam_amd.api import DmsaError

    rng = np.random.default_rng(43)
    xyz = _one_per_voxel(rng, 1200, VOXEL, 24)
    dc, _ = _still_cloud(opt, xyz[:800], VOXEL)
    path = tmp_path / "n.pcd"
    with pytest.raises(DmsaError) as e:
        dc.save_pcd_normals(path)  # nothing computed yet
    assert e.value.status == -1 and "compute_normals first" in e.value.args[0] and not path.exists()
    dc.compute_normals(RADIUS, MIN_NB)
    assert dc.save_pcd_normals(path)[0] == 800
    dc.add_scan(xyz[800:], _stamps(400))
    with pytest.raises(DmsaError) as e:
        dc.save_pcd_normals(path)
    assert e.value.status == -1 and "since the last added scan" in e.value.args[0]
    normals, _ = dc.compute_normals(RADIUS, MIN_NB)
    points, size = dc.save_pcd_normals(path)
    _, body, _ = _read_pcd7(path)
    g, _ = dc.retained()
    dc.close()
    assert points == 1200 == body.shape[0] and np.array_equal(_bits(body[:, :3]), _bits(g[:, :3])) and np.array_equal(_bits(body[:, 3:]), _bits(normals))
    assert np.array_equal(_bits(g[:, :3]), _bits(xyz))  # the new rows are included, behind the old ones


def test_preconditions_are_refused_with_their_reason(opt):
    from dmsa_lidar_slam_amd.api import DmsaError

    def refused(call, text):
        with pytest.raises(DmsaError) as e:
            call()
        assert e.value.status == -1 and text in e.value.args[0], e.value.args[0]

    rng = np.random.default_rng(44)
    xyz = _one_per_voxel(rng, 100, VOXEL, 8)
    empty, _ = _creator(opt, still=True, voxel_size=VOXEL)
    refused(lambda: empty.compute_normals(RADIUS), "no retained point")
    refused(lambda: empty.neighbour_moments(RADIUS), "no retained point")
    empty.close()
    no_voxel, _ = _creator(opt, still=True, voxel_size=0.0)
    no_voxel.add_scan(xyz, _stamps(100))
    refused(lambda: no_voxel.compute_normals(RADIUS), "voxel_size must be > 0")
    no_voxel.close()
    dc, _ = _still_cloud(opt, xyz, VOXEL)
    for call in (dc.compute_normals, dc.neighbour_moments):
        refused(lambda: call(np.inf), "radius is not finite")
        refused(lambda: call(np.nan), "radius is not finite")
        refused(lambda: call(np.nextafter(f32(VOXEL), f32(0))), "[voxel_size, 64 * voxel_size]")
        refused(lambda: call(np.nextafter(f32(64.0) * f32(VOXEL), f32(10))), "[voxel_size, 64 * voxel_size]")
        refused(lambda: call(-1.0), "[voxel_size, 64 * voxel_size]")
    refused(lambda: dc.compute_normals(RADIUS, -1), "min_neighbours")
    refused(lambda: dc.neighbour_moments(RADIUS, 90, 11), "beyond the retained store")
    # the bounds themselves are legal
    assert dc.neighbour_moments(VOXEL).shape == (100, 10) and dc.compute_normals(64.0 * VOXEL)[0].shape == (100, 4)
    dc.close()


# ---- 6. the file ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_file_is_its_header_and_28_byte_rows(mixed, tmp_path):
    from dmsa_lidar_slam_amd.api import DmsaError
    from dmsa_lidar_slam_amd.dense_cloud import pcdHeaderNormalsBinary

    dc, g = mixed["dc"], mixed["g"]
    normals, _ = dc.compute_normals(RADIUS, MIN_NB)
    path = tmp_path / "DenseCloudNormals.pcd"
    points, size = dc.save_pcd_normals(path)
    head, body, file_size = _read_pcd7(path)
    assert head == pcdHeaderNormalsBinary(g.shape[0])
    assert points == g.shape[0] == body.shape[0] and size == file_size == len(head) + 28 * points
    assert np.array_equal(_bits(body[:, :3]), _bits(g[:, :3])) and np.array_equal(_bits(body[:, 3:]), _bits(normals))
    # the path of a directory: refused, nothing left behind
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(DmsaError) as e:
        dc.save_pcd_normals(tmp_path)
    assert e.value.status == -1 and "cannot open" in e.value.args[0] and sorted(os.listdir(tmp_path)) == before
    # the streaming x y z file is independent of all this
    assert dc.save_pcd_normals(path) == (points, size)


# ---- 7. the demo -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_demo_writes_a_seven_field_file_of_the_kept_points(tmp_path):
    out = tmp_path / "Normals.pcd"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dense_cloud_demo.py"), "--scans", "6", "--normals", "0.3", "--normals-out", str(out),
                        "--out", str(tmp_path / "Dense.pcd")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    kept = int(re.search(r"\bkept (\d+)", p.stdout).group(1))
    head, body, _ = _read_pcd7(out)
    fields = dict(line.split(" ", 1) for line in head.splitlines()[1:])
    assert fields["FIELDS"] == "x y z normal_x normal_y normal_z curvature" and int(fields["POINTS"]) == kept == body.shape[0] and kept > 2000
    assert str(out) in p.stdout and np.isfinite(body[:, :3]).all() and np.isfinite(body[:, 3:]).all(axis=1).mean() > 0.5
