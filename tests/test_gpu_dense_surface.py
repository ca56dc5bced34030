"""GPU tests of include/dmsa_dense_surface.h against the model of S2-S9 (tests/dense_surface_model.py).

For every store: the listing (cells, sum, n), all statistics but the table's two, the bytes of the voxel file, and per min_weight the vertices,
the triangles, the mesh statistics and the bytes of the PLY, each array_equal or equal as bytes.  No tolerance anywhere.

Stores are built as tests/test_gpu_dense_carve.py builds them (_store: a trajectory that stands still at a different place for every scan), and
the model is fed the store's own g and o, read back.  k_surface_integrate takes a ray per lane in the grid's sorted order, so the shapes are totals
around the wave and the block (1 / 63 / 64 / 65 / 257 / 4 097), 65 rays sampling one cell, two origins on opposite sides of a thin wall (sums
of mixed sign, and two dyadic rays whose samples in one cell cancel to a sum of exactly 0), a ray shorter than the truncation, skipped rays,
the edge of the 21-bit cell range, a table that starts too small, min_weight 1 against 3, a sphere seen from its centre with the checks of a
closed mesh on the device's own triangles, and a store with intensities.

Skipped rays: L2 == 0 and L > max_length are here.  T2's third case on the segment needs an end beyond 2^31 cells or end cells more than 2^11
apart; a store holds rows within 2^20 voxels of at least 1/64 cell, and a segment spans 32 cells at most, so no retained ray can reach it: that
case is tested on the host through the same header (tests/test_dense_surface_cpu.py).

Not tested here: S1's bound of 2^26 retained rows, a table beyond 2^31 slots, and a mesh beyond 2^31 - 1 vertices or triangles."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_carve_model as cm
import dense_surface_model as sm
import test_dense_surface_cpu as cpu
import test_gpu_dense_carve as cv
import test_gpu_dense_cloud as base
import test_gpu_dense_normals as ng

pytestmark = pytest.mark.gpu

f32 = np.float32
VOXEL = 0.1
ROOT = ng.ROOT
FINE_VOXEL = 0.01
FINE_CELL = float(f32(0.01) * f32(64.0))  # 64 voxels of 1 cm: many rows of one cell
_store = cv._store
_bits = ng._bits


@pytest.fixture(scope="module")
def opt():
    from dmsa_lidar_slam_amd.api import DmsaOptimizer

    o = DmsaOptimizer(device=0)
    yield o
    o.close()


def _cfg(**kw):
    from dmsa_lidar_slam_amd.dense_cloud import DenseSurfaceConfig

    return DenseSurfaceConfig(**kw), sm.Config(**kw)


def _refused(call, text):
    from dmsa_lidar_slam_amd.api import DmsaError

    with pytest.raises(DmsaError) as e:
        call()
    assert e.value.status == -1 and text in e.value.args[0], e.value.args[0]


def _products(dc, tmp_path, weights, tag=""):
    """Everything a built volume gives, as bytes: the listing, the voxel file and per min_weight the mesh, its statistics and the PLY."""
    cells, total, n = dc.surface_cells()
    path = tmp_path / f"tsdf{tag}.pcd"
    assert dc.save_pcd_tsdf(path) == n.size
    out = {"cells": cells.tobytes(), "sum": total.tobytes(), "n": n.tobytes(), "pcd": open(path, "rb").read()}
    for mw in weights:
        stats = dc.extract_mesh(mw)
        ply = tmp_path / f"mesh{tag}_{mw}.ply"
        dc.save_ply_mesh(ply)
        out[f"mesh{mw}"] = (stats, dc.mesh_vertices().tobytes(), dc.mesh_triangles().tobytes(), open(ply, "rb").read())
    return out


def _check(dc, g, o, py, model, tmp_path, weights=None, tag=""):
    """build_surface and extract_mesh against the model in everything; returns (the model's listing, the library's statistics, the meshes)."""
    weights = (model.min_weight,) if weights is None else weights
    want, want_stats = sm.build(g, o, model)
    stats = dc.build_surface(py)
    assert list(stats) == list(sm.STAT_NAMES) + ["table_slots", "table_builds"]
    assert {k: stats[k] for k in sm.STAT_NAMES} == want_stats, [(k, stats[k], want_stats[k]) for k in sm.STAT_NAMES if stats[k] != want_stats[k]]
    slots = stats["table_slots"]
    assert stats["table_builds"] >= 1 and slots >= 64 and slots & (slots - 1) == 0 and 2 * stats["cells"] <= slots
    assert stats["rows"] == g.shape[0] == stats["rays_walked"] + stats["rays_skipped"]
    _refused(dc.mesh_vertices, "no mesh of the volume")  # a new volume has no mesh yet
    cells, total, n = dc.surface_cells()
    assert (cells.dtype, total.dtype, n.dtype) == (np.int32, np.int64, np.uint32)
    for got, ref, name in zip((cells, total, n), want, ("cells", "sum", "n")):
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, np.flatnonzero((got != ref).reshape(got.shape[0], -1).any(axis=1))[:10])
    assert int(n.sum()) == stats["cells_traversed"] - stats["cells_out_of_range"]
    m = cells.shape[0]
    if m > 2:  # a window of the listing
        w = dc.surface_cells(m // 3, m - m // 3 - 1)
        assert all(np.array_equal(a, b[m // 3 : m - 1]) for a, b in zip(w, want))
        _refused(lambda: dc.surface_cells(m - 1, 2), "beyond the listing")
    got = _products(dc, tmp_path, weights, tag)
    assert got["pcd"] == sm.pcd_bytes(want, model)
    meshes = {}
    for mw in weights:
        xyz, faces, mstats = sm.mesh(want, model, mw)
        stats_d, v, t, ply = got[f"mesh{mw}"]
        assert stats_d == mstats, (mw, stats_d, mstats)
        assert v == xyz.tobytes(), (mw, "vertices")
        assert t == faces.tobytes(), (mw, "triangles")
        assert ply == sm.ply_bytes(xyz, faces), (mw, "ply")
        meshes[mw] = (xyz, faces)
    return want, stats, meshes


# ---- 1. every total -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [1, 63, 64, 65, 257, 4097])
def test_surface_at_every_total(opt, tmp_path, total):
    """The cube of voxels two metres in front of four origins of the carve test."""
    rng = np.random.default_rng(total)
    side = 8 if total < 300 else 20
    xyz = ng._one_per_voxel(rng, total, VOXEL, side, corner=(2.0, -0.4, -0.3))
    dc, g, o = _store(opt, cv._split(rng, xyz, 4))
    assert g.shape[0] == total
    py, model = _cfg()
    _, stats, meshes = _check(dc, g, o, py, model, tmp_path, (1, 2))
    assert stats["rays_skipped"] == 0 and stats["cells"] >= 5 and (total < 257 or meshes[1][1].shape[0] > 100)
    if total < 4097:  # ... and cells of one voxel with a truncation of one cell
        py, model = _cfg(cell_size=VOXEL, truncation=VOXEL, max_length=2.6, min_weight=1)
        _check(dc, g, o, py, model, tmp_path, tag="b")
    if total > 2:  # windows of the mesh
        dc.extract_mesh(1)
        v, t = dc.mesh_vertices(), dc.mesh_triangles()
        if t.shape[0] > 2:
            assert np.array_equal(dc.mesh_triangles(1, t.shape[0] - 2), t[1:-1]) and np.array_equal(_bits(dc.mesh_vertices(1, v.shape[0] - 2)), _bits(v[1:-1]))
            _refused(lambda: dc.mesh_triangles(t.shape[0] - 1, 2), "beyond the mesh")
            _refused(lambda: dc.mesh_vertices(v.shape[0], 1), "beyond the mesh")
    dc.close()


# ---- 2. many rays, one cell -------------------------------------------------------------------------------------------------------------------------
def test_65_rays_sample_one_cell(opt, tmp_path):
    """65 rows in one cell seen from one origin: 65 consecutive lanes, across a wave boundary, add to the same few slots."""
    rng = np.random.default_rng(65)
    xyz = ng._one_per_voxel(rng, 65, FINE_VOXEL, 20, corner=(3 * FINE_CELL + 0.1, 0.1, 0.1))
    dc, g, o = _store(opt, [xyz], voxel=FINE_VOXEL, origins=np.array([[0.1, 0.2, 0.3]]))
    assert g.shape[0] == 65
    py, model = _cfg(cell_size=FINE_CELL, truncation=FINE_CELL, min_weight=1)
    (cells, total, n), stats, _ = _check(dc, g, o, py, model, tmp_path, (1, 65, 66))
    at = {tuple(c): (int(s), int(w)) for c, s, w in zip(cells.tolist(), total, n)}
    assert at[(3, 0, 0)][1] == 65 and at[(2, 0, 0)][1] == 65 and at[(2, 0, 0)][0] > 0 > at[(4, 0, 0)][0]
    dc.close()


# ---- 3. a thin wall seen from both sides --------------------------------------------------------------------------------------------------------------
def test_two_origins_on_opposite_sides_of_a_thin_wall(opt, tmp_path):
    """Dyadic numbers (voxel 0.125, cells of 0.25, truncation 0.75): a wall at x = 2.2 seen from x = 0.19 and from x = 4.19, so that what is in
    front for one scan is behind for the other, and one pair of rays along x that end at the same x on either side of one cell's centre plane:
    their samples there are +2731 and -2731, a sum of exactly 0, which is OUTSIDE."""
    rng = np.random.default_rng(3)
    origins = np.array([[0.1875, 0.0625, 0.0625], [4.1875, 0.1875, 0.0625]])
    wall = [np.c_[2.2 + rng.normal(0, 0.01, 300), rng.uniform(0.5, 2.0, 300), rng.uniform(-0.5, 1.0, 300)] for _ in range(2)]
    pair = [np.array([[2.1875, 0.0625, 0.0625]]), np.array([[2.1875, 0.1875, 0.0625]])]
    dc, g, o = _store(opt, [np.concatenate([wall[k], pair[k]]) for k in range(2)], voxel=0.125, origins=origins)
    py, model = _cfg(cell_size=0.25, truncation=0.75, min_weight=1)
    (cells, total, n), stats, meshes = _check(dc, g, o, py, model, tmp_path, (1, 2))
    at = {tuple(c): (int(s), int(w)) for c, s, w in zip(cells.tolist(), total, n)}
    assert at[(8, 0, 0)] == (0, 2) and at[(7, 0, 0)] == (0, 2) and at[(9, 0, 0)] == (0, 2)  # +-2731, +-13653 (a cell further), -+8192
    assert (total > 0).any() and (total < 0).any() and meshes[1][1].shape[0] > 0
    both = [c for c, (s, w) in at.items() if w >= 2 and 1 <= c[1] and 7 <= c[0] <= 9]
    assert len(both) > 20  # cells that both scans sampled
    dc.close()


# ---- 4. a short ray, skipped rays ----------------------------------------------------------------------------------------------------------------------
def test_a_ray_shorter_than_the_truncation_and_skipped_rays(opt, tmp_path):
    """From the origin (0.1, 0.2, 0.3): a point 0.47 m away (its segment starts at the origin), twenty rays of a few metres and two beyond
    max_length.  From a second origin: a point so close that g == o in float (L2 == 0) and ten more rays."""
    rng = np.random.default_rng(4)
    first, second = np.array([0.1, 0.2, 0.3]), np.array([0.5, 2.0, 0.25])
    mid = first + np.c_[rng.uniform(1.0, 5.0, 20), rng.uniform(-3, 3, 20), rng.uniform(-1, 2, 20)]
    far = first + np.array([[9.0, 1.0, 0.5], [-8.5, 2.0, 1.0]])
    near = second + np.concatenate([[[2.0**-30, 0.0, 0.0]], np.c_[rng.uniform(0.5, 3.0, 10), rng.uniform(-2, 2, 10), rng.uniform(-1, 1, 10)]])
    dc, g, o = _store(opt, [np.concatenate([[[0.4, 0.5, 0.1]], mid, far]), near], origins=np.array([first, second]))
    assert g.shape[0] == 34
    length = np.array([cm.ray(o[r, :3], g[r, :3])[2] for r in range(34)])
    assert length[0] < f32(0.6) and (length > 8).sum() == 2 and cm.ray(o[23, :3], g[23, :3])[1] == 0
    py, model = _cfg(max_length=8.0, min_weight=1)
    (cells, _, _), stats, _ = _check(dc, g, o, py, model, tmp_path, (1,))
    assert stats["rays_skipped"] == 3 and cm.cell_of(o[0, :3], 0.2) in {tuple(c) for c in cells.tolist()}  # the short ray's segment begins in the origin's cell
    # max_length exactly the length of one ray: that ray is walked; one ulp less: it is skipped
    at = float(length[7])
    _, exact, _ = _check(dc, g, o, *_cfg(max_length=at, min_weight=1), tmp_path, (1,), tag="b")
    _, below, _ = _check(dc, g, o, *_cfg(max_length=float(np.nextafter(f32(at), f32(0))), min_weight=1), tmp_path, (1,), tag="c")
    assert exact["rays_skipped"] == int((length > f32(at)).sum()) + 1 and below["rays_skipped"] == exact["rays_skipped"] + 1
    dc.close()


# ---- 5. the edge of the cell range ------------------------------------------------------------------------------------------------------------------
def test_cells_at_the_edge_of_the_range(opt, tmp_path):
    """The scene of the carve test: rows in cells up to +-(2^20 - 1), seen from inside the range, so that the segments behind the endpoints leave it.
    The cells out of range are counted and absent from the listing."""
    rng = np.random.default_rng(9)
    edge = (2**20 - 2) * 0.1
    first = np.array([2**20 - 2 - 59, -(2**20), 2**20 - 100])
    cellsv = rng.choice(60**3, 400, replace=False)
    idx = np.stack([cellsv // 3600, (cellsv // 60) % 60, cellsv % 60], axis=1)
    idx = np.concatenate([idx, [[59, 0, 30], [59, 30, 0], [0, 0, 59]]])
    xyz = (first + idx + 0.5) * 0.1
    origins = np.array([[edge - 8.0, -edge + 8.0, edge - 4.0], [edge - 9.0, -edge + 6.0, edge - 2.0], [edge - 7.25, -edge + 7.0, edge - 5.0]])
    dc, g, o = _store(opt, cv._split(rng, xyz, 3), origins=origins)
    assert g.shape[0] >= 400
    py, model = _cfg(cell_size=VOXEL, truncation=0.4, min_weight=1)
    (cells, _, _), stats, _ = _check(dc, g, o, py, model, tmp_path, (1,))
    assert stats["cells_out_of_range"] > 0 and stats["rays_skipped"] == 0 and cells[:, 0].max() == 2**20 - 1 and cells[:, 1].min() == -(2**20)
    dc.close()


# ---- 6. growth, min_weight, determinism ----------------------------------------------------------------------------------------------------------------
def test_a_table_that_starts_too_small_is_doubled_and_changes_nothing(opt, tmp_path):
    rng = np.random.default_rng(257)
    xyz = ng._one_per_voxel(rng, 257, VOXEL, 8, corner=(2.0, -0.4, -0.3))
    dc, g, o = _store(opt, cv._split(rng, xyz, 4))
    py, model = _cfg()
    _, auto, _ = _check(dc, g, o, py, model, tmp_path, (1, 2))
    reference = _products(dc, tmp_path, (1, 2), "auto")
    assert auto["cells"] > 200 and auto["table_builds"] == 1
    py, model = _cfg(initial_slots=64)
    _, small, _ = _check(dc, g, o, py, model, tmp_path, (1, 2), tag="s")
    assert small["table_builds"] > 1 and small["table_slots"] >= 2 * auto["cells"] and {k: small[k] for k in sm.STAT_NAMES} == {k: auto[k] for k in sm.STAT_NAMES}
    assert _products(dc, tmp_path, (1, 2), "auto") == reference
    py, model = _cfg(initial_slots=2**16)
    _, large, _ = _check(dc, g, o, py, model, tmp_path, (1, 2), tag="l")
    assert large["table_builds"] == 1 and large["table_slots"] == 2**16 and _products(dc, tmp_path, (1, 2), "auto") == reference
    dc.close()


@pytest.fixture(scope="module")
def trail():
    """The scene of the carve test: a wall 6 m in front of three origins and, in the first scan only, a blob half way."""
    rng = np.random.default_rng(11)
    scans = []
    for k in range(3):
        far = np.c_[6.05 + 0.1 * k + rng.normal(0, 0.01, 700), rng.uniform(-1.5, 1.5, 700), rng.uniform(-1.0, 1.5, 700)]
        scans.append(far if k else np.concatenate([np.c_[3.0 + rng.normal(0, 0.08, 300), rng.uniform(-0.3, 0.3, 300), rng.uniform(-0.2, 0.9, 300)], far]))
    return scans, np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.25], [0.0, -0.5, 0.125]])


def test_min_weight_1_against_3_drops_tetrahedra_and_vertices(opt, tmp_path, trail):
    dc, g, o = _store(opt, trail[0], origins=trail[1])
    py, model = _cfg()
    (_, _, n), stats, meshes = _check(dc, g, o, py, model, tmp_path, (1, 3, 2**20))
    assert stats["cells_valid"] == int((n >= 2).sum()) and (n < 3).any() and (n >= 3).any()
    assert 0 < meshes[3][1].shape[0] < meshes[1][1].shape[0] and 0 < meshes[3][0].shape[0] < meshes[1][0].shape[0]
    assert meshes[2**20][1].shape[0] == 0 and meshes[2**20][0].shape[0] == 0  # a mesh without a triangle is a legal file: the header alone
    # an extraction replaces the one before it
    dc.extract_mesh(3)
    assert dc.mesh_triangles().tobytes() == meshes[3][1].tobytes()
    dc.extract_mesh(1)
    assert dc.mesh_triangles().tobytes() == meshes[1][1].tobytes()
    for bad in (0, -1, 2**20 + 1):
        _refused(lambda: dc.extract_mesh(bad), "min_weight must lie in [1, 2^20]")
    # a refused extraction changes nothing: the mesh of the last one and the volume are still there
    assert dc.mesh_triangles().tobytes() == meshes[1][1].tobytes() and dc.surface_cells()[2].tobytes() == n.tobytes()
    dc.close()


def test_two_fresh_objects_and_two_builds_of_one_give_the_same_bytes(opt, tmp_path, trail):
    out = []
    for _ in range(2):
        dc, g, o = _store(opt, trail[0], origins=trail[1])
        for _ in range(2):
            stats = dc.build_surface()
            out.append((stats, _products(dc, tmp_path, (1, 2), "same")))
        dc.close()
    assert out[0] == out[1] == out[2] == out[3] and out[0][1]["mesh2"][0]["triangles"] > 100


# ---- 7. a closed surface ----------------------------------------------------------------------------------------------------------------------------------
def test_a_sphere_seen_from_its_centre_gives_a_closed_mesh_on_the_device(opt, tmp_path):
    """4 000 Fibonacci directions, radius 2 m, cell 0.2, truncation 0.6, min_weight 1 (voxels of 5 cm, so that thinning leaves the rays alone): the
    device's own triangles are closed, of genus 0, face the sensor and enclose the sphere's volume to within one cell."""
    centre = np.array([0.03, -0.02, 0.05])
    world = cpu.fibonacci_sphere(4000, 2.0).astype(np.float64) + centre
    dc, g, o = _store(opt, [world], voxel=0.05, origins=np.array([centre]))
    assert g.shape[0] > 3950
    py, model = _cfg(min_weight=1)
    _check(dc, g, o, py, model, tmp_path, (1,))
    dc.extract_mesh(1)
    cpu.check_sphere_mesh(dc.mesh_vertices(), dc.mesh_triangles(), 2.0, 0.2, o[0, :3])
    dc.close()


# ---- 8. intensity -----------------------------------------------------------------------------------------------------------------------------------------
def test_a_store_with_intensities_gives_identical_surface_products(opt, tmp_path, trail):
    from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator

    plain, g, o = _store(opt, trail[0], origins=trail[1])
    plain.build_surface()
    want = _products(plain, tmp_path, (1, 2), "plain")
    plain.close()
    pos = np.repeat(np.concatenate([trail[1], trail[1][-1:]]), 2, axis=0)
    dc = DenseCloudCreator(base.S, pos, np.tile([0.0, 0.0, 0.0, 1.0], (8, 1)), DenseCloudConfig(voxelSize=VOXEL), optimizer=opt, retain=True, intensity=True)
    rng = np.random.default_rng(8)
    for k, world in enumerate(trail[0]):
        local = np.c_[(world - trail[1][k]).astype(f32), rng.uniform(0, 255, world.shape[0]).astype(f32)]
        a, b = base.S[2 * k], base.S[2 * k + 1]
        dc.add_scan(local, np.linspace(a + 0.25 * (b - a), a + 0.75 * (b - a), world.shape[0]))
    gi, oi = dc.retained()
    assert gi.shape[1] == 4 and np.array_equal(_bits(gi[:, :3]), _bits(g[:, :3])) and np.array_equal(_bits(oi[:, :3]), _bits(o[:, :3]))
    dc.build_surface()
    assert _products(dc, tmp_path, (1, 2), "plain") == want
    dc.close()


# ---- 9. validity --------------------------------------------------------------------------------------------------------------------------------------------
def test_building_touches_nothing_and_a_changed_store_makes_volume_and_mesh_stale(opt, tmp_path, trail):
    from dmsa_lidar_slam_amd.dense_cloud import DenseCarveConfig

    dc, g, o = _store(opt, trail[0], origins=trail[1])
    no_volume, no_mesh = "no volume of the store as it stands", "no mesh of the volume as it stands"
    volume_calls = (dc.surface_cells, lambda: dc.save_pcd_tsdf(tmp_path / "v.pcd"), dc.extract_mesh)
    mesh_calls = (dc.mesh_vertices, dc.mesh_triangles, lambda: dc.save_ply_mesh(tmp_path / "m.ply"))
    for call in volume_calls + mesh_calls:  # nothing built yet: extract_mesh before build_surface is refused
        _refused(call, no_volume)
    assert not (tmp_path / "v.pcd").exists() and not (tmp_path / "m.ply").exists()
    normals, without = dc.compute_normals(0.4, 5)
    dc.save_pcd_normals(tmp_path / "n0.pcd")
    carve = DenseCarveConfig()
    c_stats, passes = dc.count_passes(carve, download=True)
    o_stats = dc.build_occupancy()
    occ_before = [a.tobytes() for a in dc.occupancy_cells()]
    dc.save_pcd_occupancy(tmp_path / "o0.pcd")
    py, model = _cfg()
    _check(dc, g, o, py, model, tmp_path)
    for call in mesh_calls:  # (_check leaves a mesh; a new volume has none)
        call()
    dc.build_surface(py)
    for call in mesh_calls:
        _refused(call, no_mesh)
    # the store, the normals, the carve classification and the occupancy map are as they were
    g2, o2 = dc.retained()
    assert np.array_equal(_bits(g2), _bits(g)) and np.array_equal(_bits(o2), _bits(o))
    dc.save_pcd_normals(tmp_path / "n1.pcd")  # (refused if the normals had been invalidated)
    assert open(tmp_path / "n0.pcd", "rb").read() == open(tmp_path / "n1.pcd", "rb").read()
    assert [a.tobytes() for a in dc.occupancy_cells()] == occ_before
    dc.save_pcd_occupancy(tmp_path / "o1.pcd")
    assert open(tmp_path / "o0.pcd", "rb").read() == open(tmp_path / "o1.pcd", "rb").read()
    # a build that S1 refuses changes nothing: volume and mesh of the last build are still there
    dc.extract_mesh(2)
    before = (dc.surface_cells()[1].tobytes(), dc.mesh_triangles().tobytes())
    _refused(lambda: dc.build_surface(_cfg(min_weight=0)[0]), "min_weight must lie in [1, 2^20]")
    assert (dc.surface_cells()[1].tobytes(), dc.mesh_triangles().tobytes()) == before
    # a scan added: every call is refused until the volume is built again
    far = np.c_[np.full(40, 6.0), np.linspace(3.0, 4.0, 40), np.linspace(0.0, 1.0, 40)]
    dc.add_scan((far - trail[1][2]).astype(f32), np.linspace(base.S[4] + 0.01, base.S[5] - 0.01, 40))
    for call in volume_calls + mesh_calls:
        _refused(call, no_volume)
    g, o = dc.retained()
    c_stats, passes = dc.count_passes(carve, download=True)
    _check(dc, g, o, py, model, tmp_path, tag="b")
    # the carve classification outlived the build: the removal is accepted, and makes volume and mesh stale
    assert dc.remove_transients() == c_stats["kept"] < g.shape[0]
    for call in volume_calls + mesh_calls:
        _refused(call, no_volume)
    keep = passes < carve.min_passes
    _check(dc, g[keep], o[keep], py, model, tmp_path, tag="c")
    dc.close()


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_every_breach_of_s1_is_refused_with_its_reason(opt, tmp_path):
    from dmsa_lidar_slam_amd.dense_cloud import DenseSurfaceConfig as Cfg

    rng = np.random.default_rng(44)
    xyz = ng._one_per_voxel(rng, 100, VOXEL, 8, corner=(1.0, 0.0, 0.0))
    off, _ = ng._creator(opt, retain=False, still=True, voxel_size=VOXEL)
    off.add_scan(xyz, ng._stamps(100))
    _refused(off.build_surface, "retention is off")
    _refused(off.surface_cells, "no volume of the store")
    off.close()
    empty, _ = ng._creator(opt, still=True, voxel_size=VOXEL)
    _refused(empty.build_surface, "no retained point")
    empty.close()
    no_voxel, _ = ng._creator(opt, still=True, voxel_size=0.0)
    no_voxel.add_scan(xyz, ng._stamps(100))
    _refused(no_voxel.build_surface, "voxel_size must be > 0")
    no_voxel.close()
    dc, _ = ng._still_cloud(opt, xyz, VOXEL)
    call = dc.build_surface
    _refused(lambda: call(Cfg(cell_size=np.inf)), "cell_size is not finite")
    _refused(lambda: call(Cfg(cell_size=np.nan)), "cell_size is not finite")
    _refused(lambda: call(Cfg(cell_size=float(np.nextafter(f32(VOXEL), f32(0))))), "[voxel_size, 64 * voxel_size]")
    _refused(lambda: call(Cfg(cell_size=float(np.nextafter(f32(64.0) * f32(VOXEL), f32(10))), truncation=7.0)), "[voxel_size, 64 * voxel_size]")
    _refused(lambda: call(Cfg(truncation=np.inf)), "truncation must be finite")
    _refused(lambda: call(Cfg(truncation=np.nan)), "truncation must be finite")
    _refused(lambda: call(Cfg(truncation=float(np.nextafter(f32(0.2), f32(0))))), "truncation must lie in [cell_size, 16 * cell_size]")
    _refused(lambda: call(Cfg(truncation=float(np.nextafter(f32(16.0) * f32(0.2), f32(10))))), "truncation must lie in [cell_size, 16 * cell_size]")
    _refused(lambda: call(Cfg(max_length=np.inf)), "max_length must be finite")
    _refused(lambda: call(Cfg(max_length=np.nan)), "max_length must be finite")
    _refused(lambda: call(Cfg(max_length=0.0)), "max_length must be > 0")
    for bad in (0, -1, 2**20 + 1):
        _refused(lambda: call(Cfg(min_weight=bad)), "min_weight must lie in [1, 2^20]")
    for bad in (1, 32, 96, 2**32, -64):
        _refused(lambda: call(Cfg(initial_slots=bad)), "initial_slots must be 0 or a power of two in [64, 2^31]")
    _refused(dc.surface_cells, "no volume of the store")  # a refused call is no volume
    # the bounds themselves are legal
    s = call(Cfg(cell_size=VOXEL, truncation=VOXEL, min_weight=2**20, initial_slots=64))
    assert s["rows"] == 100 and s["cells_valid"] == 0 and s["cells"] > 0 and dc.extract_mesh(2**20) == dict(tetrahedra_meshed=0, vertices=0, triangles=0)
    assert call(Cfg(cell_size=float(f32(64.0) * f32(VOXEL)), truncation=float(f32(16.0) * (f32(64.0) * f32(VOXEL)))))["cells"] >= 1
    dc.extract_mesh(1)
    _refused(lambda: dc.save_pcd_tsdf(tmp_path / "no" / "such" / "dir.pcd"), "dense surface")
    _refused(lambda: dc.save_ply_mesh(tmp_path / "no" / "such" / "dir.ply"), "dense surface")
    dc.close()


# ---- 11. the two programs -----------------------------------------------------------------------------------------------------------------------------------
def test_the_program_without_python_writes_the_same_ply_as_the_demo(tmp_path):
    """The demo's recording through both programs: the same PLY and the same voxel file, byte for byte, and the PLY is a mesh."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import dense_cloud_demo
    from dmsa_lidar_slam_amd.dense_cloud import DenseSurfaceConfig

    r = dense_cloud_demo.run(scans=6, workdir=str(tmp_path), mesh=DenseSurfaceConfig(cell_size=0.4, truncation=1.2, min_weight=2), tsdf_out=str(tmp_path / "py_tsdf.pcd"))
    assert r["mesh"]["triangles"] > 500 and r["surface"]["cells"] > 1000
    exe = os.path.join(ROOT, "examples", "dense_cloud_from_raw")
    ply, tsdf = tmp_path / "cpp.ply", tmp_path / "cpp_tsdf.pcd"
    p = subprocess.run([exe, r["dump"], r["poses_file"], "ouster", str(tmp_path / "cpp.pcd"), "--voxel", "0.1", "--min-range", "0.5", "--mesh", str(ply), "--surface-cell", "0.4",
                        "--surface-trunc", "1.2", "--surface-min-weight", "2", "--tsdf-out", str(tsdf)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
    assert f"vertices {r['mesh']['vertices']}  triangles {r['mesh']['triangles']}" in p.stdout
    raw = open(ply, "rb").read()
    assert raw == open(r["mesh_ply"], "rb").read() and open(tsdf, "rb").read() == open(r["tsdf_pcd"], "rb").read()
    head = sm.ply_header(r["mesh"]["vertices"], r["mesh"]["triangles"]).encode()
    assert raw.startswith(head) and len(raw) == len(head) + 12 * r["mesh"]["vertices"] + 13 * r["mesh"]["triangles"]
