"""GPU tests of include/dmsa_dense_occupancy.h against the model of M2-M7 (tests/dense_occupancy_model.py).

For every store: the listing (cells, hits, passes, state), all statistics but the table's two, the bytes of the voxel file at every min_state and
the bytes of the slice, its PGM and its YAML, each array_equal or equal as bytes.  No tolerance anywhere.

Stores are built as tests/test_gpu_dense_carve.py builds them (_store: a trajectory that stands still at a different place for every scan), and
the model is fed the store's own g and o, read back.  The kernel takes a ray per lane in the grid's sorted order and merges equal cells within
a wave, so the shapes are totals around the wave and the block (1 / 63 / 64 / 65 / 257 / 4 097), 65 rays into one cell, two origins whose rays
share a cell in one step as endpoint and as pass-through, a ray of one cell, a ray through lattice corners, skipped rays, the largest extent, the
edge of the 21-bit cell range, and a table that starts too small.

The corner ray of cell_size 0.2 from (0.1, 0.1, 0.1) to (0.5, 0.5, 0.1) runs from X = 1025 to X = 5119 on x and y alike (float32(0.5) / float32(0.2)
lies just below 2.5): both axes cross 2048 and 4096 together.

Not tested here: the M1 bound of 2^26 retained rows (a store of 2 GiB) and a table beyond 2^31 slots."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_carve_model as cm
import dense_occupancy_model as occ
import test_gpu_dense_carve as cv
import test_gpu_dense_cloud as base
import test_gpu_dense_normals as ng

pytestmark = pytest.mark.gpu

f32 = np.float32
VOXEL = 0.1
ORIGINS = cv.ORIGINS
ROOT = ng.ROOT
EVERYTHING = (-3.0e5, 3.0e5)  # a slab that holds every cell there is
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
    from dmsa_lidar_slam_amd.dense_cloud import DenseOccupancyConfig

    return DenseOccupancyConfig(**kw), occ.Config(**kw)


def _refused(call, text):
    from dmsa_lidar_slam_amd.api import DmsaError

    with pytest.raises(DmsaError) as e:
        call()
    assert e.value.status == -1 and text in e.value.args[0], e.value.args[0]


def _products(dc, tmp_path, slabs, tag=""):
    """Everything a built map gives, as bytes: the listing, the three files, and per slab the info, the pixels and the two map files."""
    cells, hits, passes, state = dc.occupancy_cells()
    out = {"cells": cells.tobytes(), "hits": hits.tobytes(), "passes": passes.tobytes(), "state": state.tobytes()}
    for ms in (0, 1, 2):
        path = tmp_path / f"occ{tag}_{ms}.pcd"
        rows = dc.save_pcd_occupancy(path, ms)
        out[f"pcd{ms}"] = open(path, "rb").read()
        assert rows == int((state >= ms).sum())
    for k, (lo, hi) in enumerate(slabs):
        try:
            info, pixels = dc.occupancy_slice(lo, hi)
        except Exception as e:  # noqa: BLE001
            out[f"slice{k}"] = ("refused", getattr(e, "status", None))
            continue
        pgm, yaml = tmp_path / f"map{tag}_{k}.pgm", tmp_path / f"map{tag}_{k}.yaml"
        dc.save_occupancy_map(pgm, yaml, lo, hi)
        out[f"slice{k}"] = (info, pixels.tobytes(), open(pgm, "rb").read(), open(yaml, "rb").read())
    return out


def _check(dc, g, o, py, model, tmp_path, slabs=(EVERYTHING,), tag=""):
    """build_occupancy against the model in everything; returns (the model's listing, the library's statistics)."""
    want, want_stats = occ.build(g, o, model)
    stats = dc.build_occupancy(py)
    assert list(stats) == list(occ.STAT_NAMES) + ["table_slots", "table_builds"]
    assert {n: stats[n] for n in occ.STAT_NAMES} == want_stats, [(n, stats[n], want_stats[n]) for n in occ.STAT_NAMES if stats[n] != want_stats[n]]
    slots = stats["table_slots"]
    assert stats["table_builds"] >= 1 and slots >= 64 and slots & (slots - 1) == 0 and 2 * stats["cells"] <= slots
    assert stats["rows"] == g.shape[0] == stats["rays_walked"] + stats["rays_skipped"] and stats["cells"] == stats["occupied"] + stats["free"] + stats["unknown"]
    cells, hits, passes, state = dc.occupancy_cells()
    assert (cells.dtype, hits.dtype, passes.dtype, state.dtype) == (np.int32, np.uint32, np.uint32, np.uint8) and dc.occupancy_count() == want[0].shape[0]
    for got, ref, name in zip((cells, hits, passes, state), want, ("cells", "hits", "passes", "state")):
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, np.flatnonzero((got != ref).reshape(got.shape[0], -1).any(axis=1))[:10])
    assert int(hits.sum()) + int(passes.sum()) == stats["cells_traversed"] - stats["cells_out_of_range"] and int(hits.sum()) <= stats["rays_walked"]
    m = cells.shape[0]
    if m > 2:  # a window of the listing
        w = dc.occupancy_cells(m // 3, m - m // 3 - 1)
        assert all(np.array_equal(a, b[m // 3 : m - 1]) for a, b in zip(w, want))
        _refused(lambda: dc.occupancy_cells(m - 1, 2), "beyond the listing")
    got = _products(dc, tmp_path, slabs, tag)
    for ms in (0, 1, 2):
        assert got[f"pcd{ms}"] == occ.pcd_bytes(want, model, ms), ms
    for k, (lo, hi) in enumerate(slabs):
        ref = occ.slice_of(want, model, lo, hi)
        if ref is None:
            assert got[f"slice{k}"] == ("refused", -1), (lo, hi)
            continue
        info, pixels, pgm, yaml = got[f"slice{k}"]
        assert info == ref[0], (lo, hi, info, ref[0])
        assert pixels == ref[1].tobytes() and pgm == occ.pgm_bytes(ref[1])
        assert yaml.decode() == occ.yaml_text(f"map{tag}_{k}.pgm", model.cell_size, ref[0]["cx_min"], ref[0]["cy_min"])
        assert info["occupied"] + info["free"] + info["unknown"] == info["width"] * info["height"]
    return want, stats


# ---- 1. every total -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [1, 63, 64, 65, 257, 4097])
def test_map_at_every_total(opt, tmp_path, total):
    """The cube of voxels two metres in front of four origins of the carve test."""
    rng = np.random.default_rng(total)
    side = 8 if total < 300 else 20
    xyz = ng._one_per_voxel(rng, total, VOXEL, side, corner=(2.0, -0.4, -0.3))
    dc, g, o = _store(opt, cv._split(rng, xyz, 4))
    assert g.shape[0] == total
    py, model = _cfg()
    want, stats = _check(dc, g, o, py, model, tmp_path, (EVERYTHING, (0.0, 0.25)))
    assert stats["rays_skipped"] == 0 and stats["cells"] > 10 and (total < 257 or (stats["occupied"] > 0 and stats["free"] > 0 and stats["unknown"] > 0))
    if total < 4097:  # ... and cells of one voxel with other thresholds
        py, model = _cfg(cell_size=VOXEL, min_hits=2, min_passes=3, occ_num=3, occ_den=2, max_length=2.6)
        _check(dc, g, o, py, model, tmp_path, tag="b")
    dc.close()


# ---- 2. the wave merge ----------------------------------------------------------------------------------------------------------------------------
def _along_x(rng, n, cell_x):
    """n points in n voxels of cell (cell_x, 0, 0) of the fine grid."""
    return ng._one_per_voxel(rng, n, FINE_VOXEL, 20, corner=(cell_x * FINE_CELL + 0.1, 0.1, 0.1))


def test_65_rays_from_one_origin_into_one_cell(opt, tmp_path):
    """The 65 rows lie in one cell, so they are 65 consecutive lanes, across a wave boundary: the endpoint's cell holds 65 hits, the origin's 65
    passes, and so does every cell between them."""
    rng = np.random.default_rng(65)
    dc, g, o = _store(opt, [_along_x(rng, 65, 3)], voxel=FINE_VOXEL, origins=np.array([[0.1, 0.2, 0.3]]))
    assert g.shape[0] == 65
    py, model = _cfg(cell_size=FINE_CELL)
    (cells, hits, passes, state), stats = _check(dc, g, o, py, model, tmp_path)
    assert cells.tolist() == [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]] and hits.tolist() == [0, 0, 0, 65] and passes.tolist() == [65, 65, 65, 0]
    assert state.tolist() == [1, 1, 1, 2] and stats["cells_traversed"] == 4 * 65
    dc.close()


def test_two_origins_share_a_cell_as_endpoint_and_as_pass_through_in_one_step(opt, tmp_path):
    """65 rays end in cell (2, 0, 0), 65 more from a second origin go through it into (3, 0, 0), both in their third step.  Sorted by cell, the
    second wave holds one lane of the first kind beside 63 of the second: the two counters of the cell stay apart."""
    rng = np.random.default_rng(66)
    origins = np.array([[0.1, 0.2, 0.3], [0.3, 0.4, 0.2]])
    dc, g, o = _store(opt, [_along_x(rng, 65, 2), _along_x(rng, 65, 3)], voxel=FINE_VOXEL, origins=origins)
    assert g.shape[0] == 130
    py, model = _cfg(cell_size=FINE_CELL)
    (cells, hits, passes, state), _ = _check(dc, g, o, py, model, tmp_path)
    assert cells.tolist() == [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]] and hits.tolist() == [0, 0, 65, 65] and passes.tolist() == [130, 130, 65, 0]
    dc.close()


def test_a_cell_hit_once_and_crossed_by_17_rays_is_free_at_16_and_occupied_at_32(opt, tmp_path):
    rng = np.random.default_rng(67)
    origins = np.array([[0.1, 0.2, 0.3], [0.3, 0.4, 0.2]])
    dc, g, o = _store(opt, [_along_x(rng, 1, 2), _along_x(rng, 17, 3)], voxel=FINE_VOXEL, origins=origins)
    assert g.shape[0] == 18
    py, model = _cfg(cell_size=FINE_CELL)
    (cells, hits, passes, state), _ = _check(dc, g, o, py, model, tmp_path)
    assert cells[2].tolist() == [2, 0, 0] and (hits[2], passes[2], state[2]) == (1, 17, occ.FREE)
    py, model = _cfg(cell_size=FINE_CELL, occ_num=32)
    (_, _, _, state), _ = _check(dc, g, o, py, model, tmp_path, tag="b")
    assert state[2] == occ.OCCUPIED
    py, model = _cfg(cell_size=FINE_CELL, occ_num=17)  # 17 * 1 <= 1 * 17: the comparison at equality
    (_, _, _, state), _ = _check(dc, g, o, py, model, tmp_path, tag="c")
    assert state[2] == occ.OCCUPIED
    dc.close()


# ---- 3. single rays ---------------------------------------------------------------------------------------------------------------------------------
def test_a_ray_inside_one_cell_is_one_hit_and_a_one_pixel_image(opt, tmp_path):
    dc, g, o = _store(opt, [np.array([[0.4, 0.5, 0.1]])], voxel=FINE_VOXEL, origins=np.array([[0.1, 0.2, 0.3]]))
    py, model = _cfg(cell_size=FINE_CELL)
    (cells, hits, passes, state), stats = _check(dc, g, o, py, model, tmp_path, (EVERYTHING, (0.0, 0.0), (-1.0, -0.1)))
    assert (cells.tolist(), hits.tolist(), passes.tolist(), state.tolist()) == ([[0, 0, 0]], [1], [0], [2]) and stats["cells_traversed"] == 1
    info, pixels = dc.occupancy_slice(0.0, 0.0)
    assert (info["width"], info["height"], info["occupied"], info["free"], info["unknown"]) == (1, 1, 1, 0, 0) and pixels.tolist() == [[0]]
    _refused(lambda: dc.occupancy_slice(-1.0, -0.1), "no map cell in the slab")
    dc.close()


def test_a_ray_through_exact_lattice_corners(opt, tmp_path):
    """cell_size 0.2, o = (0.1, 0.1, 0.1), g = (0.5, 0.5, 0.1): x and y cross their planes together, twice; the four cells the segment touches at an
    edge only get nothing."""
    dc, g, o = _store(opt, [np.array([[0.5, 0.5, 0.1]])], origins=np.array([[0.1, 0.1, 0.1]]))
    assert np.array_equal(_bits(g[0, :3]), _bits(f32([0.5, 0.5, 0.1]))) and np.array_equal(_bits(o[0, :3]), _bits(f32([0.1, 0.1, 0.1])))
    assert cm.walk(0.2, o[0, :3], g[0, :3]) == [(0, 0, 0), (1, 1, 0), (2, 2, 0)]
    py, model = _cfg(cell_size=0.2)
    (cells, hits, passes, _), stats = _check(dc, g, o, py, model, tmp_path)
    assert cells.tolist() == [[0, 0, 0], [1, 1, 0], [2, 2, 0]] and hits.tolist() == [0, 0, 1] and passes.tolist() == [1, 1, 0] and stats["cells_traversed"] == 3
    dc.close()


# ---- 4. skipped rays, the largest extent, max_length ------------------------------------------------------------------------------------------------
def test_skipped_rays_contribute_nothing_and_the_largest_extent_is_walked(opt, tmp_path):
    """Voxels of 1 cm, cells of 64.  From the origin (0, 0, 0): twenty rays of a few cells, two whose end cells are exactly 2^11 apart along x
    (walked) and two of 2^11 + 1 (skipped).  From a second origin: a point so close that g == o in float (L2 == 0, skipped) and ten more rays."""
    rng = np.random.default_rng(4)
    c = FINE_CELL
    mid = np.c_[rng.uniform(1.0, 6.0, 20), rng.uniform(-3, 3, 20), rng.uniform(-1, 2, 20)]
    far = np.array([[2048.5 * c, 3.0, 1.0], [2049.5 * c, -3.0, 1.5], [-2047.5 * c, 2.0, 0.55], [-2048.5 * c, 2.0, 0.7]])
    second = np.array([0.5, 2.0, 0.25])
    near = second + np.concatenate([[[2.0**-30, 0.0, 0.0]], np.c_[rng.uniform(0.5, 3.0, 10), rng.uniform(-2, 2, 10), rng.uniform(-1, 1, 10)]])
    dc, g, o = _store(opt, [np.concatenate([mid, far]), near], voxel=FINE_VOXEL, origins=np.array([[0.0, 0.0, 0.0], second]))
    assert g.shape[0] == 35
    paths = [cm.walk(c, o[r, :3], g[r, :3]) for r in range(35)]
    assert [r for r in range(35) if paths[r] is None] == [21, 23, 24] and cm.ray(o[24, :3], g[24, :3])[1] == 0  # (rows 21 and 23: 2^11 + 1 cells; row 24: L2 == 0)
    assert len(paths[20]) >= 2049 and len(paths[22]) >= 2049
    py, model = _cfg(cell_size=c, max_length=5000.0)
    _, stats = _check(dc, g, o, py, model, tmp_path)
    assert stats["rays_skipped"] == 3 and stats["cells_traversed"] > 2 * 2049
    # max_length exactly the length of one ray: that ray is walked; one ulp less: it is skipped, with every longer one
    length = np.array([cm.ray(o[r, :3], g[r, :3])[2] for r in range(35)])
    at = float(length[7])
    py, model = _cfg(cell_size=c, max_length=at)
    _, exact = _check(dc, g, o, py, model, tmp_path, tag="b")
    py, model = _cfg(cell_size=c, max_length=float(np.nextafter(f32(at), f32(0))))
    _, below = _check(dc, g, o, py, model, tmp_path, tag="c")
    assert exact["rays_skipped"] == int((length > f32(at)).sum()) + 1 and below["rays_skipped"] == exact["rays_skipped"] + 1  # (+ 1: the ray of L2 == 0)
    dc.close()


# ---- 5. the edge of the cell range ------------------------------------------------------------------------------------------------------------------
def test_cells_at_the_edge_of_the_range_and_origins_beyond_it(opt, tmp_path):
    """The scene of the carve test: rows in cells up to +-(2^20 - 1), two scans measured from beyond the range.  The cells out of range are counted
    and absent from the listing."""
    rng = np.random.default_rng(9)
    edge = (2**20 - 2) * 0.1
    first = np.array([2**20 - 2 - 59, -(2**20), 2**20 - 100])
    cellsv = rng.choice(60**3, 400, replace=False)
    idx = np.stack([cellsv // 3600, (cellsv // 60) % 60, cellsv % 60], axis=1)
    idx = np.concatenate([idx, [[59, 0, 30], [59, 30, 0], [0, 0, 59]]])
    xyz = (first + idx + 0.5) * 0.1
    origins = np.array([[edge - 8.0, -edge + 8.0, edge - 4.0], [edge + 2.0, -edge - 3.0, edge - 2.0], [edge + 0.75, -edge + 7.0, edge - 5.0]])
    dc, g, o = _store(opt, cv._split(rng, xyz, 3), origins=origins)
    assert g.shape[0] >= 400
    py, model = _cfg(cell_size=VOXEL)
    (cells, _, _, _), stats = _check(dc, g, o, py, model, tmp_path, (EVERYTHING, (edge - 6.0, edge - 5.0)))
    assert stats["cells_out_of_range"] > 0 and stats["rays_skipped"] == 0 and cells[:, 0].max() == 2**20 - 1 and cells[:, 1].min() == -(2**20)
    dc.close()


# ---- 6. growth, determinism --------------------------------------------------------------------------------------------------------------------------
def test_a_table_that_starts_too_small_is_doubled_and_changes_nothing(opt, tmp_path):
    rng = np.random.default_rng(257)
    xyz = ng._one_per_voxel(rng, 257, VOXEL, 8, corner=(2.0, -0.4, -0.3))
    dc, g, o = _store(opt, cv._split(rng, xyz, 4))
    slabs = (EVERYTHING, (0.0, 0.25))
    py, model = _cfg()
    want, auto = _check(dc, g, o, py, model, tmp_path, slabs)
    reference = _products(dc, tmp_path, slabs, "auto")
    assert auto["cells"] > 200
    py, model = _cfg(initial_slots=64)
    _, small = _check(dc, g, o, py, model, tmp_path, slabs, tag="s")
    assert small["table_builds"] > 1 and small["table_slots"] >= 2 * auto["cells"] and {n: small[n] for n in occ.STAT_NAMES} == {n: auto[n] for n in occ.STAT_NAMES}
    grown = _products(dc, tmp_path, slabs, "auto")  # (the same file names: the YAML names its image)
    assert grown == reference
    py, model = _cfg(initial_slots=2**16)
    _, large = _check(dc, g, o, py, model, tmp_path, slabs, tag="l")
    assert large["table_builds"] == 1 and large["table_slots"] == 2**16 and _products(dc, tmp_path, slabs, "auto") == reference
    dc.close()


def test_two_fresh_objects_give_the_same_bytes(opt, tmp_path, wall):
    out = []
    for _ in range(2):
        dc, g, o = _store(opt, wall[0], origins=wall[1])
        stats = dc.build_occupancy()
        out.append((stats, _products(dc, tmp_path, (EVERYTHING, (0.0, 0.5)), "same")))
        dc.close()
    assert out[0] == out[1] and out[0][0]["occupied"] > 0


# ---- 7. the three states ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wall():
    """A wall 6 m in front of two origins, and one stray ray of a third origin off to the side."""
    rng = np.random.default_rng(11)
    scans = [np.c_[6.05 + 0.1 * k + rng.normal(0, 0.01, 600), rng.uniform(-1.0, 1.0, 600), rng.uniform(-0.5, 1.0, 600)] for k in range(2)]
    scans.append(np.array([[-3.0, 8.0, 2.05]]))
    return scans, np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.25], [-3.1, -2.0, 2.1]])


def test_wall_occupied_corridor_free_stray_ray_unknown(opt, tmp_path, wall):
    dc, g, o = _store(opt, wall[0], origins=wall[1])
    n = g.shape[0]
    assert n > 400 and np.array_equal(_bits(o[n - 1, :3]), _bits(f32(wall[1][2])))
    py, model = _cfg()
    z_on_boundary = 0.2
    (cells, hits, passes, state), stats = _check(dc, g, o, py, model, tmp_path, (EVERYTHING, (-0.5, 1.0), (-90.0, -80.0), (z_on_boundary, z_on_boundary)))
    by_cell = {tuple(c): (int(h), int(p), int(s)) for c, h, p, s in zip(cells.tolist(), hits, passes, state)}
    wall_cells = {cm.cell_of(p, 0.2) for p in g[: n - 1, :3]}
    assert all(by_cell[c][2] == occ.OCCUPIED for c in wall_cells)  # every cell a wall point lies in
    corridor = [v for c, v in by_cell.items() if 5 <= c[0] <= 25 and v[0] == 0 and c[1] > -20]
    assert len(corridor) > 50 and sum(1 for v in corridor if v[2] == occ.FREE) > 0.8 * len(corridor)
    stray = cm.walk(0.2, o[n - 1, :3], g[n - 1, :3])
    assert len(stray) > 20 and all(by_cell[c] == (0, 1, occ.UNKNOWN) for c in stray[:-1]) and by_cell[stray[-1]] == (1, 0, occ.OCCUPIED)
    assert occ.slab(z_on_boundary, z_on_boundary, 0.2) == (1, 1)
    _refused(lambda: dc.occupancy_slice(-90.0, -80.0), "no map cell in the slab")
    # with two hits asked for, the stray ray's endpoint is unknown too
    py, model = _cfg(min_hits=2)
    (cells, hits, passes, state), _ = _check(dc, g, o, py, model, tmp_path, tag="b")
    assert {tuple(c): int(s) for c, s in zip(cells.tolist(), state)}[stray[-1]] == occ.UNKNOWN
    dc.close()


# ---- 8. validity ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trail():
    """The scene of the carve test: a wall 6 m in front of three origins and, in the first scan only, a blob half way, which the rays of the other
    two scans pass through."""
    rng = np.random.default_rng(11)
    scans = []
    for k in range(3):
        far = np.c_[6.05 + 0.1 * k + rng.normal(0, 0.01, 700), rng.uniform(-1.5, 1.5, 700), rng.uniform(-1.0, 1.5, 700)]
        scans.append(far if k else np.concatenate([np.c_[3.0 + rng.normal(0, 0.08, 300), rng.uniform(-0.3, 0.3, 300), rng.uniform(-0.2, 0.9, 300)], far]))
    return scans, np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.25], [0.0, -0.5, 0.125]])


def test_building_touches_nothing_and_a_changed_store_makes_the_map_stale(opt, tmp_path, trail):
    from dmsa_lidar_slam_amd.dense_cloud import DenseCarveConfig

    wall = trail
    dc, g, o = _store(opt, wall[0], origins=wall[1])
    path = tmp_path / "m.pcd"
    stale = "no map of the store as it stands"
    calls = (dc.occupancy_cells, dc.occupancy_count, lambda: dc.save_pcd_occupancy(path), lambda: dc.occupancy_slice(*EVERYTHING),
             lambda: dc.save_occupancy_map(tmp_path / "m.pgm", tmp_path / "m.yaml", *EVERYTHING))
    for call in calls:  # nothing built yet
        _refused(call, stale)
    assert not path.exists() and not (tmp_path / "m.pgm").exists()
    normals, without = dc.compute_normals(0.4, 5)
    dc.save_pcd_normals(tmp_path / "n0.pcd")
    carve = DenseCarveConfig()
    c_stats, passes = dc.count_passes(carve, download=True)
    py, model = _cfg()
    _check(dc, g, o, py, model, tmp_path)
    g2, o2 = dc.retained()
    assert np.array_equal(_bits(g2), _bits(g)) and np.array_equal(_bits(o2), _bits(o))
    dc.save_pcd_normals(tmp_path / "n1.pcd")  # (refused if the normals had been invalidated)
    assert open(tmp_path / "n0.pcd", "rb").read() == open(tmp_path / "n1.pcd", "rb").read()
    # a scan added: every call is refused until the map is built again
    far = np.c_[np.full(40, 6.0), np.linspace(3.0, 4.0, 40), np.linspace(0.0, 1.0, 40)]
    dc.add_scan((far - wall[1][2]).astype(f32), np.linspace(base.S[4] + 0.01, base.S[5] - 0.01, 40))
    for call in calls:
        _refused(call, stale)
    g, o = dc.retained()
    c_stats, passes = dc.count_passes(carve, download=True)
    _check(dc, g, o, py, model, tmp_path, tag="b")
    # the carve classification outlived the build: the removal is accepted, and makes the map stale
    assert dc.remove_transients() == c_stats["kept"] < g.shape[0]
    for call in calls:
        _refused(call, stale)
    keep = passes < carve.min_passes
    _check(dc, g[keep], o[keep], py, model, tmp_path, tag="c")
    # a build that M1 refuses changes nothing: the map of the last build is still there
    before = _products(dc, tmp_path, (EVERYTHING,), "kept")
    _refused(lambda: dc.build_occupancy(_cfg(min_hits=0)[0]), "min_hits must lie in [1, 2^20]")
    assert _products(dc, tmp_path, (EVERYTHING,), "kept") == before
    dc.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_every_breach_of_m1_is_refused_with_its_reason(opt, tmp_path):
    from dmsa_lidar_slam_amd.dense_cloud import DenseOccupancyConfig as Cfg

    rng = np.random.default_rng(44)
    xyz = ng._one_per_voxel(rng, 100, VOXEL, 8, corner=(1.0, 0.0, 0.0))
    off, _ = ng._creator(opt, retain=False, still=True, voxel_size=VOXEL)
    off.add_scan(xyz, ng._stamps(100))
    _refused(off.build_occupancy, "retention is off")
    _refused(off.occupancy_cells, "no map of the store")
    off.close()
    empty, _ = ng._creator(opt, still=True, voxel_size=VOXEL)
    _refused(empty.build_occupancy, "no retained point")
    empty.close()
    no_voxel, _ = ng._creator(opt, still=True, voxel_size=0.0)
    no_voxel.add_scan(xyz, ng._stamps(100))
    _refused(no_voxel.build_occupancy, "voxel_size must be > 0")
    no_voxel.close()
    dc, _ = ng._still_cloud(opt, xyz, VOXEL)
    call = dc.build_occupancy
    _refused(lambda: call(Cfg(cell_size=np.inf)), "cell_size is not finite")
    _refused(lambda: call(Cfg(cell_size=np.nan)), "cell_size is not finite")
    _refused(lambda: call(Cfg(cell_size=float(np.nextafter(f32(VOXEL), f32(0))))), "[voxel_size, 64 * voxel_size]")
    _refused(lambda: call(Cfg(cell_size=float(np.nextafter(f32(64.0) * f32(VOXEL), f32(10))))), "[voxel_size, 64 * voxel_size]")
    _refused(lambda: call(Cfg(max_length=np.inf)), "max_length must be finite")
    _refused(lambda: call(Cfg(max_length=np.nan)), "max_length must be finite")
    _refused(lambda: call(Cfg(max_length=0.0)), "max_length must be > 0")
    for name in ("min_hits", "min_passes", "occ_num", "occ_den"):
        for bad in (0, -1, 2**20 + 1):
            _refused(lambda: call(Cfg(**{name: bad})), f"{name} must lie in [1, 2^20]")
    for bad in (1, 32, 96, 2**32, -64):
        _refused(lambda: call(Cfg(initial_slots=bad)), "initial_slots must be 0 or a power of two in [64, 2^31]")
    _refused(dc.occupancy_cells, "no map of the store")  # a refused call is no map
    # the bounds themselves are legal
    s = call(Cfg(cell_size=VOXEL, min_hits=2**20, min_passes=2**20, occ_num=2**20, occ_den=2**20, initial_slots=64))
    assert s["rows"] == 100 and s["occupied"] == 0 and s["free"] == 0 and s["unknown"] == s["cells"] > 0
    assert call(Cfg(cell_size=float(f32(64.0) * f32(VOXEL))))["cells"] >= 1
    _refused(lambda: dc.save_pcd_occupancy(tmp_path / "x.pcd", 3), "min_state must lie in [0, 2]")
    _refused(lambda: dc.save_pcd_occupancy(tmp_path / "x.pcd", -1), "min_state must lie in [0, 2]")
    _refused(lambda: dc.occupancy_slice(np.nan, 1.0), "must be finite")
    _refused(lambda: dc.occupancy_slice(0.0, np.inf), "must be finite")
    _refused(lambda: dc.occupancy_slice(1.0, 0.5), "z_lo must be <= z_hi")
    _refused(lambda: dc.save_pcd_occupancy(tmp_path / "no" / "such" / "dir.pcd"), "dense occupancy")
    assert not (tmp_path / "x.pcd").exists()
    dc.close()


# ---- 10. the demo ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_demo_writes_the_voxel_file_and_the_map(tmp_path):
    """Carve, then the map of what carving left: the three files are there, their headers parse, and the voxel file's rows are the model's on the
    store the demo leaves (its rays, written beside the files)."""
    out = {n: tmp_path / n for n in ("Dense.pcd", "Carved.pcd", "Occupancy.pcd", "map.pgm", "rays.npz")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dense_cloud_demo.py"), "--scans", "6", "--voxel", "0.4", "--carve", "0.4", "--occupancy", "0.4",
                        "--occupancy-slice", "0.2", "1.5", "--out", str(out["Dense.pcd"]), "--carved-out", str(out["Carved.pcd"]), "--occupancy-out", str(out["Occupancy.pcd"]),
                        "--map-out", str(out["map.pgm"]), "--occupancy-rays-out", str(out["rays.npz"])], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert [i for i, l in enumerate(lines) if l.startswith("carve (")][0] < [i for i, l in enumerate(lines) if l.startswith("occupancy (cell 0.4 m)")][0]
    rays = np.load(out["rays.npz"])
    g, o = rays["xyz"], rays["origin"]
    model = occ.Config(cell_size=0.4)
    want, stats = occ.build(g, o, model)
    assert stats["cells"] > 500 and stats["occupied"] > 0 and stats["free"] > 0
    raw = open(out["Occupancy.pcd"], "rb").read()
    assert raw == occ.pcd_bytes(want, model, 0) and f"cells {stats['cells']}  occupied {stats['occupied']}  free {stats['free']}  unknown {stats['unknown']}" in p.stdout
    ref = occ.slice_of(want, model, 0.2, 1.5)
    assert open(out["map.pgm"], "rb").read() == occ.pgm_bytes(ref[1])
    assert open(tmp_path / "map.yaml").read() == occ.yaml_text("map.pgm", 0.4, ref[0]["cx_min"], ref[0]["cy_min"])
    assert f"{ref[0]['width']} x {ref[0]['height']} pixels" in p.stdout
