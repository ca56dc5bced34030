"""CPU-side checks of include/dmsa_dense_surface.h: the symbols, structs and defaults; dmsa_dense_surface_samples (S2-S4 through the header the
device kernels compile) against the model (tests/dense_surface_model.py, the yardstick of the GPU tests) on every kind of ray; the two header
texts; the refusals that need no device; and, on the model alone, the mesh of a sphere seen from its centre (closed, of genus 0, facing the
sensor, its volume within the bound one cell gives) and the mesh of a linear field (a plane where the field says, facing +x)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from dmsa_lidar_slam_amd import _capi as capi
from dmsa_lidar_slam_amd import dense_cloud as dcl

import dense_carve_model as cm
import dense_surface_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
f64 = np.float64


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def _as_c(cfg):
    return dcl.DenseSurfaceConfig(cfg.cell_size, cfg.truncation, cfg.max_length, cfg.min_weight, cfg.initial_slots)


def _same(cfg, o, g):
    """The C call and the model agree on the ray o -> g; returns the model's answer."""
    o, g = np.asarray(o, f32), np.asarray(g, f32)
    want, got = sm.samples(o, g, cfg), dcl.surface_samples(_as_c(cfg), o, g)
    if want is None:
        assert got is None, (o, g)
        return None
    assert got is not None, (o, g)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (o, g, got, want)
    return want


# ---- exports, layouts, defaults --------------------------------------------------------------------------------------------------------------
def test_symbol_tuple_equals_the_header_and_the_library_exports_it(lib):
    header = open(os.path.join(ROOT, "include", "dmsa_dense_surface.h")).read()
    declared = set(re.findall(r"\b(dmsa_[a-z_0-9]+)\s*\(", header))
    assert declared == set(capi.DENSE_SURFACE_SYMBOLS) and len(capi.DENSE_SURFACE_SYMBOLS) == len(declared) == 11
    others = (set(capi.EXPORTED_SYMBOLS) | set(capi.DENSE_CLOUD_SYMBOLS) | set(capi.DENSE_NORMALS_SYMBOLS) | set(capi.DENSE_OUTLIERS_SYMBOLS) | set(capi.DENSE_CARVE_SYMBOLS) |
              set(capi.DENSE_INTENSITY_SYMBOLS) | set(capi.DENSE_CLUSTERS_SYMBOLS) | set(capi.DENSE_COMPARE_SYMBOLS) | set(capi.DENSE_ALIGN_SYMBOLS) |
              set(capi.DENSE_ALIGN_PLANE_SYMBOLS) | set(capi.DENSE_OCCUPANCY_SYMBOLS))
    assert not declared & others
    for name in declared:
        assert hasattr(lib, name), name
    for rule in ("S1", "S2", "S3", "S4", "S5", "S6", "S7", "S8", "S9", "S10"):
        assert re.search(rf"\b{rule}\b", header)


def test_struct_layouts_and_defaults(lib):
    names = ("cell_size", "truncation", "max_length", "min_weight", "initial_slots")
    assert C.sizeof(capi.DenseSurfaceConfig) == 24 and [getattr(capi.DenseSurfaceConfig, n).offset for n in names] == [0, 4, 8, 12, 16]
    assert C.sizeof(capi.DenseSurfaceStats) == 72 and dcl.SURFACE_STAT_NAMES == sm.STAT_NAMES + ("table_slots", "table_builds")
    assert C.sizeof(capi.DenseMeshStats) == 24 and dcl.MESH_STAT_NAMES == sm.MESH_STAT_NAMES
    c = capi.DenseSurfaceConfig()
    C.memset(C.byref(c), 0x5A, C.sizeof(c))
    lib.dmsa_default_dense_surface_config(C.byref(c))
    want = [float(f32(0.2)), float(f32(0.6)), 30.0, 2, 0]
    assert [getattr(c, n) for n in names] == want
    lib.dmsa_default_dense_surface_config(None)
    py, model = dcl.DenseSurfaceConfig().to_c(), sm.Config()
    assert [getattr(py, n) for n in names] == want
    assert [float(f32(model.cell_size)), float(f32(model.truncation)), float(f32(model.max_length)), model.min_weight, model.initial_slots] == want


# ---- S2-S4 ------------------------------------------------------------------------------------------------------------------------------------
def test_samples_of_random_rays_equal_the_model():
    rng = np.random.default_rng(5)
    seen = set()
    for cfg in (sm.Config(max_length=100.0), sm.Config(cell_size=0.1, truncation=0.1, max_length=100.0), sm.Config(cell_size=0.05, truncation=0.8, max_length=100.0),
                sm.Config(cell_size=0.37, truncation=1.0, max_length=100.0)):
        for _ in range(150):
            o = rng.uniform(-3, 3, 3)
            g = o + rng.normal(0, 1, 3) * rng.choice([0.05, 0.7, 4.0, 12.0])
            got = _same(cfg, o, g)
            assert got is not None and got[0].shape[0] >= 1 and got[3] == 0
            seen.update(got[1].tolist())
            assert got[1].min() >= -32768 and got[1].max() <= 32768
    assert min(seen) < -30000 and max(seen) > 30000 and any(abs(v) < 2000 for v in seen)  # both clamps' neighbourhood and the surface itself


def test_samples_of_axis_parallel_rays_equal_the_model():
    cfg = sm.Config()
    for axis in range(3):
        for sign in (1.0, -1.0):
            for length in (0.35, 1.0, 5.0):
                o = np.array([0.13, -0.21, 0.07])
                g = o.copy()
                g[axis] += sign * length
                cells, q, traversed, _ = _same(cfg, o, g)
                assert traversed == cells.shape[0] and len({tuple(np.delete(c, axis)) for c in cells.tolist()}) == 1  # one column of cells
                assert np.all(np.diff(q) < 0)  # from in front of the surface to behind it
    # the endpoint at a cell centre: q is exactly 0 there, and +-2^15 * (k * cell / truncation) rounded k cells away
    o, g = f32([0.1, 0.1, 0.1]), f32([2.1, 0.1, 0.1])
    cells, q, _, _ = _same(sm.Config(cell_size=0.2, truncation=0.6), o, g)
    at = {tuple(c): int(v) for c, v in zip(cells.tolist(), q)}
    assert at[cm.cell_of(g, 0.2)] in (-1, 0, 1) and at[(7, 0, 0)] > 30000 and at[(13, 0, 0)] < -30000


def test_the_corner_ray_and_a_ray_shorter_than_the_truncation():
    """The corner ray of the occupancy tests is shorter than the truncation: its segment starts at the origin itself and ends one truncation
    behind the endpoint, and x and y still step together."""
    cfg = sm.Config(cell_size=0.2, truncation=0.6)
    o, g = f32([0.1, 0.1, 0.1]), f32([0.5, 0.5, 0.1])
    a, b, d, length = sm.segment(o, g, cfg)
    assert length < f32(0.6) and np.array_equal(np.array(a, f32), o) and b[0] > g[0] and b[0] == b[1] and b[2] == g[2]
    cells, q, traversed, outside = _same(cfg, o, g)
    assert cells[0].tolist() == [0, 0, 0] and all(c[0] == c[1] and c[2] == 0 for c in cells.tolist()) and traversed == cells.shape[0] >= 4 and outside == 0
    # a ray whose length is exactly the truncation starts at the origin too (L > truncation is false); one ulp longer does not
    o, g = f32([0.0, 0.0, 0.0]), f32([0.6, 0.0, 0.0])
    assert cm.ray(o, g)[2] == f32(0.6)
    assert np.array_equal(np.array(sm.segment(o, g, cfg)[0], f32), o)
    _same(cfg, o, g)
    g2 = f32([np.nextafter(f32(0.6), f32(1)), 0.0, 0.0])
    assert sm.segment(o, g2, cfg)[0][0] != 0
    _same(cfg, o, g2)


def test_skipped_rays_of_all_three_kinds():
    cfg = sm.Config(cell_size=0.64, truncation=0.64 * 16, max_length=5000.0)
    assert _same(cfg, [1.0, 2.0, 3.0], [1.0, 2.0, 3.0]) is None  # L2 == 0
    assert _same(sm.Config(max_length=2.0), [0, 0, 0], [0, 2.0, 0.1]) is None  # L > max_length
    assert _same(sm.Config(max_length=2.0), [0, 0, 0], [0, 2.0, 0.0]) is not None  # L == max_length
    # T2's third case on the segment: the ends of a -> b lie 2 * 16 cells apart at most, so only cells beyond 2^31 refuse it
    far = f32(2.0**31 * 0.64)  # (floats are 128 apart out there)
    assert sm.samples([far - 1024, 0, 0], [far + 1024, 0, 0], cfg) is None and sm.segment([far - 1024, 0, 0], [far + 1024, 0, 0], cfg) is not None
    assert _same(cfg, [far - 1024, 0, 0], [far + 1024, 0, 0]) is None
    # ... while the ray itself may be longer than 2^11 cells: only its last two truncations are walked
    got = _same(cfg, [0, 0, 0], [2100 * 0.64, 1.0, 0.5])
    assert got is not None and cm.walk(0.64, f32([0, 0, 0]), f32([2100 * 0.64, 1.0, 0.5])) is None and got[0].shape[0] >= 32


def test_cells_at_the_edge_of_the_range():
    cfg = sm.Config(cell_size=0.2, truncation=0.6)
    edge = (2**20) * float(f32(0.2))
    o, g = [edge - 3.0, 0.05, 0.05], [edge - 0.1, 0.05, 0.05]  # ends in the last cell; the segment goes on beyond the range
    cells, q, traversed, outside = _same(cfg, o, g)
    assert cells[:, 0].max() == 2**20 - 1 and outside >= 2 and traversed == cells.shape[0] + outside
    o, g = [-edge + 3.0, 0.05, 0.05], [-edge + 0.1, 0.05, 0.05]
    cells, q, traversed, outside = _same(cfg, o, g)
    assert cells[:, 0].min() == -(2**20) and outside >= 2
    # all of the segment outside: no sample, but no skip either
    cells, q, traversed, outside = _same(cfg, [edge + 3.0, 0, 0], [edge + 6.0, 0, 0])
    assert cells.shape[0] == 0 and traversed == outside > 0


# ---- S7, S9: the texts ---------------------------------------------------------------------------------------------------------------------------
def test_texts_equal_the_c_calls(lib):
    for n in (0, 1, 123456, 10**12 - 1):
        assert dcl.pcdHeaderTsdfBinary(n) == sm.pcd_header(n)
    assert "FIELDS x y z tsdf weight\nSIZE 4 4 4 4 4\nTYPE F F F F U\n" in dcl.pcdHeaderTsdfBinary(7) and sm.ROW.itemsize == 20
    for v, t in ((0, 0), (3, 1), (123456, 654321), (2**31 - 1, 2**31 - 1)):
        assert dcl.plyHeaderMesh(v, t) == sm.ply_header(v, t)
    assert dcl.plyHeaderMesh(3, 1).splitlines() == ["ply", "format binary_little_endian 1.0", "element vertex 3", "property float x", "property float y", "property float z",
                                                    "element face 1", "property list uchar int vertex_indices", "end_header"]
    raw = sm.ply_bytes(np.zeros((3, 3), f32), np.array([[0, 1, 2]], np.int32))
    assert len(raw) == len(sm.ply_header(3, 1)) + 36 + 13 and raw[-13:] == b"\x03" + np.array([0, 1, 2], "<i4").tobytes()
    assert sm.tsdf(-32768 * 5, 5, 0.6) == -f32(0.6) and sm.tsdf(0, 3, 0.6) == 0 and sm.tsdf(16384, 1, 0.5) == f32(0.25)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_that_needs_no_device(lib):
    from dmsa_lidar_slam_amd.api import DmsaError

    o, g = f32([0, 0, 0]), f32([1, 0.5, 0.25])
    bad = (dict(cell_size=np.nan), dict(cell_size=np.inf), dict(cell_size=0.0), dict(cell_size=-0.2), dict(truncation=np.nan), dict(truncation=np.inf),
           dict(truncation=float(np.nextafter(f32(0.2), f32(0)))), dict(truncation=float(np.nextafter(f32(16.0) * f32(0.2), f32(10)))), dict(max_length=np.nan),
           dict(max_length=np.inf), dict(max_length=0.0), dict(max_length=-1.0), dict(min_weight=0), dict(min_weight=-1), dict(min_weight=2**20 + 1), dict(initial_slots=1),
           dict(initial_slots=32), dict(initial_slots=96), dict(initial_slots=2**32), dict(initial_slots=-64))
    for kw in bad:
        assert sm.Config(**kw).refused(), kw
        with pytest.raises(DmsaError):
            dcl.surface_samples(dcl.DenseSurfaceConfig(**kw), o, g)
    for kw in (dict(truncation=0.2), dict(truncation=float(f32(16.0) * f32(0.2))), dict(min_weight=1), dict(min_weight=2**20), dict(initial_slots=64), dict(initial_slots=2**31)):
        assert not sm.Config(**kw).refused(), kw  # the bounds themselves are legal
        assert dcl.surface_samples(dcl.DenseSurfaceConfig(**kw), o, g) is not None
    cfg = dcl.DenseSurfaceConfig().to_c()
    po, pg = capi.ptr(o, C.c_float), capi.ptr(g, C.c_float)
    n = C.c_int64(0)
    cells, q = np.zeros((4, 3), np.int32), np.zeros(4, np.int32)
    assert lib.dmsa_dense_surface_samples(None, po, pg, None, None, 0, C.byref(n)) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_surface_samples(C.byref(cfg), None, pg, None, None, 0, C.byref(n)) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_surface_samples(C.byref(cfg), po, None, None, None, 0, C.byref(n)) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_surface_samples(C.byref(cfg), po, pg, None, None, 0, None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_surface_samples(C.byref(cfg), po, pg, None, None, -1, C.byref(n)) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_surface_samples(C.byref(cfg), po, pg, None, capi.ptr(q, C.c_int32), 4, C.byref(n)) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_surface_samples(C.byref(cfg), po, pg, capi.ptr(cells, C.c_int32), None, 4, C.byref(n)) == capi.DMSA_ERR_INVALID
    # a buffer shorter than the samples: filled to its end, the count is the whole
    assert lib.dmsa_dense_surface_samples(C.byref(cfg), po, pg, capi.ptr(cells, C.c_int32), capi.ptr(q, C.c_int32), 4, C.byref(n)) == capi.DMSA_OK
    want = sm.samples(o, g, sm.Config())
    assert n.value == want[0].shape[0] > 4 and np.array_equal(cells, want[0][:4]) and np.array_equal(q, want[1][:4])
    buf = C.create_string_buffer(512)
    assert lib.dmsa_pcd_header_tsdf_binary(-1, buf, 512) == capi.DMSA_ERR_INVALID and lib.dmsa_pcd_header_tsdf_binary(10**12, buf, 512) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_pcd_header_tsdf_binary(5, None, 512) == capi.DMSA_ERR_INVALID and lib.dmsa_pcd_header_tsdf_binary(5, buf, 40) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_ply_header_mesh(-1, 0, buf, 512) == capi.DMSA_ERR_INVALID and lib.dmsa_ply_header_mesh(0, -1, buf, 512) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_ply_header_mesh(2**31, 0, buf, 512) == capi.DMSA_ERR_INVALID and lib.dmsa_ply_header_mesh(0, 2**31, buf, 512) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_ply_header_mesh(1, 1, None, 512) == capi.DMSA_ERR_INVALID and lib.dmsa_ply_header_mesh(1, 1, buf, 40) == capi.DMSA_ERR_INVALID
    # the device calls refuse a null object before they touch anything
    assert lib.dmsa_dense_cloud_build_surface(None, C.byref(cfg), None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_surface_cells(None, 0, 0, None, None, None, None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_save_pcd_tsdf(None, b"/dev/null", None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_extract_mesh(None, 2, None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_mesh_vertices(None, 0, 0, None, None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_mesh_triangles(None, 0, 0, None, None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_save_ply_mesh(None, b"/dev/null") == capi.DMSA_ERR_INVALID


# ---- S8 on the model alone ------------------------------------------------------------------------------------------------------------------------
def test_the_orientation_table_covers_every_case_and_opposite_cases_mirror():
    assert len(sm.ORIENTATION) == 6 * 14
    for (t, inside), flips in sm.ORIENTATION.items():
        outside = tuple(p for p in range(4) if p not in inside)
        assert len(flips) == (2 if len(inside) == 2 else 1)
        if len(inside) != 2:  # one corner against three: the same triangle seen from the other side
            assert sm.case_triangles(inside) == sm.case_triangles(outside) and sm.ORIENTATION[(t, outside)] == [not f for f in flips]
    assert [sm.chain_of(t) for t in range(6)] == [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]


def fibonacci_sphere(n, radius):
    """n quasi-uniform directions times radius, float32."""
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * math.pi * (3.0 - math.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return (radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)).astype(f32)


def check_sphere_mesh(xyz, faces, radius, cell, sensor):
    """What the mesh of a sphere seen from inside has to satisfy: closed, genus 0, facing the sensor, the volume within one cell's bound."""
    assert faces.shape[0] > 1000 and faces.min() == 0 and faces.max() == xyz.shape[0] - 1
    assert sm.closed_manifold(faces)  # every directed edge exactly once, its reverse exactly once
    assert sm.euler_characteristic(xyz.shape[0], faces) == 2
    volume = sm.volume_towards(xyz, faces, sensor)
    assert volume > 0
    assert 4.0 / 3.0 * math.pi * (radius - cell) ** 3 <= volume <= 4.0 / 3.0 * math.pi * (radius + cell) ** 3, volume
    return volume


def test_a_sphere_seen_from_its_centre_is_closed_faces_the_sensor_and_has_its_volume():
    """Radius 2 m, 20 000 Fibonacci directions, cell 0.2, truncation 0.6, min_weight 1.  The normals point to the sensor, which stands inside:
    the enclosed volume is taken on that side (dense_surface_model.volume_towards), so it is positive exactly when the orientation is S8's."""
    g = fibonacci_sphere(20000, 2.0)
    centre = f32([0.03, -0.02, 0.05])  # (off the lattice, so that no ray runs along cell planes)
    g = g + centre
    o = np.tile(centre, (g.shape[0], 1))
    cfg = sm.Config(cell_size=0.2, truncation=0.6, min_weight=1)
    lst, stats = sm.build(g, o, cfg)
    assert stats["rays_skipped"] == 0 and stats["cells"] == stats["cells_valid"] > 5000
    xyz, faces, mstats = sm.mesh(lst, cfg, 1)
    assert mstats["vertices"] == xyz.shape[0] and mstats["triangles"] == faces.shape[0] and mstats["tetrahedra_meshed"] > faces.shape[0] / 2
    check_sphere_mesh(xyz, faces, 2.0, 0.2, centre)
    radius = np.linalg.norm(xyz.astype(f64) - centre, axis=1)
    assert abs(radius.mean() - 2.0) < 0.02 and radius.min() > 1.8 and radius.max() < 2.2  # the surface lies within one cell of the sphere


def test_a_linear_field_gives_the_plane_where_it_says_facing_plus_x():
    """sum = round(k * (x - x0)) at the nodes of a block, n = 1: inside (sum < 0) is x < x0, so the outside, where the sensor stood, is +x.  The
    interpolation is exact for a linear field up to the rounding of the sums: every vertex has x == x0 to float rounding of the field, and every
    normal points to +x."""
    cell, x0, k = 0.2, 0.5234, 40000.0
    cfg = sm.Config(cell_size=cell, truncation=0.6, min_weight=1)
    cells = np.array([(x, y, z) for x in range(-2, 8) for y in range(-3, 4) for z in range(0, 5)], np.int32)
    cx = np.array([float(sm.centre(c, cell)) for c in cells[:, 0]])
    total = np.rint(k * (cx - x0)).astype(np.int64)
    assert (total < 0).any() and (total > 0).any() and not (total == 0).any()
    order = np.argsort([sm.key_of(tuple(c)) for c in cells.tolist()])
    lst = (cells[order], total[order], np.ones(cells.shape[0], np.uint32))
    xyz, faces, stats = sm.mesh(lst, cfg, 1)
    assert stats["triangles"] == faces.shape[0] >= 2 * 6 * 4 and stats["tetrahedra_meshed"] == 9 * 6 * 4 * 6
    # rounding a sum moves m by at most 0.5, the crossing by at most 0.5 / k metres on either node: 1 / k in all, plus float32's own rounding
    assert np.abs(xyz[:, 0].astype(f64) - x0).max() <= 1.0 / k + 2.0**-24
    v = xyz.astype(f64)
    normal = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    assert (normal[:, 0] > 0).all() and (normal[:, 0] > 10 * np.abs(normal[:, 1:]).max(axis=1)).all()
    # the plane is tiled exactly once: the triangles' areas add up to the block's cross-section between the outermost node centres
    assert abs(0.5 * np.linalg.norm(normal, axis=1).sum() - (6 * cell) * (4 * cell)) < 1e-4
    # sum == 0 is outside: a node exactly on the plane gives vertices AT that node (t = 1 from below, t = 0 never: the node is no lower inside end)
    total2 = total.copy()
    total2[cells[:, 0] == 3] = 0
    lst2 = (cells[order], total2[order], np.ones(cells.shape[0], np.uint32))
    xyz2, faces2, _ = sm.mesh(lst2, cfg, 1)
    assert faces2.shape[0] > 0 and np.array_equal(np.unique(xyz2[:, 0]), [sm.centre(3, cell)])
