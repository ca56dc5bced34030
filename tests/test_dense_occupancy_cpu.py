"""CPU-side checks of include/dmsa_dense_occupancy.h: the symbols, structs and defaults, M5 on the host against the model
(tests/dense_occupancy_model.py, the yardstick of the GPU tests) around every boundary, the model's accumulation against a brute-force twin that
rasterises every ray with exact rationals, the model's projection against a loop over columns, the texts of M6 and M7 against the C calls, and
the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dmsa_lidar_slam_amd import _capi as capi
from dmsa_lidar_slam_amd import dense_cloud as dcl

import dense_carve_model as cm
import dense_occupancy_model as occ
import test_dense_carve_cpu as exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def _as_c(cfg):
    return dcl.DenseOccupancyConfig(cfg.cell_size, cfg.max_length, cfg.min_hits, cfg.min_passes, cfg.occ_num, cfg.occ_den, cfg.initial_slots)


# ---- exports, layouts, defaults --------------------------------------------------------------------------------------------------------------
def test_symbol_tuple_equals_the_header_and_the_library_exports_it(lib):
    header = open(os.path.join(ROOT, "include", "dmsa_dense_occupancy.h")).read()
    declared = set(re.findall(r"\b(dmsa_[a-z_0-9]+)\s*\(", header))
    assert declared == set(capi.DENSE_OCCUPANCY_SYMBOLS) and len(capi.DENSE_OCCUPANCY_SYMBOLS) == len(declared) == 10
    others = (set(capi.EXPORTED_SYMBOLS) | set(capi.DENSE_CLOUD_SYMBOLS) | set(capi.DENSE_NORMALS_SYMBOLS) | set(capi.DENSE_OUTLIERS_SYMBOLS) | set(capi.DENSE_CARVE_SYMBOLS) |
              set(capi.DENSE_INTENSITY_SYMBOLS) | set(capi.DENSE_CLUSTERS_SYMBOLS) | set(capi.DENSE_COMPARE_SYMBOLS) | set(capi.DENSE_ALIGN_SYMBOLS) |
              set(capi.DENSE_ALIGN_PLANE_SYMBOLS))
    assert not declared & others
    for name in declared:
        assert hasattr(lib, name), name
    for rule in ("M1", "M2", "M3", "M4", "M5", "M6", "M7", "M8"):
        assert re.search(rf"\b{rule}\b", header)


def test_struct_layouts_and_defaults(lib):
    names = ("cell_size", "max_length", "min_hits", "min_passes", "occ_num", "occ_den", "initial_slots")
    assert C.sizeof(capi.DenseOccupancyConfig) == 32 and [getattr(capi.DenseOccupancyConfig, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24]
    assert C.sizeof(capi.DenseOccupancyStats) == 88 and dcl.OCCUPANCY_STAT_NAMES == occ.STAT_NAMES + ("table_slots", "table_builds")
    info = ("width", "height", "cx_min", "cy_min", "origin_x", "origin_y", "occupied", "free", "unknown")
    assert C.sizeof(capi.DenseOccupancySliceInfo) == 56 and [getattr(capi.DenseOccupancySliceInfo, n).offset for n in info] == [0, 4, 8, 12, 16, 24, 32, 40, 48]
    assert dcl.OCCUPANCY_SLICE_NAMES == info
    c = capi.DenseOccupancyConfig()
    C.memset(C.byref(c), 0x5A, C.sizeof(c))
    lib.dmsa_default_dense_occupancy_config(C.byref(c))
    want = [float(f32(0.2)), 30.0, 1, 2, 16, 1, 0]
    assert [getattr(c, n) for n in names] == want
    lib.dmsa_default_dense_occupancy_config(None)
    py, model = dcl.DenseOccupancyConfig().to_c(), occ.Config()
    assert [getattr(py, n) for n in names] == want
    assert [float(f32(model.cell_size)), float(f32(model.max_length)), model.min_hits, model.min_passes, model.occ_num, model.occ_den, model.initial_slots] == want
    assert (dcl.OCCUPANCY_UNKNOWN, dcl.OCCUPANCY_FREE, dcl.OCCUPANCY_OCCUPIED) == (occ.UNKNOWN, occ.FREE, occ.OCCUPIED) == (0, 1, 2)


# ---- M5 -------------------------------------------------------------------------------------------------------------------------------------
def _around(cfg):
    """(hits, passes) around every boundary of M5 for cfg."""
    hits = {0, 1, cfg.min_hits - 1, cfg.min_hits, cfg.min_hits + 1, 2 * cfg.min_hits, 2**26}
    hits = sorted(h for h in hits if 0 <= h <= 2**26)
    pairs = set()
    for h in hits:
        edge = h * cfg.occ_num // cfg.occ_den  # the largest passes with passes * den <= hits * num
        for p in (0, 1, cfg.min_passes - 1, cfg.min_passes, cfg.min_passes + 1, edge - 1, edge, edge + 1, 2**26):
            if 0 <= p <= 2**26:
                pairs.add((h, p))
    return sorted(pairs)


def test_state_equals_the_model_around_every_boundary():
    configs = [occ.Config(), occ.Config(occ_num=32), occ.Config(min_hits=3, min_passes=5, occ_num=7, occ_den=3), occ.Config(min_hits=2, min_passes=1, occ_num=1, occ_den=1),
               occ.Config(occ_num=1, occ_den=16), occ.Config(min_hits=2**20, min_passes=2**20, occ_num=2**20, occ_den=2**20),
               occ.Config(min_hits=2**20, min_passes=2**20, occ_num=2**20, occ_den=2**20 - 1), occ.Config(occ_num=2**20, occ_den=1), occ.Config(occ_num=1, occ_den=2**20)]
    seen = set()
    for cfg in configs:
        py = _as_c(cfg)
        for h, p in _around(cfg):
            want = occ.state(cfg, h, p)
            assert dcl.occupancy_state(py, h, p) == want, (cfg, h, p)
            seen.add(want)
    assert seen == {0, 1, 2}
    # each comparison at equality and one to either side, by hand
    d = occ.Config()
    assert [occ.state(d, 1, p) for p in (15, 16, 17)] == [2, 2, 1] and [occ.state(d, 0, p) for p in (0, 1, 2)] == [0, 0, 1] and occ.state(d, 1, 0) == 2
    t = occ.Config(min_hits=3, min_passes=5, occ_num=7, occ_den=3)
    assert [occ.state(t, 2, 0), occ.state(t, 3, 7), occ.state(t, 3, 8), occ.state(t, 2, 4), occ.state(t, 2, 5)] == [0, 2, 1, 0, 1]  # 3 * 7 = 21 = 7 * 3; 24 > 21
    # the products need 64 bits: 2^26 * 2^20 on either side
    big = occ.Config(occ_num=2**20, occ_den=2**20)
    assert dcl.occupancy_state(_as_c(big), 2**26, 2**26) == 2 and dcl.occupancy_state(_as_c(big), 2**26 - 1, 2**26) == 1
    # (a product taken modulo 2^32 would be 0 on both sides: occupied)
    assert occ.state(big, 2**26 - 1, 2**26) == 1


# ---- M2-M3: the model's accumulation against exact geometry ------------------------------------------------------------------------------------
def _short_rays():
    rng = np.random.default_rng(17)
    o = np.tile(np.array([[0.11, -0.07, 0.13], [0.52, 0.31, -0.22]]), (24, 1))[:45]
    g = o + rng.uniform(-1, 1, (45, 3)) * rng.choice([0.15, 0.6, 1.3], (45, 1))
    g[:6] = o[:6] + np.array([0.02, 0.01, -0.015])  # inside the origin's cell
    g[6:12] = np.array([0.7, 0.5, 0.3])  # several rays into one cell, from both origins
    o, g = o.astype(f32), g.astype(f32)
    # the ray through exact lattice corners (cells of 0.2: X from 1025 to 5119 on x and y alike)
    return np.concatenate([o, f32([[0.1, 0.1, 0.1]])]), np.concatenate([g, f32([[0.5, 0.5, 0.1]])])


def test_model_accumulation_equals_the_brute_force_twin():
    o, g = _short_rays()
    cfg = occ.Config(cell_size=0.2)
    counts, stats = occ.accumulate(g, o, cfg)
    twin = {}
    for r in range(g.shape[0]):
        end = cm.cell_of(g[r], 0.2)
        cells = exact._exact_cells(0.2, o[r], g[r])
        assert end in cells and cm.cell_of(o[r], 0.2) in cells
        for cell in cells:
            twin.setdefault(cell, [0, 0])[0 if cell == end else 1] += 1
    assert counts == twin and stats["rays_walked"] == g.shape[0] and stats["cells_traversed"] == sum(h + p for h, p in twin.values())
    assert sum(h for h, _ in counts.values()) == g.shape[0] and stats["cells_out_of_range"] == 0
    assert counts[cm.cell_of(g[0], 0.2)][0] >= 1 and max(h for h, _ in counts.values()) >= 6 and any(h > 0 and p > 0 for h, p in counts.values())
    # the corner ray: both axes step at once; the cells its segment touches at an edge only get nothing
    # (float32(0.5) / float32(0.2) lies just below 2.5, so the end is X = 5119, not 5121: x and y still run side by side, through 2048 and 4096)
    assert exact._fixed(0.1, 0.2) == 1025 and exact._fixed(0.5, 0.2) == 5119
    assert cm.walk(0.2, o[-1], g[-1]) == [(0, 0, 0), (1, 1, 0), (2, 2, 0)]
    # a skipped ray contributes nothing, a cell out of range is counted and not recorded
    more_o, more_g = np.concatenate([o, o[:1], f32([[(2**20 - 1.5) * 0.2, 0, 0]])]), np.concatenate([g, o[:1], f32([[(2**20 + 1.5) * 0.2, 0, 0]])])
    counts2, stats2 = occ.accumulate(more_g, more_o, cfg)
    assert stats2["rays_skipped"] == 1 and stats2["cells_out_of_range"] == 2 and stats2["cells_traversed"] == stats["cells_traversed"] + 4
    assert {c: v for c, v in counts2.items() if c[0] < 2**19} == counts and counts2[(2**20 - 2, 0, 0)] == [0, 1] and counts2[(2**20 - 1, 0, 0)] == [0, 1]
    # the listing is in ascending key order and complete
    cells, hits, passes, states = occ.listing(counts, cfg)
    keys = [occ.key_of(tuple(c)) for c in cells.tolist()]
    assert keys == sorted(keys) and len(set(keys)) == len(counts) and [counts[tuple(c)] for c in cells.tolist()] == np.stack([hits, passes], 1).tolist()
    assert states.tolist() == [occ.state(cfg, h, p) for h, p in zip(hits, passes)]


# ---- M7: the projection against a loop over columns ----------------------------------------------------------------------------------------------
def test_projection_equals_a_loop_over_columns():
    o, g = _short_rays()
    cfg = occ.Config(cell_size=0.2, min_passes=1)
    lst, stats = occ.build(g, o, cfg)
    cells, _, _, states = lst
    assert stats["occupied"] > 0 and stats["free"] > 0
    for z_lo, z_hi in ((-10.0, 10.0), (0.0, 0.0), (0.05, 0.35), (-0.2, -0.2), (0.2, 0.2)):
        got = occ.slice_of(lst, cfg, z_lo, z_hi)
        lo, hi = occ.slab(z_lo, z_hi, 0.2)
        inside = [(tuple(c), s) for c, s in zip(cells.tolist(), states.tolist()) if lo <= c[2] <= hi]
        assert inside and got is not None
        info, pixels = got
        xs, ys = [c[0] for c, _ in inside], [c[1] for c, _ in inside]
        assert (info["cx_min"], info["cy_min"], info["width"], info["height"]) == (min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1)
        for row in range(info["height"]):
            for col in range(info["width"]):
                seen = {s for c, s in inside if c[0] == info["cx_min"] + col and c[1] == max(ys) - row}
                assert pixels[row, col] == (0 if 2 in seen else 254 if 1 in seen else 205), (z_lo, z_hi, row, col)
        assert info["occupied"] + info["free"] + info["unknown"] == info["width"] * info["height"] == pixels.size
        assert (info["origin_x"], info["origin_y"]) == (min(xs) * float(f32(0.2)), min(ys) * float(f32(0.2)))
    assert occ.slab(0.2, 0.2, 0.2) == (1, 1) and occ.slab(-0.2, -0.2, 0.2) == (-1, -1)  # float32(0.2) / float32(0.2) is exactly 1: a z on a cell boundary belongs to the cell above
    assert occ.slice_of(lst, cfg, -50.0, -40.0) is None
    assert occ.pgm_bytes(np.array([[0, 254, 205]], np.uint8)) == b"P5\n3 1\n255\n\x00\xfe\xcd"


# ---- M6, M7: the texts ----------------------------------------------------------------------------------------------------------------------------
def test_texts_equal_the_c_calls(lib):
    for n in (0, 1, 123456, 10**12 - 1):
        assert dcl.pcdHeaderOccupancyBinary(n) == occ.pcd_header(n)
    assert "FIELDS x y z hits passes state\nSIZE 4 4 4 4 4 4\nTYPE F F F U U U\n" in dcl.pcdHeaderOccupancyBinary(7) and occ.ROW.itemsize == 24
    for w, h in ((1, 1), (640, 480), (2**14, 2**14)):
        assert dcl.occupancy_map_pgm_header(w, h) == f"P5\n{w} {h}\n255\n"
    for path, cell, x, y in (("map.pgm", 0.2, -17, 4), ("/tmp/some dir/a.b/map.pgm", 0.05, 0, 0), ("rel/m.pgm", 0.37, -(2**20), 2**20 - 1), ("dir/", 1.0, 3, -3)):
        text = dcl.occupancy_map_yaml(path, cell, x, y)
        assert text == occ.yaml_text(path, cell, x, y), (path, text)
        assert len(text.splitlines()) == 6 and text.endswith("free_thresh: 0.196\n")
    assert dcl.occupancy_map_yaml("a/map.pgm", 0.2, -17, 4).splitlines()[:3] == ["image: map.pgm", "resolution: 0.200000003", "origin: [-3.40000005, 0.800000012, 0]"]
    assert occ.centre(-1, 0.2) == f32(-0.1) and occ.centre(0, 0.2) == f32(0.1) and occ.centre(2**20 - 1, 0.2).dtype == f32


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_that_needs_no_device(lib):
    from dmsa_lidar_slam_amd.api import DmsaError

    assert dcl.occupancy_state(None, 1, 0) == 2
    for kw in (dict(min_hits=0), dict(min_hits=2**20 + 1), dict(min_passes=0), dict(min_passes=-3), dict(min_passes=2**20 + 1), dict(occ_num=0), dict(occ_num=2**20 + 1),
               dict(occ_den=0), dict(occ_den=2**20 + 1)):
        assert occ.Config(**kw).rule_refused() and occ.Config(**kw).refused(), kw
        with pytest.raises(DmsaError):
            dcl.occupancy_state(dcl.DenseOccupancyConfig(**kw), 1, 1)
    for kw in (dict(min_hits=2**20), dict(min_passes=2**20), dict(occ_num=2**20), dict(occ_den=2**20), dict(max_length=np.nan), dict(initial_slots=3), dict(cell_size=np.inf)):
        assert not occ.Config(**kw).rule_refused()  # the bounds are legal; the other fields are not looked at
        dcl.occupancy_state(dcl.DenseOccupancyConfig(**kw), 1, 1)
    for kw in (dict(max_length=np.nan), dict(max_length=np.inf), dict(max_length=0.0), dict(max_length=-1.0), dict(initial_slots=3), dict(initial_slots=32), dict(initial_slots=96),
               dict(initial_slots=2**32), dict(initial_slots=-64)):
        assert occ.Config(**kw).refused(), kw
    for kw in (dict(initial_slots=0), dict(initial_slots=64), dict(initial_slots=2**31)):
        assert not occ.Config(**kw).refused(), kw
    cfg = dcl.DenseOccupancyConfig().to_c()
    buf = C.create_string_buffer(512)
    assert lib.dmsa_dense_occupancy_state(None, 1, 1) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_pcd_header_occupancy_binary(-1, buf, 512) == capi.DMSA_ERR_INVALID and lib.dmsa_pcd_header_occupancy_binary(10**12, buf, 512) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_pcd_header_occupancy_binary(5, None, 512) == capi.DMSA_ERR_INVALID and lib.dmsa_pcd_header_occupancy_binary(5, buf, 40) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_occupancy_map_pgm_header(0, 5, buf, 512) == capi.DMSA_ERR_INVALID and lib.dmsa_occupancy_map_pgm_header(5, 0, buf, 512) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_occupancy_map_pgm_header(5, 5, buf, 4) == capi.DMSA_ERR_INVALID and lib.dmsa_occupancy_map_pgm_header(5, 5, None, 64) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_occupancy_map_yaml(None, 0.2, 0, 0, buf, 512) == capi.DMSA_ERR_INVALID and lib.dmsa_occupancy_map_yaml(b"m.pgm", 0.2, 0, 0, buf, 20) == capi.DMSA_ERR_INVALID
    for cell in (0.0, -0.2, np.nan, np.inf):
        assert lib.dmsa_occupancy_map_yaml(b"m.pgm", cell, 0, 0, buf, 512) == capi.DMSA_ERR_INVALID
    # the device calls refuse a null object before they touch anything
    info = capi.DenseOccupancySliceInfo()
    assert lib.dmsa_dense_cloud_build_occupancy(None, C.byref(cfg), None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_occupancy_cells(None, 0, 0, None, None, None, None, None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_save_pcd_occupancy(None, b"/dev/null", 0, None) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_occupancy_slice(None, 0.0, 1.0, C.byref(info), None, 0) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_dense_cloud_save_occupancy_map(None, b"/dev/null", b"/dev/null", 0.0, 1.0) == capi.DMSA_ERR_INVALID
