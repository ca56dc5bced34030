"""GPU tests of include/dmsa_dense_align_plane.h against the model of P0-P9 (tests/dense_align_plane_model.py: the pairs of
dense_compare_model.nearest, Python-int sums and re-centring, a pure-Python solve).  Every comparison is == on integers and on the bits of
doubles: the 64 words are integers whatever the split, and the step is one stated sequence of double operations, so a pair missed or
doubled, a product taken through a float, a limb shifted the wrong way or a fused multiply-add in the solve changes a bit.

The store is one scan on the identity trajectory (tests/test_gpu_dense_normals.py); the normals are the device's own compute_normals,
downloaded and given to the model, so that only this stage is under test.  k_align_plane_sums takes 16 rows per lane and 256 lanes per
workgroup: 4096 rows per workgroup, so 4097 rows are two workgroups."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import dense_align_model as am
import dense_align_plane_model as pm
import dense_compare_model as dm
import test_gpu_dense_cloud as base
import test_gpu_dense_normals as ng

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL, REACH = ng.VOXEL, ng.RADIUS  # 0.05 and 0.2: the sums; the normals' radius there as well
ROOM_VOXEL = 0.1                    # the alignments, normals at 0.3
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


def _dbits(values):
    return [struct.unpack("<Q", struct.pack("<d", float(v)))[0] for v in np.asarray(values, np.float64).reshape(-1)]


def _same_direction(got, want):
    assert list(got) == list(want)
    for k in want:
        a, b = got[k], want[k]
        assert (_dbits([a]) == _dbits([b])) if isinstance(b, float) else a == b, (k, a, b)


def _check_sums(dc, g, normals, ref, reach=REACH, voxel=VOXEL, valid=None):
    """align_plane_sums of the reference as it stands against the model: the 64 words (recombined) and D4's block."""
    valid = dm.valid_rows(ref, voxel) if valid is None else valid
    want, d2, _ = pm.plane_sums(g, normals, ref, valid, reach, voxel)
    got, d4 = dc.align_plane_sums(reach, with_d4=True)
    assert got == want, (got, want)
    _same_direction(d4, dm.direction(d2, valid, reach, reach))
    assert d4["matched"] == want["n"] + want["no_normal"]
    return want


def _same_result(got, want):
    """align_reference(metric="plane") against the model: the transform, every history entry, the stop, the sums."""
    assert got["stop"] == want["stop"] and got["iterations"] == want["iterations"] == len(got["history"]), (got["stop"], got["iterations"], want["stop"], want["iterations"])
    assert got["scale_c"] == want["scale_c"] and got["sums"] == want["sums"]
    for k, (a, b) in enumerate(zip(got["history"], want["history"])):
        assert list(a) == list(b)
        for name in b:
            assert (_dbits([a[name]]) == _dbits([b[name]])) if isinstance(b[name], float) else a[name] == b[name], (k, name, a[name], b[name])
    assert got["transform"].shape == (3, 4) and got["transform"].dtype == np.float64
    assert _dbits(got["transform"]) == _dbits(want["transform"]), (got["transform"], want["transform"])


# ---- 1. the sums -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sum_cloud(opt):
    """3 000 rows in a cube of 1.6 m and 40 isolated rows half a metre apart: those have fewer than min_neighbours neighbours and no normal."""
    rng = np.random.default_rng(61)
    cube = ng._one_per_voxel(rng, 3000, VOXEL, 32, corner=(-0.7, -0.9, -0.8))
    lonely = (np.stack([3.0 + 0.5 * np.arange(40), np.zeros(40), np.zeros(40)], axis=1) + rng.uniform(0.01, 0.04, (40, 3))).astype(f32)
    dc, _ = ng._still_cloud(opt, np.concatenate([cube, lonely]), VOXEL)
    g, _ = dc.retained()
    normals, without = dc.compute_normals(radius=REACH)
    assert g.shape[0] == 3040 and without >= 40 and np.isnan(normals[3000:, :3]).all() and np.isfinite(normals[:3000, :3]).all(axis=1).sum() > 2900
    assert sum(n is None for n in pm.quantise_normals(normals)) == without
    yield dc, g, normals
    dc.close()


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_the_sums_at_every_row_count(sum_cloud, rows):
    dc, g, normals = sum_cloud
    rng = np.random.default_rng(rows)
    ref = (g[rng.integers(0, 3000, rows), :3] + rng.uniform(-0.02, 0.02, (rows, 3))).astype(f32)
    dc.set_reference(ref)
    want = _check_sums(dc, g, normals, ref)
    assert want["n"] + want["no_normal"] == rows and want["n"] > 0.9 * rows


def test_the_sums_of_a_reference_that_matches_nothing_are_all_zero(sum_cloud):
    dc, g, normals = sum_cloud
    rng = np.random.default_rng(2)
    ref = (rng.uniform(-1, 1, (700, 3)) + np.array([0.0, 50.0, 0.0])).astype(f32)
    dc.set_reference(ref)
    want = _check_sums(dc, g, normals, ref)
    assert want == pm.sums_of_pairs([], [], []) and dc.align_plane_sums(REACH, with_d4=True)[1]["unmatched"] == 700


def test_invalid_rows_take_no_part_rows_without_a_normal_are_counted_and_identical_rows_all_count(sum_cloud):
    dc, g, normals = sum_cloud
    rng = np.random.default_rng(3)
    ref = (g[rng.integers(0, 3000, 900), :3] + rng.uniform(-0.3, 0.3, (900, 3))).astype(f32)  # some beyond the reach
    ref[5], ref[64], ref[300, 1], ref[899, 2] = np.nan, np.inf, -np.inf, np.nan
    ref[7], ref[640] = (1e6, 0.0, 0.0), (0.0, -60000.0, 0.0)  # outside rule 6's grid at 0.05 m
    valid = dm.valid_rows(ref, VOXEL)
    assert valid.sum() == 894
    dc.set_reference(ref)
    want = _check_sums(dc, g, normals, ref, valid=valid)
    assert 100 < want["n"] + want["no_normal"] < 894
    # rows at the isolated store rows: matched, without a normal
    near_lonely = np.concatenate([g[3000:3040, :3] + f32(0.01), g[:60, :3] + f32(0.01)]).astype(f32)
    dc.set_reference(near_lonely)
    want = _check_sums(dc, g, normals, near_lonely)
    assert want["no_normal"] >= 40 and want["n"] + want["no_normal"] == 100 and want["n"] > 50
    dc.set_reference(near_lonely[:40])
    want = _check_sums(dc, g, normals, near_lonely[:40])
    assert want["no_normal"] == 40 and want["n"] == 0 and all(v == 0 for v in want["cc"] + want["sp"])
    same = np.repeat((g[1234:1235, :3] + f32(0.01)).astype(f32), 200, axis=0)
    dc.set_reference(same)
    want = _check_sums(dc, g, normals, same)
    assert want["n"] == 200 and want["sp"][0] % 200 == 0 and want["ee"] % 200 == 0


def test_the_sums_at_the_edge_of_the_grid(opt):
    """Coordinates just inside +-2^20 voxels of 0.05 m, 52 428.8 m, in two clusters of opposite signs: |P| near 2^29.7, c near 2^44 in either
    sign, c * c near 2^88 and c * N near 2^58: the third limb is in use, the top limbs of the mixed sums are negative.  A 64-bit product, an
    unsigned shift for a top limb or a float anywhere cannot pass this."""
    rng = np.random.default_rng(71)
    far = 52400.0
    a = ng._one_per_voxel(rng, 1500, VOXEL, 24, corner=(far, -far - 1.2, far))
    b = ng._one_per_voxel(rng, 1500, VOXEL, 24, corner=(-far - 1.2, far, -far - 1.2))
    dc, _ = ng._still_cloud(opt, np.concatenate([a, b]), VOXEL)
    g, _ = dc.retained()
    normals, without = dc.compute_normals(radius=REACH)
    assert g.shape[0] > 2500 and np.abs(g[:, :3]).min() > 52000 and without < g.shape[0] // 2
    ref = g[rng.integers(0, g.shape[0], 5000), :3].copy()
    ref += (rng.integers(-8, 9, ref.shape) * 2.0**-8).astype(f32)  # a few float steps at this magnitude: up to 0.03 m per axis
    dc.set_reference(ref)
    want = _check_sums(dc, g, normals, ref)
    assert want["n"] > 2500 and want["cc"][0] > 2**96 and min(min(r) for r in want["cn"]) < -(2**63) and max(max(r) for r in want["cn"]) > 2**63
    assert abs(want["sp"][0]) < 2**41 and want["ee"] > 0
    dc.close()


# ---- 2. the alignment of the room ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room(opt):
    """The room of tests/test_dense_align_plane_cpu.py with the device's normals at 0.3 m, 1 000 reference rows with 1 cm noise displaced by 2
    degrees and 0.146 m; the model once."""
    rng = np.random.default_rng(5)
    dc, _ = ng._still_cloud(opt, am.room(rng), ROOM_VOXEL)
    g, o = dc.retained()
    normals, without = dc.compute_normals(radius=0.3)
    motion = am.rigid(2.0, (0.2, -0.3, 1.0), (0.1, -0.08, 0.07))
    ref = am.sample_reference(rng, g, 1000, 0.01, motion)
    want = pm.align(g, normals, ref, ROOM_VOXEL)
    assert g.shape[0] > 4500 and without < 100 and want["stop"] == "CONVERGED" and 2 <= want["iterations"] <= 6
    assert np.abs(np.array(want["transform"]).reshape(3, 4) - motion).max() < 2e-3
    yield dc, g, o, normals, ref, want
    dc.close()


def test_the_alignment_equals_the_model_bit_for_bit_and_twice_gives_the_same_bytes(room):
    dc, g, _, normals, ref, want = room
    got = dc.align_reference(ref, metric="plane")
    _same_result(got, want)
    again = dc.align_reference(ref, metric="plane")
    assert again["transform"].tobytes() == got["transform"].tobytes() and again["history"] == got["history"] and again["sums"] == got["sums"]
    _same_result(dc.align_reference(ref, transform=np.eye(4), metric="plane"), want)
    with pytest.raises(ValueError):
        dc.align_reference(ref, metric="planes")


def test_the_state_afterwards_is_that_of_set_reference_with_the_result(opt, room):
    dc, g, _, normals, ref, want = room
    got = dc.align_reference(ref, metric="plane")
    other, _ = ng._still_cloud(opt, g[:, :3], ROOM_VOXEL)
    g2, _ = other.retained()
    assert np.array_equal(_bits(g2), _bits(g))
    other.set_reference(ref, got["transform"])
    assert dc.reference_count() == other.reference_count() == 1000
    (xyz, valid), (xyz2, valid2) = dc.reference(), other.reference()
    assert np.array_equal(_bits(xyz), _bits(xyz2)) and np.array_equal(valid, valid2)
    assert np.array_equal(_bits(xyz), _bits(dm.transform(ref, got["transform"])))
    assert dc.compare(1.0, 0.1) == other.compare(1.0, 0.1)
    assert dc.align_sums(1.0) == other.align_sums(1.0)
    # the normals are untouched: the stage call on this object equals the model on the normals downloaded before
    _check_sums(dc, g, normals, xyz, reach=1.0, voxel=ROOM_VOXEL)
    other.close()


# ---- 3. the stop reasons --------------------------------------------------------------------------------------------------------------------------------
def test_max_iterations_and_too_few_pairs(room):
    dc, g, _, normals, ref, want = room
    short = pm.align(g, normals, ref, ROOM_VOXEL, max_iterations=2)
    assert short["stop"] == "MAX_ITERATIONS" and short["iterations"] == 2 and short["history"] == want["history"][:2]
    _same_result(dc.align_reference(ref, max_iterations=2, metric="plane"), short)
    rng = np.random.default_rng(16)
    T0 = am.rigid(3.0, (1.0, 0.0, 0.0), (0.0, 0.0, 0.5))
    disjoint = (rng.uniform(-1, 1, (300, 3)) + np.array([0.0, 40.0, 0.0])).astype(f32)
    got = dc.align_reference(disjoint, transform=T0, metric="plane")
    _same_result(got, pm.align(g, normals, disjoint, ROOM_VOXEL, T0=T0))
    assert got["stop"] == "TOO_FEW_PAIRS" and got["iterations"] == 1 and got["history"][0]["used"] == 0 and got["history"][0]["unmatched"] == 300
    assert got["transform"].tobytes() == T0.tobytes() and got["history"][0]["shift_m"] == 0.0 and got["history"][0]["min_pivot"] == 0.0
    assert np.array_equal(_bits(dc.reference()[0]), _bits(dm.transform(disjoint, T0)))  # P8 holds here too
    # exactly min_pairs - 1 used pairs
    five = np.concatenate([g[[10, 700, 2000, 3000, 4000], :3] + f32(0.02), disjoint[:50]]).astype(f32)
    got = dc.align_reference(five, metric="plane")
    _same_result(got, pm.align(g, normals, five, ROOM_VOXEL))
    assert got["stop"] == "TOO_FEW_PAIRS" and got["history"][0]["used"] == 5 and got["sums"]["n"] == 5 and np.array_equal(got["transform"], np.eye(3, 4))
    got = dc.align_reference(np.full((5, 3), np.nan, f32), metric="plane")
    assert got["stop"] == "TOO_FEW_PAIRS" and got["history"][0]["matched"] == 0 and dc.reference_count() == 5 and not dc.reference()[1].any()


def test_a_flat_lattice_with_normals_exactly_along_z_is_degenerate(opt):
    xs = np.arange(0.05, 3.0, 0.2)
    flat = np.stack([*(v.ravel() for v in np.meshgrid(xs, xs, indexing="ij")), np.zeros(xs.size**2)], axis=1).astype(f32)
    dc, _ = ng._still_cloud(opt, flat, ROOM_VOXEL)
    g, _ = dc.retained()
    normals, without = dc.compute_normals(radius=0.3)
    have = np.isfinite(normals[:, 0])
    assert g.shape[0] == 225 and without == 4 and have.sum() == 221
    assert np.array_equal(np.abs(normals[have, :3]), np.tile(np.array([0.0, 0.0, 1.0], f32), (221, 1)))  # exactly +-e_z
    ref = (g[:, :3] + np.array([0.01, 0.0, 0.02])).astype(f32)
    T0 = am.rigid(0.2, (0, 0, 1), (0.0, 0.01, 0.0))
    got = dc.align_reference(ref, transform=T0, metric="plane")
    _same_result(got, pm.align(g, normals, ref, ROOM_VOXEL, T0=T0))
    h = got["history"][0]
    assert got["stop"] == "DEGENERATE" and got["iterations"] == 1 and got["transform"].tobytes() == T0.tobytes() and h["used"] > 200 and h["min_pivot"] <= 2.0**-40
    assert h["shift_m"] == 0.0 and h["rotation_rad"] == 0.0 and h["plane_rms_m"] > 0.01
    assert np.array_equal(_bits(dc.reference()[0]), _bits(dm.transform(ref, T0)))  # no step was applied: P8 with T0
    dc.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_missing_and_stale_normals_and_every_breach_of_p0_are_refused_and_leave_no_reference(opt):
    rng = np.random.default_rng(51)
    ref = rng.uniform(0, 0.5, (50, 3)).astype(f32)
    dc, _ = ng._still_cloud(opt, ng._one_per_voxel(rng, 400, VOXEL, 10), VOXEL)
    no_normals = "no normals of the store as it stands"

    def refused_and_dropped(call, text):
        dc.set_reference(ref)
        _refused(call, text)
        assert dc.reference_count() == 0

    refused_and_dropped(lambda: dc.align_reference(ref, max_distance=REACH, metric="plane"), no_normals)
    dc.set_reference(ref)
    _refused(lambda: dc.align_plane_sums(REACH), no_normals)
    assert dc.reference_count() == 50  # the stage call leaves the reference alone
    dc.compute_normals(radius=REACH)
    assert dc.align_reference(ref, max_distance=REACH, metric="plane")["iterations"] >= 1 and dc.reference_count() == 50
    _refused(lambda: dc.align_plane_sums(np.nan), "max_distance is not finite")
    dc.set_reference(np.full((4, 3), np.nan, f32))
    _refused(lambda: dc.align_plane_sums(REACH), "the reference cloud has no valid row")
    T = np.eye(4)[:3].copy()
    T[2, 0] = np.nan
    refused_and_dropped(lambda: dc.align_reference(ref, transform=T, max_distance=REACH, metric="plane"), "the transform is not finite")
    for reach, text in ((np.inf, "max_distance is not finite"), (0.04, "max_distance must lie in [voxel_size, 64 * voxel_size]"), (3.3, "max_distance must lie in [voxel_size, 64 * voxel_size]")):
        refused_and_dropped(lambda: dc.align_reference(ref, max_distance=reach, metric="plane"), text)
    for kw, text in ((dict(max_iterations=0), "max_iterations must lie in [1, 64]"), (dict(max_iterations=65), "max_iterations must lie in [1, 64]"),
                     (dict(min_pairs=5), "min_pairs must be at least 6"), (dict(stop_translation=-1e-9), "stop_translation must be finite and >= 0"),
                     (dict(stop_rotation=np.inf), "stop_rotation must be finite and >= 0")):
        refused_and_dropped(lambda: dc.align_reference(ref, max_distance=REACH, metric="plane", **kw), text)
    # a compaction makes the normals stale
    stats = dc.classify_outliers(radius=REACH, k=8, stddev_mul=0.5)
    assert 0 < stats["inliers"] < 400 and dc.remove_outliers() == stats["inliers"]
    refused_and_dropped(lambda: dc.align_reference(ref, max_distance=REACH, metric="plane"), no_normals)
    dc.set_reference(ref)
    _refused(lambda: dc.align_plane_sums(REACH), no_normals)
    dc.compute_normals(radius=REACH)
    got = dc.align_reference(ref, max_distance=REACH, max_iterations=64, min_pairs=6, stop_translation=0.0, stop_rotation=0.0, metric="plane")
    assert got["iterations"] >= 1 and dc.reference_count() == 50
    dc.close()
    off, _ = ng._creator(opt, retain=False, still=True, voxel_size=VOXEL)
    off.add_scan(np.full((1, 3), 0.5, f32), ng._stamps(1))
    _refused(lambda: off.align_reference(ref, max_distance=REACH, metric="plane"), "retention is off")
    off.close()


# ---- 5. independence ------------------------------------------------------------------------------------------------------------------------------------
def test_the_point_to_point_call_and_the_other_stages_are_what_they_were_and_the_intensity_object_behaves_the_same(opt, room):
    from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator

    dc, g, o, normals, ref, want = room
    point_want = am.align(g, ref, ROOM_VOXEL)
    before = dc.align_reference(ref)
    between = dc.align_reference(ref, metric="plane")
    after = dc.align_reference(ref)
    for got in (before, after):
        assert got["stop"] == point_want["stop"] and got["history"] == point_want["history"] and got["sums"] == point_want["sums"]
        assert _dbits(got["transform"]) == _dbits(point_want["transform"])
    _same_result(between, want)
    g2, o2 = dc.retained()
    assert np.array_equal(_bits(g2), _bits(g)) and np.array_equal(_bits(o2), _bits(o))
    again, _ = dc.compute_normals(radius=0.3)
    assert np.array_equal(again.view(np.uint8), normals.view(np.uint8))
    s, p, q = base._still_trajectory()
    with_i = DenseCloudCreator(s, p, q, DenseCloudConfig(voxelSize=ROOM_VOXEL), optimizer=opt, retain=True, intensity=True)
    rows = np.concatenate([g[:, :3], np.arange(g.shape[0], dtype=f32)[:, None]], axis=1).astype(f32)
    with_i.add_scan(rows, ng._stamps(rows.shape[0]))
    gi, _ = with_i.retained()
    assert np.array_equal(_bits(gi[:, :3]), _bits(g[:, :3])) and np.array_equal(gi[:, 3], rows[:, 3])
    ni, _ = with_i.compute_normals(radius=0.3)
    assert np.array_equal(ni.view(np.uint8), normals.view(np.uint8))
    _same_result(with_i.align_reference(ref, metric="plane"), want)
    gi2, _ = with_i.retained()
    assert np.array_equal(_bits(gi2), _bits(gi))
    with_i.close()


# ---- 6. the programs ------------------------------------------------------------------------------------------------------------------------------------
def test_both_programs_align_a_displaced_copy_of_the_file_they_wrote_by_point_to_plane(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import dense_cloud_demo
    from dmsa_lidar_slam_amd import dense_cloud as dcl

    r = dense_cloud_demo.run(scans=6, workdir=str(tmp_path))
    xyz = dcl.read_pcd_xyz(r["pcd"])
    applied = dense_cloud_demo.displacement(1.0, 0.08, xyz.mean(axis=0))
    moved = (xyz.astype(np.float64) @ applied[:, :3].T + applied[:, 3]).astype(f32)
    displaced = tmp_path / "displaced.pcd"
    with open(displaced, "wb") as f:
        f.write(dcl.pcdHeaderXyzBinary(moved.shape[0]).encode() + moved.tobytes())
    exe = os.path.join(ROOT, "examples", "dense_cloud_from_raw")
    t_out = tmp_path / "T.txt"
    p = subprocess.run([exe, r["dump"], r["poses_file"], "ouster", str(tmp_path / "b.pcd"), "--voxel", "0.1", "--min-range", "0.5", "--compare", str(displaced), "--align",
                        "--align-metric", "plane", "--align-out", str(t_out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
    lines = re.findall(r"^align: iteration (\d+)  matched (\d+) .* used (\d+)  plane rms [0-9.]+ m  min pivot [0-9.e+-]+$", p.stdout, re.M)
    stop = re.search(r"^align: .*stop ([A-Z_]+) after (\d+) iterations$", p.stdout, re.M)
    assert stop and int(stop.group(2)) == len(lines) >= 2 and stop.group(1) in ("CONVERGED", "MAX_ITERATIONS") and all(0 < int(u) <= int(m) for _, m, u in lines)
    T = dcl.read_transform(t_out)
    assert np.abs(T - dense_cloud_demo.inverse_motion(applied)).max() < 0.05  # (it found its way back: the figures are the model's business)
    assert float(re.search(r"^compare: .*\bprecision ([0-9.]+)", p.stdout, re.M).group(1)) > 0.9
    assert open(tmp_path / "b.pcd", "rb").read() == open(r["pcd"], "rb").read()
    bad = subprocess.run([exe, r["dump"], r["poses_file"], "ouster", str(tmp_path / "c.pcd"), "--voxel", "0.1", "--compare", str(displaced), "--align-metric", "planar"],
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dense_cloud_demo.py"), "--scans", "6", "--compare", r["pcd"], "--align", "--align-metric", "plane",
                        "--compare-displace", "1.0,0.08", "--compare-out", str(tmp_path / "Dist.pcd"), "--out", str(tmp_path / "Dense2.pcd")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert re.search(r"^align: stop (CONVERGED|MAX_ITERATIONS) after \d+ iterations$", p.stdout, re.M) and re.search(r"^align iteration 0: .* used \d+  plane rms ", p.stdout, re.M)
    assert float(re.search(r"^align: largest entry difference ([0-9.e+-]+)$", p.stdout, re.M).group(1)) < 0.05
    assert float(re.search(r"^compare .*\bprecision ([0-9.]+)", p.stdout, re.M).group(1)) > 0.9


# ---- 7. the callers of the one pair pass on one object ----------------------------------------------------------------------------------------------------
def test_compare_both_stage_calls_and_a_range_call_interleaved_on_one_object_give_what_each_gives_alone(sum_cloud):
    """compare(), align_sums(), align_plane_sums() and a range call of nearest_in_store() go through one pair pass (dense_compare_api.cpp) and share
    the buffers of the completeness direction; the two stage calls share one copy-back slot as well.  One object, a reference of two
    workgroups and then one of 65 rows: the range call shrinks those buffers and the next call grows them again, the plane call's block
    follows the shorter point block into the slot, and every result is the model's.  The range [63, 193) lies beyond a reference of 65 rows:
    there that call is refused and changes nothing, and the range cut to the reference runs in its place."""
    import test_gpu_dense_align as ag
    import test_gpu_dense_compare as cg

    dc, g, normals = sum_cloud
    for rows in (4097, 65):
        rng = np.random.default_rng(700 + rows)
        ref = (g[rng.integers(0, 3000, rows), :3] + rng.uniform(-0.02, 0.02, (rows, 3))).astype(f32)
        ref[5], ref[64] = np.nan, (0.0, 50.0, 0.0)  # an invalid row and one that matches nothing
        valid = dm.valid_rows(ref, VOXEL)
        dc.set_reference(ref)
        want, (_, _, c_d2, c_idx) = dm.compare(g, ref, valid, REACH, cg.TOL)
        first = dc.compare(REACH, cg.TOL)
        cg._stats_equal(first, want)
        ag._check_sums(dc, g, ref, valid=valid)
        _check_sums(dc, g, normals, ref, valid=valid)
        if rows < 193:
            _refused(lambda: dc.nearest_in_store(REACH, 63, 130), "rows beyond the reference cloud")
        count = min(130, rows - 63)
        cg._same(dc.nearest_in_store(REACH, 63, count), (c_d2[63 : 63 + count], c_idx[63 : 63 + count]))
        again = dc.compare(REACH, cg.TOL)
        cg._stats_equal(again, want)
        assert again == first and first["ref_rows"] == rows and first["ref_invalid"] == 1 and first["completeness"]["unmatched"] >= 1
