"""GPU tests of include/dmsa_dense_align.h against the model of A0-A8 (tests/dense_align_model.py: the pairs of dense_compare_model.nearest,
Python-int sums, a pure-Python solve).  Every comparison is == on integers and on the bits of doubles: the 25 sums are integers whatever the
split, and the step is one stated sequence of double operations, so a pair missed or doubled, a product taken through a float or a 32-bit
accumulator, or a fused multiply-add in the solve changes a bit.

The store is one scan on the identity trajectory (tests/test_gpu_dense_normals.py), what the object retained is what the model is given.
k_align_pair_sums takes 16 rows per lane and 256 lanes per workgroup: 4096 rows per workgroup, so 4097 rows are two workgroups and 5000 is
no multiple of either."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import dense_align_model as am
import dense_compare_model as dm
import test_gpu_dense_cloud as base
import test_gpu_dense_normals as ng

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL, REACH = ng.VOXEL, ng.RADIUS  # 0.05 and 0.2: the sums
ROOM_VOXEL = 0.1                    # the alignments
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


def _check_sums(dc, g, ref, reach=REACH, voxel=VOXEL, valid=None):
    """align_sums of the reference as it stands against the model: the 25 words (recombined) and D4's block."""
    valid = dm.valid_rows(ref, voxel) if valid is None else valid
    want, d2, _ = am.pair_sums(g, ref, valid, reach, voxel)
    got, d4 = dc.align_sums(reach, with_d4=True)
    assert got == want, (got, want)
    _same_direction(d4, dm.direction(d2, valid, reach, reach))
    return want


def _same_result(got, want):
    """align_reference against the model: the transform, every history entry, the stop, the sums."""
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
    rng = np.random.default_rng(61)
    dc, _ = ng._still_cloud(opt, ng._one_per_voxel(rng, 3000, VOXEL, 32, corner=(-0.7, -0.9, -0.8)), VOXEL)
    g, _ = dc.retained()
    assert g.shape[0] == 3000
    yield dc, g
    dc.close()


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257, 4097, 5000])
def test_the_sums_with_every_reference_row_matched(sum_cloud, rows):
    dc, g = sum_cloud
    rng = np.random.default_rng(rows)
    ref = (g[rng.integers(0, g.shape[0], rows), :3] + rng.uniform(-0.02, 0.02, (rows, 3))).astype(f32)
    dc.set_reference(ref)
    want = _check_sums(dc, g, ref)
    assert want["n"] == rows


def test_the_sums_of_a_reference_that_matches_nothing_are_all_zero(sum_cloud):
    dc, g = sum_cloud
    rng = np.random.default_rng(2)
    ref = (rng.uniform(-1, 1, (700, 3)) + np.array([50.0, 0.0, 0.0])).astype(f32)
    dc.set_reference(ref)
    want = _check_sums(dc, g, ref)
    assert want == dict(n=0, sp=[0, 0, 0], sg=[0, 0, 0], spg=[[0, 0, 0]] * 3)
    assert dc.align_sums(REACH, with_d4=True)[1]["unmatched"] == 700


def test_invalid_reference_rows_take_no_part_and_identical_rows_all_count(sum_cloud):
    dc, g = sum_cloud
    rng = np.random.default_rng(3)
    ref = (g[rng.integers(0, g.shape[0], 900), :3] + rng.uniform(-0.3, 0.3, (900, 3))).astype(f32)  # some beyond the reach
    ref[5], ref[64], ref[300, 1], ref[899, 2] = np.nan, np.inf, -np.inf, np.nan
    ref[7], ref[640] = (1e6, 0.0, 0.0), (0.0, -60000.0, 0.0)  # outside rule 6's grid at 0.05 m
    valid = dm.valid_rows(ref, VOXEL)
    assert valid.sum() == 894
    dc.set_reference(ref)
    want = _check_sums(dc, g, ref, valid=valid)
    assert 100 < want["n"] < 894
    same = np.repeat((g[1234:1235, :3] + f32(0.01)).astype(f32), 200, axis=0)
    dc.set_reference(same)
    want = _check_sums(dc, g, same)
    assert want["n"] == 200 and want["sp"][0] % 200 == 0


def test_the_sums_at_the_edge_of_the_grid_where_a_product_is_near_two_to_the_sixty(opt):
    """Coordinates just inside +-2^20 voxels of 0.05 m, 52 428.8 m, in two clusters of opposite signs: |P|, |G| near 2^29.7, every product
    near 2^59.4 in either sign, lo carries past 2^32 thousands of times, hi is negative for the mixed sums.  A 32-bit or float accumulator,
    or an unsigned shift for hi, cannot pass this."""
    rng = np.random.default_rng(71)
    far = 52400.0
    a = ng._one_per_voxel(rng, 1500, VOXEL, 24, corner=(far, -far - 1.2, far))
    b = ng._one_per_voxel(rng, 1500, VOXEL, 24, corner=(-far - 1.2, far, -far - 1.2))
    dc, _ = ng._still_cloud(opt, np.concatenate([a, b]), VOXEL)
    g, _ = dc.retained()
    assert g.shape[0] > 2500 and np.abs(g[:, :3]).min() > 52000
    ref = g[rng.integers(0, g.shape[0], 5000), :3].copy()
    ref += (rng.integers(-8, 9, ref.shape) * 2.0**-8).astype(f32)  # a few float steps at this magnitude: up to 0.03 m per axis
    dc.set_reference(ref)
    want = _check_sums(dc, g, ref)
    assert want["n"] == 5000 and want["spg"][0][0] > 2**70 and want["spg"][0][1] < -(2**70) and abs(want["sp"][0]) < 2**40
    dc.close()


# ---- 2. the alignment of the room ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room(opt):
    """The room of tests/test_dense_align_cpu.py, 1 000 reference rows with 1 cm noise displaced by 2 degrees and 0.146 m; the model once."""
    rng = np.random.default_rng(5)
    dc, _ = ng._still_cloud(opt, am.room(rng), ROOM_VOXEL)
    g, o = dc.retained()
    motion = am.rigid(2.0, (0.2, -0.3, 1.0), (0.1, -0.08, 0.07))
    ref = am.sample_reference(rng, g, 1000, 0.01, motion)
    want = am.align(g, ref, ROOM_VOXEL)
    assert g.shape[0] > 4500 and want["stop"] == "CONVERGED" and 3 < want["iterations"] <= 20
    assert np.abs(np.array(want["transform"]).reshape(3, 4) - motion).max() < 1e-3
    yield dc, g, o, ref, want
    dc.close()


def test_the_alignment_equals_the_model_bit_for_bit_and_twice_gives_the_same_bytes(room):
    dc, g, _, ref, want = room
    got = dc.align_reference(ref)
    _same_result(got, want)
    again = dc.align_reference(ref)
    assert again["transform"].tobytes() == got["transform"].tobytes() and again["history"] == got["history"] and again["sums"] == got["sums"]
    # from a start: the identity given as a matrix is the identity
    _same_result(dc.align_reference(ref, transform=np.eye(4)), want)


def test_the_state_afterwards_is_that_of_set_reference_with_the_result(opt, room):
    dc, g, _, ref, want = room
    got = dc.align_reference(ref)
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
    other.close()


def test_max_iterations_stops_after_the_last_step(room):
    dc, g, _, ref, want = room
    short = am.align(g, ref, ROOM_VOXEL, max_iterations=2)
    assert short["stop"] == "MAX_ITERATIONS" and short["iterations"] == 2 and short["history"] == want["history"][:2]
    _same_result(dc.align_reference(ref, max_iterations=2), short)
    # the result of two steps is a start like any other
    rest = dc.align_reference(ref, transform=np.array(short["transform"]).reshape(3, 4), max_iterations=1)
    assert rest["history"][0]["matched"] == want["history"][2]["matched"] and _dbits([rest["history"][0]["rms_m"]]) == _dbits([want["history"][2]["rms_m"]])


def test_a_partial_overlap_where_rows_enter_and_leave_the_reach(opt, room):
    """The reference runs 2 m beyond the store along x and the reach is 0.3 m: most rows out there are unmatched, and `matched` goes up and
    down from one iteration to the next as rows enter and leave the reach (the model: 676 678 678 673 670 660 ... 658).  A monotonicity stop
    would end this early; the model has none and stops CONVERGED after 12 iterations.  (The overhang biases the fit by a centimetre: trimming
    is out of scope.)"""
    dc, g, _, _, _ = room
    rng = np.random.default_rng(15)
    motion = am.rigid(1.0, (0.1, 0.2, 1.0), (0.1, -0.05, 0.03))
    inside = g[rng.choice(g.shape[0], 600, replace=False), :3].astype(np.float64) + rng.normal(0.0, 0.01, (600, 3))
    beyond = np.stack([rng.uniform(4.0, 6.0, 400), rng.uniform(-3.0, 3.0, 400), np.full(400, -1.0)], axis=1)  # the floor, continued
    inv = am.inverse(motion)
    ref = (np.concatenate([inside, beyond]) @ inv[:, :3].T + inv[:, 3]).astype(f32)
    want = am.align(g, ref, ROOM_VOXEL, max_distance=0.3)
    matched = [h["matched"] for h in want["history"]]
    assert len(set(matched)) > 3 and all(0 < h["unmatched"] < 400 for h in want["history"]) and want["stop"] == "CONVERGED" and 3 < want["iterations"] <= 20
    assert any(b < a for a, b in zip(matched, matched[1:])) and any(b > a for a, b in zip(matched, matched[1:]))
    _same_result(dc.align_reference(ref, max_distance=0.3), want)


# ---- 3. the stop reasons --------------------------------------------------------------------------------------------------------------------------------
def test_too_few_pairs_gives_no_step(room):
    dc, g, _, _, _ = room
    rng = np.random.default_rng(16)
    T0 = am.rigid(3.0, (1.0, 0.0, 0.0), (0.0, 0.0, 0.5))
    disjoint = (rng.uniform(-1, 1, (300, 3)) + np.array([0.0, 40.0, 0.0])).astype(f32)
    got = dc.align_reference(disjoint, transform=T0)
    _same_result(got, am.align(g, disjoint, ROOM_VOXEL, T0=T0))
    assert got["stop"] == "TOO_FEW_PAIRS" and got["iterations"] == 1 and got["history"][0]["matched"] == 0 and got["history"][0]["unmatched"] == 300
    assert got["transform"].tobytes() == T0.tobytes() and got["history"][0]["shift_m"] == 0.0
    assert np.array_equal(_bits(dc.reference()[0]), _bits(dm.transform(disjoint, T0)))  # A7 holds here too
    # exactly min_pairs - 1 pairs
    two = np.concatenate([g[[10, 2000], :3] + f32(0.02), disjoint[:50]]).astype(f32)
    got = dc.align_reference(two, min_pairs=3)
    assert got["stop"] == "TOO_FEW_PAIRS" and got["history"][0]["matched"] == 2 and got["sums"]["n"] == 2 and np.array_equal(got["transform"], np.eye(3, 4))
    _same_result(got, am.align(g, two, ROOM_VOXEL))
    got = dc.align_reference(two, min_pairs=3, max_iterations=1, max_distance=1.0)
    assert got["stop"] == "TOO_FEW_PAIRS"
    # a reference without a valid row has no pair either
    got = dc.align_reference(np.full((5, 3), np.nan, f32))
    assert got["stop"] == "TOO_FEW_PAIRS" and got["history"][0] == dict(matched=0, unmatched=0, s2=0, rms_m=0.0, shift_m=0.0, rotation_rad=0.0)
    assert dc.reference_count() == 5 and not dc.reference()[1].any()


def test_an_identical_cloud_converges_at_iteration_zero(room):
    dc, g, _, _, _ = room
    ref = g[::5, :3].copy()
    got = dc.align_reference(ref)
    _same_result(got, am.align(g, ref, ROOM_VOXEL))
    assert got["stop"] == "CONVERGED" and got["iterations"] == 1 and got["history"][0] == dict(matched=ref.shape[0], unmatched=0, s2=0, rms_m=0.0, shift_m=0.0, rotation_rad=0.0)
    assert np.array_equal(got["transform"], np.eye(3, 4))  # the identity composed with an identity step


# ---- 4. independence ------------------------------------------------------------------------------------------------------------------------------------
def test_the_store_and_the_other_stages_are_untouched_and_the_intensity_object_behaves_the_same(opt, room):
    from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator

    dc, g, o, ref, want = room
    normals_before = dc.compute_normals(radius=0.3)
    flags_before = dc.classify_outliers(radius=0.3, download=True)
    labels_before = dc.cluster_labels(0.3)
    dc.align_reference(ref)
    g2, o2 = dc.retained()
    assert np.array_equal(_bits(g2), _bits(g)) and np.array_equal(_bits(o2), _bits(o)) and dc.retained_count() == g.shape[0]
    for before, after in ((normals_before, dc.compute_normals(radius=0.3)), (flags_before, dc.classify_outliers(radius=0.3, download=True)),
                          (labels_before, dc.cluster_labels(0.3))):
        for a, b in zip(before, after):
            assert (a == b) if not isinstance(a, np.ndarray) else np.array_equal(a.view(np.uint8), b.view(np.uint8))
    s, p, q = base._still_trajectory()
    with_i = DenseCloudCreator(s, p, q, DenseCloudConfig(voxelSize=ROOM_VOXEL), optimizer=opt, retain=True, intensity=True)
    rows = np.concatenate([g[:, :3], np.arange(g.shape[0], dtype=f32)[:, None]], axis=1).astype(f32)
    with_i.add_scan(rows, ng._stamps(rows.shape[0]))
    gi, _ = with_i.retained()
    assert np.array_equal(_bits(gi[:, :3]), _bits(g[:, :3])) and np.array_equal(gi[:, 3], rows[:, 3])
    _same_result(with_i.align_reference(ref), want)
    gi2, _ = with_i.retained()
    assert np.array_equal(_bits(gi2), _bits(gi))
    with_i.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_every_breach_of_a0_is_refused_with_its_reason_and_leaves_no_reference(opt):
    from dmsa_lidar_slam_amd import _capi as capi

    rng = np.random.default_rng(51)
    ref = rng.uniform(0, 0.5, (50, 3)).astype(f32)
    off, _ = ng._creator(opt, retain=False, still=True, voxel_size=VOXEL)
    off.add_scan(np.full((1, 3), 0.5, f32), ng._stamps(1))
    _refused(lambda: off.align_reference(ref, max_distance=REACH), "retention is off")
    off.set_reference(ref)
    _refused(lambda: off.align_sums(REACH), "retention is off")
    off.close()
    empty, _ = ng._creator(opt, still=True, voxel_size=VOXEL)
    _refused(lambda: empty.align_reference(ref, max_distance=REACH), "no retained point")
    empty.close()
    dc, _ = ng._still_cloud(opt, ng._one_per_voxel(rng, 100, VOXEL, 8), VOXEL)
    lib, handle = dc._lib, dc._dc
    _refused(lambda: dc.align_sums(REACH), "no reference cloud")
    dc.set_reference(np.full((4, 3), np.nan, f32))
    _refused(lambda: dc.align_sums(REACH), "the reference cloud has no valid row")

    def refused_and_dropped(call, text):
        dc.set_reference(ref)
        _refused(call, text)
        assert dc.reference_count() == 0

    cfg = capi.DenseAlignConfig()
    lib.dmsa_default_dense_align_config(C.byref(cfg))
    cfg.max_distance = REACH
    for n, stride, text in ((50, 2, b"stride_floats must be at least 3"), (2**26 + 1, 3, b"more than 2^26 reference rows"), (0, 3, b"less than one row"), (-1, 3, b"less than one row")):
        dc.set_reference(ref)
        assert lib.dmsa_dense_cloud_align_reference(handle, capi.ptr(ref, C.c_float), n, stride, None, C.byref(cfg), None, None) == -1
        assert text in lib.dmsa_last_error(opt._ctx) and dc.reference_count() == 0
    assert lib.dmsa_dense_cloud_align_reference(handle, None, 5, 3, None, C.byref(cfg), None, None) == -1
    assert lib.dmsa_dense_cloud_align_reference(handle, capi.ptr(ref, C.c_float), 50, 3, None, None, None, None) == -1
    T = np.eye(4)[:3].copy()
    T[2, 0] = np.nan
    refused_and_dropped(lambda: dc.align_reference(ref, transform=T, max_distance=REACH), "the transform is not finite")
    for reach, text in ((np.nan, "max_distance is not finite"), (np.inf, "max_distance is not finite"), (0.04, "max_distance must lie in [voxel_size, 64 * voxel_size]"),
                        (3.3, "max_distance must lie in [voxel_size, 64 * voxel_size]")):
        refused_and_dropped(lambda: dc.align_reference(ref, max_distance=reach), text)
        dc.set_reference(ref)
        _refused(lambda: dc.align_sums(reach), text)
    for kw, text in ((dict(max_iterations=0), "max_iterations must lie in [1, 64]"), (dict(max_iterations=65), "max_iterations must lie in [1, 64]"),
                     (dict(min_pairs=2), "min_pairs must be at least 3"), (dict(stop_translation=-1e-9), "stop_translation must be finite and >= 0"),
                     (dict(stop_translation=np.nan), "stop_translation must be finite and >= 0"), (dict(stop_rotation=np.inf), "stop_rotation must be finite and >= 0"),
                     (dict(stop_rotation=-1.0), "stop_rotation must be finite and >= 0")):
        refused_and_dropped(lambda: dc.align_reference(ref, max_distance=REACH, **kw), text)
    with pytest.raises(ValueError):
        dc.align_reference(ref[:, :2])
    # the limits themselves are legal
    got = dc.align_reference(ref, max_distance=REACH, max_iterations=64, min_pairs=3, stop_translation=0.0, stop_rotation=0.0)
    assert got["iterations"] >= 1 and dc.reference_count() == 50
    dc.close()


# ---- 6. the programs ------------------------------------------------------------------------------------------------------------------------------------
def test_the_cpp_example_aligns_a_displaced_copy_of_the_file_it_wrote_a_moment_earlier(tmp_path):
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
    args = [exe, r["dump"], r["poses_file"], "ouster", "OUT", "--voxel", "0.1", "--min-range", "0.5", "--compare", str(displaced)]
    precision = lambda text: float(re.search(r"^compare: .*\bprecision ([0-9.]+)", text, re.M).group(1))
    before = subprocess.run([str(tmp_path / "a.pcd") if a == "OUT" else a for a in args], capture_output=True, text=True, timeout=300)
    assert before.returncode == 0 and "align:" not in before.stdout, before.stdout[-1000:] + before.stderr[-1000:]
    p = subprocess.run([str(tmp_path / "b.pcd") if a == "OUT" else a for a in args] + ["--align", "--align-out", str(t_out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
    lines = re.findall(r"^align: iteration (\d+)  matched (\d+) ", p.stdout, re.M)
    stop = re.search(r"^align: .*stop ([A-Z_]+) after (\d+) iterations$", p.stdout, re.M)
    assert stop and int(stop.group(2)) == len(lines) >= 2 and stop.group(1) in ("CONVERGED", "MAX_ITERATIONS") and [int(k) for k, _ in lines] == list(range(len(lines)))
    T = dcl.read_transform(t_out)
    assert np.abs(T - dense_cloud_demo.inverse_motion(applied)).max() < 0.05  # (it found its way back: the figures are the model's business)
    assert precision(p.stdout) >= precision(before.stdout) and precision(p.stdout) > 0.9
    assert open(tmp_path / "a.pcd", "rb").read() == open(tmp_path / "b.pcd", "rb").read() == open(r["pcd"], "rb").read()
    # the transform it wrote is one it reads: the comparison alone gives the aligned figures
    again = subprocess.run([str(tmp_path / "c.pcd") if a == "OUT" else a for a in args] + ["--compare-transform", str(t_out)], capture_output=True, text=True, timeout=300)
    assert again.returncode == 0 and re.search(r"^compare: .*$", again.stdout, re.M).group(0) == re.search(r"^compare: .*$", p.stdout, re.M).group(0)


def test_the_demo_aligns_a_displaced_reference(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import dense_cloud_demo

    r = dense_cloud_demo.run(scans=6, workdir=str(tmp_path))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dense_cloud_demo.py"), "--scans", "6", "--compare", r["pcd"], "--align", "--compare-displace", "1.0,0.08",
                        "--compare-out", str(tmp_path / "Dist.pcd"), "--out", str(tmp_path / "Dense2.pcd")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert re.search(r"^align: stop (CONVERGED|MAX_ITERATIONS) after \d+ iterations$", p.stdout, re.M) and "align recovered: " in p.stdout and "align inverse of the applied: " in p.stdout
    assert float(re.search(r"^align: largest entry difference ([0-9.e+-]+)$", p.stdout, re.M).group(1)) < 0.05
    assert float(re.search(r"^compare .*\bprecision ([0-9.]+)", p.stdout, re.M).group(1)) > 0.9
