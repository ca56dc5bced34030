"""CPU-side checks of include/dmsa_dense_cloud.h: the TUM parser against dmsa_format_tum_pose, the symbol list, the binary PCD header, and the
numpy model of the rules (tests/dense_cloud_model.py, the yardstick of the GPU tests) against scipy's Slerp."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot
from scipy.spatial.transform import Slerp

from dmsa_lidar_slam_amd import _capi as capi
from dmsa_lidar_slam_amd import dense_cloud as dcl
from dmsa_lidar_slam_amd import wire_formats as wf

import dense_cloud_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


# ---- symbols ----------------------------------------------------------------------------------------------------------------------------
def test_symbol_tuple_equals_the_header_and_the_library_exports_it(lib):
    header = open(os.path.join(ROOT, "include", "dmsa_dense_cloud.h")).read()
    declared = set(re.findall(r"\b(dmsa_[a-z_0-9]+)\s*\(", header))
    assert len(declared) == 13
    assert declared == set(capi.DENSE_CLOUD_SYMBOLS) and len(capi.DENSE_CLOUD_SYMBOLS) == len(declared)
    assert not declared & set(capi.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name


def test_struct_layouts_and_default_config(lib):
    assert C.sizeof(capi.DenseConfig) == 96 and C.sizeof(capi.DenseStats) == 64
    assert capi.DenseConfig.time_offset.offset == 72 and capi.DenseConfig.voxel_size.offset == 88
    c = capi.DenseConfig()
    C.memset(C.byref(c), 0x5A, C.sizeof(c))
    lib.dmsa_default_dense_config(C.byref(c))
    assert np.array_equal(np.array(c.lidar_to_imu[:]).reshape(4, 4), np.eye(4))
    assert (c.min_range, c.max_range, c.time_offset, c.max_pose_gap, c.voxel_size) == (0.0, 0.0, 0.0, 0.0, 0.0)


# ---- the parser --------------------------------------------------------------------------------------------------------------------------
def test_parser_round_trips_format_tum_pose():
    rng = np.random.default_rng(5)
    n = 40
    stamps = 1.6e9 + np.cumsum(rng.uniform(0.05, 0.2, n))
    pos, orient = rng.normal(0, 30, (n, 3)), rng.normal(0, 0.9, (n, 3))
    orient[3] = 0.0
    lines = [wf.addPoseToFile(stamps[k], pos[k], orient[k]) for k in range(n)]
    text = "# stamp tx ty tz qx qy qz qw\n\n" + "".join(lines[:20]) + "   \r\n\t# a comment\n" + "".join(ln.replace("\n", "\r\n") for ln in lines[20:])
    s, p, q = dcl.parse_tum_poses(text)
    assert s.shape == (n,) and p.shape == (n, 3) and q.shape == (n, 4)
    # the parsed numbers are the printed ones, exactly: strtod of "%.6f" / "%.5f" text
    for k in range(n):
        assert [float(v) for v in lines[k].split()] == [s[k], *p[k], *q[k]]
    # and they are the poses to the precision of the format
    assert np.abs(s - stamps).max() <= 0.5e-6 * 1.0000001 and np.abs(p - pos).max() <= 0.5e-5 * 1.0000001
    d = (Rot.from_quat(q) * Rot.from_rotvec(orient).inv()).magnitude()
    assert d.max() < 5e-6
    # the same text without a final newline, and as bytes
    s2, _, q2 = dcl.parse_tum_poses(text.rstrip("\n").encode())
    assert np.array_equal(s, s2) and np.array_equal(q, q2)
    e, _, _ = dcl.parse_tum_poses("")
    assert e.shape == (0,)


@pytest.mark.parametrize("bad,line_no", [
    ("1.0 0 0 0 0 0 0 1\n2.0 0 0 0 0 0 0\n", 2),                       # seven numbers
    ("# head\n\n1.0 0 0 0 0 0 0 1\n\n2.0 0 0 0 0 0 0 1 9\n", 5),        # nine numbers; blank and # lines count as lines
    ("1.0 0 0 0 0 0 0 1\r\n2.0 0 0 0 x 0 0 1\r\n", 2),                  # not a number
    ("1.0 0 0 0 0 0 0 1x\n", 1),                                        # a number with a tail
    ("1.0 0 0 0 0 0 0 1\n2.0 0 0 0 0 0 0 1\n3.0,0,0,0,0,0,0,1\n", 3),   # commas
    ("1.0 0 0 0 0 0 0 1\n" + "1 " * 600 + "\n", 2),                     # longer than the line buffer
])
def test_parser_reports_the_line_of_a_malformed_pose(lib, bad, line_no):
    with pytest.raises(ValueError, match=rf"^line {line_no}: "):
        dcl.parse_tum_poses(bad)
    raw = bad.encode()
    st, ps, qs = np.zeros(8), np.zeros((8, 3)), np.zeros((8, 4))
    n, err = C.c_int64(-1), C.create_string_buffer(64)
    rc = lib.dmsa_parse_tum_poses(raw, len(raw), capi.ptr(st, C.c_double), capi.ptr(ps, C.c_double), capi.ptr(qs, C.c_double), 8, C.byref(n), err, 64)
    assert rc == capi.DMSA_ERR_INVALID and err.value.decode().startswith(f"line {line_no}: ")
    assert n.value == sum(1 for ln in bad.split("\n")[: line_no - 1] if ln.strip() and not ln.strip().startswith("#"))  # the poses before it


def test_parser_capacity_and_arguments(lib):
    raw = b"1 0 0 0 0 0 0 1\n2 1 2 3 0 0 1 0\n3 0 0 0 0 0 0 1"
    st, ps, qs = np.zeros(2), np.zeros((2, 3)), np.zeros((2, 4))
    n = C.c_int64(0)
    args = (capi.ptr(st, C.c_double), capi.ptr(ps, C.c_double), capi.ptr(qs, C.c_double))
    assert lib.dmsa_parse_tum_poses(raw, len(raw), *args, 2, C.byref(n), None, 0) == capi.DMSA_ERR_INVALID and n.value == 3  # the count is still told
    assert np.array_equal(st, [1.0, 2.0]) and np.array_equal(ps[1], [1, 2, 3]) and np.array_equal(qs[1], [0, 0, 1, 0])
    assert lib.dmsa_parse_tum_poses(raw, len(raw) - 16, *args, 2, C.byref(n), None, 0) == capi.DMSA_OK and n.value == 2  # `bytes` bounds the text
    assert lib.dmsa_parse_tum_poses(raw, len(raw), *args, 2, None, None, 0) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_parse_tum_poses(None, 5, *args, 2, C.byref(n), None, 0) == capi.DMSA_ERR_INVALID
    err = C.create_string_buffer(8)  # an error text longer than its buffer is cut, with its terminating zero
    assert lib.dmsa_parse_tum_poses(b"x\n", 2, *args, 2, C.byref(n), err, 8) == capi.DMSA_ERR_INVALID and err.raw[:8] == b"line 1:\0"


# ---- the file header ---------------------------------------------------------------------------------------------------------------------
def test_binary_header_is_its_stated_text(lib):
    want = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH 000000012345\nHEIGHT 1\n"
            "VIEWPOINT 0 0 0 1 0 0 0\nPOINTS 000000012345\nDATA binary\n")
    assert dcl.pcdHeaderXyzBinary(12345) == want
    # the counts have a fixed width: every header has the same length, so close can patch them in place
    assert {len(dcl.pcdHeaderXyzBinary(n)) for n in (0, 1, 999_999_999_999)} == {len(want)}
    buf = C.create_string_buffer(512)
    assert lib.dmsa_pcd_header_xyz_binary(10**12, buf, 512) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_pcd_header_xyz_binary(-1, buf, 512) == capi.DMSA_ERR_INVALID
    assert lib.dmsa_pcd_header_xyz_binary(5, buf, len(want)) == capi.DMSA_ERR_INVALID  # no room for the terminating zero
    assert lib.dmsa_pcd_header_xyz_binary(5, buf, len(want) + 1) == len(want)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def _trajectory(rng, n_p, max_step_rad):
    """Rotations whose neighbours differ by at most max_step_rad, so that the model and scipy take the same arc."""
    rots = [Rot.from_rotvec(rng.normal(size=3))]
    for _ in range(n_p - 1):
        axis = rng.normal(size=3)
        rots.append(rots[-1] * Rot.from_rotvec(axis / np.linalg.norm(axis) * rng.uniform(0.0, max_step_rad)))
    quat = np.stack([r.as_quat() for r in rots])
    quat[::2] *= -1.0  # q and -q are the same rotation: the d < 0 branch
    return np.cumsum(rng.uniform(0.05, 0.15, n_p)), rng.normal(0, 5, (n_p, 3)), quat * rng.uniform(0.5, 2.0, (n_p, 1))


@pytest.mark.parametrize("seed", range(4))
def test_model_agrees_with_scipy_slerp(seed):
    rng = np.random.default_rng(seed)
    s, p, q = _trajectory(rng, 8, 2.5)
    q[5] = q[4] * 3.0  # identical neighbours: the linear branch
    m = dm.DenseModel(s, p, q)
    t = np.concatenate([rng.uniform(s[0], s[-1], 400), s, 0.5 * (s[:-1] + s[1:])])
    pose, seg = m.interpolate(t)
    assert np.array_equal(seg, np.clip(np.searchsorted(s, t, side="right") - 1, 0, 6))
    ref = Slerp(s, Rot.from_quat(q))(t)
    angle = (Rot.from_matrix(pose[:, :9].reshape(-1, 3, 3)) * ref.inv()).magnitude()
    print("max rotation angle between the model and scipy:", angle.max())
    assert angle.max() < 1e-12  # the project's slerp-vs-scipy bar (tests/test_oracle_math.py)
    u = (t - s[seg]) / (s[seg + 1] - s[seg])
    assert np.array_equal(pose[:, 9:], p[seg] + u[:, None] * (p[seg + 1] - p[seg]))
    assert np.abs(pose[:, 9:] - np.stack([np.interp(t, s, p[:, a]) for a in range(3)], axis=1)).max() < 1e-12


def test_model_rules_on_a_hand_made_scan():
    s, p = np.array([0.0, 1.0, 2.0, 5.0]), np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [5, 0, 0]], float)
    q = np.tile([0, 0, 0, 1.0], (4, 1))
    m = dm.DenseModel(s, p, q, min_range=1.0, max_range=10.0, max_pose_gap=2.0, voxel_size=0.5)
    xyz = np.array([[2, 0, 0], [np.nan, 0, 0], [1, 0, 0], [10, 0, 0], [2, 0, 0], [2, 0, 0], [2.1, 0, 0], [-2.25, 0, 0], [3, 0, 0]], np.float32)
    t = np.array([0.5, 0.5, 0.5, 0.5, -0.1, 3.0, 0.5, 0.5, np.inf])
    g, st = m.add_scan(xyz, t)
    #        kept  nan   r == min  r == max  before  in gap  same voxel as point 0   kept (cell -4)   inf stamp
    assert st == dict(points_in=9, kept=2, non_finite=2, out_of_range=2, out_of_time=1, in_gap=1, out_of_grid=0, thinned=1)
    assert np.array_equal(g, np.array([[2.5, 0, 0, 1], [-1.75, 0, 0, 1]], np.float32))
    g2, st2 = m.add_scan(xyz[[0, 7]], t[[0, 7]])  # both voxels are taken by the first scan
    assert st2["thinned"] == 2 and g2.shape == (0, 4) and m.total["kept"] == 2 and m.total["points_in"] == 11
