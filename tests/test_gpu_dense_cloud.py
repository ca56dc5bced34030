"""GPU tests of include/dmsa_dense_cloud.h against the numpy model of its rules (tests/dense_cloud_model.py).

Poses: the stage call dmsa_dense_cloud_interpolate against the model -- segments exact, translations bit for bit (the same three fp64
operations), rotations to 1e-12 rad (the project's slerp bar; the model runs numpy's trigonometry, the device include/dmsa_detmath.h).
Points: the model is fed the DEVICE's poses (cast to float, as rule 5 does), so kept coordinates, order and statistics must be equal bit
for bit -- what is compared is everything but the fp64 trigonometry."""
import os
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import dense_cloud_model as dm
import wire_util

pytestmark = pytest.mark.gpu

f32 = np.float32
T0 = 1.6e9 + 12.0   # the stamps of a real recording: 2.4e-7 s to the next double
MAX_GAP = 0.25


@pytest.fixture(scope="module")
def opt():
    from dmsa_lidar_slam_amd.api import DmsaOptimizer

    o = DmsaOptimizer(device=0)
    yield o
    o.close()


def _trajectory():
    """Eight poses.  Segment 0 is exactly MAX_GAP long (kept: the gate is `>`), segment 1 one step of the stamps longer (a gap); q_3 is
    -q_2 perturbed (d < 0); poses 4 and 5 have the same quaternion (the ad >= 1 - eps branch)."""
    step = np.spacing(T0)
    s = T0 + np.array([0.0, 0.25, 0.5, 0.625, 0.75, 0.8125, 0.875, 1.0])
    s[2] += step
    assert s[1] - s[0] == MAX_GAP and s[2] - s[1] == MAX_GAP + step
    rng = np.random.default_rng(11)
    rots = [Rot.from_rotvec(rng.normal(size=3))]
    for _ in range(7):
        rots.append(rots[-1] * Rot.from_rotvec(rng.normal(size=3) * 0.4))
    q = np.stack([r.as_quat() for r in rots])
    q[3] = -(Rot.from_quat(q[2]) * Rot.from_rotvec([1e-3, -2e-3, 5e-4])).as_quat()
    q[4] = q[5] = np.array([0.6, 0.0, 0.0, 0.8])
    q[6] *= 1.7  # normalised by the library
    p = np.cumsum(rng.normal(0, 0.4, (8, 3)), axis=0) + np.array([100.0, -50.0, 3.0])
    return s, p, q


S, P, Q = _trajectory()
L2I = np.eye(4, dtype=f32)
L2I[:3, :3] = Rot.from_rotvec([0.02, -0.01, 1.2]).as_matrix().astype(f32)
L2I[:3, 3] = [0.05, -0.11, 0.2]
GATES = dict(min_range=1.5, max_range=40.0, time_offset=0.01, max_pose_gap=MAX_GAP)


def _creator(opt, s=S, p=P, q=Q, lidar_to_imu=None, min_range=0.0, max_range=0.0, time_offset=0.0, max_pose_gap=0.0, voxel_size=0.0):
    from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator

    cfg = DenseCloudConfig(lidarToImu=np.eye(4, dtype=f32) if lidar_to_imu is None else lidar_to_imu, minRange=min_range, maxRange=max_range,
                           timeOffset=time_offset, maxPoseGap=max_pose_gap, voxelSize=voxel_size)
    model = dm.DenseModel(s, p, q, lidar_to_imu, min_range, max_range, time_offset, max_pose_gap, voxel_size)
    return DenseCloudCreator(s, p, q, cfg, optimizer=opt), model


# ---- 1. poses ---------------------------------------------------------------------------------------------------------------------------
def test_interpolate_matches_the_model(opt):
    dc, model = _creator(opt, max_pose_gap=MAX_GAP)
    rng = np.random.default_rng(1)
    t = np.concatenate([S, [S[0], S[-1]], [np.nextafter(S[0], -np.inf), np.nextafter(S[-1], np.inf)], np.nextafter(S, np.inf), np.nextafter(S[1:], -np.inf),
                        rng.uniform(S[0] - 0.05, S[-1] + 0.05, 3000), [np.nan, np.inf, -np.inf, 0.0]])
    pose, seg = dc.interpolate(t)
    ref, ref_seg = model.interpolate(t)
    dc.close()
    assert np.array_equal(seg, ref_seg)
    # the cases the list above is there for
    assert list(seg[:8]) == [0, -2, 2, 3, 4, 5, 6, 6] and list(seg[8:12]) == [0, 6, -1, -1]   # on every stamp; u = 1 at the last; one ulp outside
    assert set(seg[(t > S[0]) & (t < S[1])]) == {0} and set(seg[(t >= S[1]) & (t < S[2])]) == {-2}      # a gap at / just above max_pose_gap
    assert list(seg[-4:]) == [-1, -1, -1, -1]
    assert np.array_equal(pose[seg < 0], np.zeros(((seg < 0).sum(), 12)))
    ok = seg >= 0
    assert np.array_equal(pose[ok, 9:], ref[ok, 9:])  # tr = p_j + u * (p_{j+1} - p_j): the same three operations
    angle = (Rot.from_matrix(pose[ok, :9].reshape(-1, 3, 3)) * Rot.from_matrix(ref[ok, :9].reshape(-1, 3, 3)).inv()).magnitude()
    print("max rotation angle device vs model [rad]:", angle.max(), " per segment:", [float(angle[seg[ok] == j].max()) for j in (0, 2, 3, 4, 5, 6)])
    assert angle.max() < 1e-12
    R = pose[ok, :9].reshape(-1, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-13
    # on a pose stamp the pose is that pose
    on = Rot.from_matrix(pose[[0, 2, 3, 4, 5, 6, 9], :9].reshape(-1, 3, 3)) * Rot.from_quat(Q[[0, 2, 3, 4, 5, 6, 7]]).inv()
    assert on.magnitude().max() < 1e-12 and np.array_equal(pose[[0, 2, 3], 9:], P[[0, 2, 3]])  # u = 0: p_j + 0 * d


def test_create_refuses_bad_trajectories(opt):
    from dmsa_lidar_slam_amd.api import DmsaError

    bad_q, bad_q2, bad_s = Q.copy(), Q.copy(), S.copy()
    bad_q[3] = 0.0
    bad_q2[1, 2] = np.nan
    bad_s[4] = bad_s[3]
    from dmsa_lidar_slam_amd.dense_cloud import DenseCloudCreator

    for s, p, q in ((S, P, bad_q), (S, P, bad_q2), (bad_s, P, Q), (S[:1], P[:1], Q[:1])):
        with pytest.raises(DmsaError) as e:
            DenseCloudCreator(s, p, q, optimizer=opt)
        assert e.value.args[0].startswith("dmsa_dense_cloud_create failed with -1")


# ---- 2. points, bit for bit ----------------------------------------------------------------------------------------------------------------
def _scan(n, seed, ordered=True):
    """A scan over the whole trajectory and a little more, with every kind of point the rules name."""
    rng = np.random.default_rng(seed)
    xyz = np.zeros((n, 4), f32)
    xyz[:, :3] = rng.normal(0, 12, (n, 3))
    t = rng.uniform(S[0] - 0.03, S[-1] + 0.01, n)
    if ordered:
        t = np.sort(t)
    if n >= 255:
        k = rng.choice(n, 40, replace=False)
        xyz[k[0:3], 0], xyz[k[3:6], 1], xyz[k[6:9], 2] = [np.nan, np.inf, -np.inf], np.nan, np.inf
        t[k[9:12]] = [np.nan, np.inf, -np.inf]
        xyz[k[12:14], :3], xyz[k[14:16], :3] = [1.5, 0, 0], [0, 0, -40.0]                 # exactly min_range / max_range: dropped
        xyz[k[16:18], :3], xyz[k[18:20], :3] = [np.nextafter(f32(1.5), f32(2)), 0, 0], [0, np.nextafter(f32(40), f32(0)), 0]  # one ulp inside: kept
        t[k[20:23]] = [S[0] - 0.01, S[-1] - 0.01, np.nextafter(S[-1] - 0.01, np.inf)]       # first stamp, last stamp, one ulp late (time_offset = 0.01)
        t[k[23:26]] = S[3:6] - 0.01
        xyz[k[26], :3] = 1e30                                                              # finite, overflows in rule 2: r = inf
    return xyz, t


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65537])
def test_add_scan_equals_the_model_on_the_device_poses(opt, n):
    dc, model = _creator(opt, lidar_to_imu=L2I, **GATES)
    xyz, t = _scan(n, 100 + n)
    if n == 1:
        xyz[0, :3], t[0] = [3.0, -4.0, 1.0], S[5] + 0.02
    kept, st = dc.add_scan(xyz, t)
    ref, ref_st = model.add_scan(xyz, t, interpolate=dc.interpolate)
    assert st == ref_st, (st, ref_st)
    assert kept.dtype == f32 and kept.shape == ref.shape and np.array_equal(kept.view(np.uint32), ref.view(np.uint32))
    if n >= 255:
        assert min(st[k] for k in ("kept", "non_finite", "out_of_range", "out_of_time", "in_gap")) > 0 and st["out_of_grid"] == st["thinned"] == 0
    if n == 1:
        assert st["kept"] == 1
    # a second scan: the counters add up, and without a voxel size no scan knows of another
    kept2, st2 = dc.add_scan(xyz, t)
    assert np.array_equal(kept2, kept) and st2 == st and dc.stats() == {k: 2 * v for k, v in st.items()}
    dc.close()


def test_unordered_stamps_leave_the_lds_range_and_change_nothing(opt):
    """256 points of a workgroup that span all seven segments (more than the five poses a workgroup stages): the global search."""
    dc, model = _creator(opt, lidar_to_imu=L2I, **GATES)
    xyz, t = _scan(700, 7, ordered=False)
    kept, st = dc.add_scan(xyz, t)
    ref, ref_st = model.add_scan(xyz, t, interpolate=dc.interpolate)
    assert st == ref_st and np.array_equal(kept.view(np.uint32), ref.view(np.uint32)) and st["kept"] > 300
    # the same points in stamp order go through the LDS copies and come out with the same bits (a point's result does not depend on its neighbours)
    order = np.argsort(t, kind="stable")
    kept_o, st_o = dc.add_scan(xyz[order], t[order])
    assert st_o == st

    def sorted_rows(a):
        u = a.view(np.uint32)
        return u[np.lexsort(u.T)]

    assert np.array_equal(sorted_rows(kept_o), sorted_rows(kept))
    dc.close()


def test_a_scan_with_every_point_dropped(opt):
    dc, model = _creator(opt, lidar_to_imu=L2I, **GATES)
    xyz, t = _scan(300, 3)
    t = t + 10.0
    kept, st = dc.add_scan(xyz, t)
    assert kept.shape == (0, 4) and st["kept"] == 0 and st == model.add_scan(xyz, t)[1] and st["out_of_time"] > 250
    dc.close()


# ---- 3. thinning ----------------------------------------------------------------------------------------------------------------------------
def _still_trajectory():
    """The identity pose throughout: g = the point itself, bit for bit, so voxels can be constructed by hand."""
    return S, np.zeros((8, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (8, 1))


def _voxel_scans():
    rng = np.random.default_rng(21)
    scans = []
    for k in range(3):
        n = 3000 + 1000 * k  # (growing, so that the table has to grow before every scan)
        xyz = np.zeros((n, 4), f32)
        xyz[:, :3] = rng.uniform(-40, 40, (n, 3))
        xyz[:200, :3] = rng.uniform(-0.5, 0.0, (200, 3))            # cell -1 on every axis (truncation would say 0): one survivor in all three scans
        xyz[200:400, :3] = rng.uniform(-3, 3, (200, 3))             # crowded: shared voxels within the scan
        if k:
            xyz[400:900] = scans[0][0][400:900]                      # voxels an earlier scan holds
            xyz[400:900, :3] += f32(1e-3)
        xyz[900:906, :3] = [[524288.0, 1, 1], [524287.75, 1, 1], [-524288.0, 1, 1], [-524288.5, 1, 1], [1, 1, 2.0 ** 30], [1, -524287.75, 1]]
        scans.append((xyz, np.sort(rng.uniform(S[0], S[-1], n))))
    return scans


def _run_voxel_scans(opt, reserve=0):
    s, p, q = _still_trajectory()
    dc, model = _creator(opt, s, p, q, voxel_size=0.5)
    if reserve:
        dc.reserve(reserve)
    out, slots = [], []
    for xyz, t in _voxel_scans():
        kept, st = dc.add_scan(xyz, t)
        out.append((kept, st))
        slots.append(dc.table_info())
    total = dc.stats()
    dc.close()
    return out, slots, total, model


def test_thinning_equals_the_model_and_is_repeatable_whatever_the_table_size(opt):
    out, slots, total, model = _run_voxel_scans(opt)
    for (kept, st), (xyz, t) in zip(out, _voxel_scans()):
        ref, ref_st = model.add_scan(xyz, t)  # (its own poses: the identity either way)
        assert st == ref_st, (st, ref_st)
        assert np.array_equal(kept.view(np.uint32), ref.view(np.uint32))
    assert total == model.total
    st0, st1 = out[0][1], out[1][1]
    assert st0["out_of_grid"] == 3 and st0["thinned"] >= 199 and st1["thinned"] >= 600 and st1["kept"] > 1500
    # +-2^20: the cells 2^20 - 1 and -2^20 are in the grid, 2^20 and -2^20 - 1 are not
    k0 = out[0][0]
    assert (k0[:, 0] == f32(524287.75)).sum() == 1 and (k0[:, 0] == f32(-524288.0)).sum() == 1 and (k0[:, 1] == f32(-524287.75)).sum() == 1
    assert not (np.abs(k0[:, :3]) == f32(524288.5)).any() and not (k0[:, 0] == f32(524288.0)).any()
    # the table was never more than half full, and it had to grow between the scans
    assert all(2 * occ <= sl for sl, occ in slots) and [occ for _, occ in slots] == list(np.cumsum([st["kept"] for _, st in out]))
    assert slots[0][0] < slots[1][0] < slots[2][0]
    # the same input again: identical bytes
    again, slots2, total2, _ = _run_voxel_scans(opt)
    assert slots2 == slots and total2 == total
    assert all(a[0].tobytes() == b[0].tobytes() and a[1] == b[1] for a, b in zip(out, again))
    # a table that is large from the start never grows and gives the same result
    big, slots3, total3, _ = _run_voxel_scans(opt, reserve=1 << 18)
    assert slots3[0][0] == slots3[2][0] == 1 << 19 and total3 == total
    assert all(a[0].tobytes() == b[0].tobytes() and a[1] == b[1] for a, b in zip(out, big))


# ---- 4. decode fused with the placement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sensor", ["ouster", "hesai", "velodyne"])
def test_add_pointcloud2_equals_decode_then_add_scan(opt, sensor):
    from dmsa_lidar_slam_amd import wire_formats as wf

    args = dict(lidar_to_imu=L2I, min_range=1.5, max_range=60.0, voxel_size=0.5)
    a, _ = _creator(opt, **args)
    b, _ = _creator(opt, **args)
    dec = wf.PointCloud2Decoder(sensor)
    for k in range(2):
        msg, _ = wire_util.make_msg(sensor, 5000 + k, seed=k, stamp=T0 + 0.3 + 0.12 * k)
        xyz, st, _ = dec.decode(msg)
        kept_a, st_a = a.add_scan(xyz, st)
        kept_b, st_b = b.add_pointcloud2(msg, sensor)
        assert st_a == st_b and st_a["kept"] > 1000
        assert kept_a.tobytes() == kept_b.tobytes()
    assert a.stats() == b.stats() and a.table_info() == b.table_info()
    empty, _ = wire_util.make_msg(sensor, 0)
    assert b.add_pointcloud2(empty, sensor)[1]["points_in"] == 0
    bad, _ = wire_util.make_msg(sensor, 16)
    bad.field_offsets = bad.field_offsets[:2]  # the decoder's own checks, the decoder's own status
    from dmsa_lidar_slam_amd.api import DmsaError
    with pytest.raises(DmsaError) as e:
        b.add_pointcloud2(bad, sensor)
    assert e.value.status == -1
    dec.close(), a.close(), b.close()


# ---- 5. the file -------------------------------------------------------------------------------------------------------------------------------
def _read_pcd(path):
    raw = open(path, "rb").read()
    end = raw.index(b"DATA binary\n") + len(b"DATA binary\n")
    head = dict(line.split(" ", 1) for line in raw[:end].decode().splitlines()[1:])
    return head, np.frombuffer(raw[end:], "<f4").reshape(-1, 3), len(raw)


def test_three_scans_to_a_pcd(opt, tmp_path):
    from dmsa_lidar_slam_amd.api import DmsaError
    from dmsa_lidar_slam_amd.dense_cloud import pcdHeaderXyzBinary

    dc, _ = _creator(opt, lidar_to_imu=L2I, voxel_size=0.25, **GATES)
    path = tmp_path / "DenseCloud.pcd"
    dc.open_pcd(path)
    with pytest.raises(DmsaError):
        dc.open_pcd(tmp_path / "second.pcd")  # one file at a time
    kept = [dc.add_scan(*_scan(n, 40 + n))[0] for n in (3000, 1, 5000)]
    kept.append(dc.add_scan(*_scan(400, 1), download=False)[0])  # survivors that go to the file only
    assert kept.pop() is None and dc.lastKept > 0
    extra = dc.lastKept
    points, size = dc.close_pcd()
    rows = np.concatenate(kept)[:, :3]
    head, body, file_size = _read_pcd(path)
    assert points == rows.shape[0] + extra and size == file_size == len(pcdHeaderXyzBinary(0)) + 12 * points
    assert open(path, "rb").read().startswith(pcdHeaderXyzBinary(points).encode())  # the counts are patched in
    assert head["WIDTH"] == head["POINTS"] == "%012d" % points and head["FIELDS"] == "x y z" and head["HEIGHT"] == "1" and head["DATA"] == "binary"
    assert body.shape == (points, 3) and np.array_equal(body[: rows.shape[0]].view(np.uint32), rows.view(np.uint32))
    # closing with zero points leaves no file
    empty = tmp_path / "Empty.pcd"
    dc.open_pcd(empty)
    dc.add_scan(*[a + 10.0 if a.ndim == 1 else a for a in _scan(300, 3)])  # every point out of time
    assert os.path.exists(empty)
    with pytest.raises(DmsaError) as e:
        dc.close_pcd()
    assert e.value.status == -1 and not os.path.exists(empty)
    # a path that cannot be opened
    with pytest.raises(DmsaError) as e:
        dc.open_pcd(tmp_path / "no_such_directory" / "x.pcd")
    assert e.value.status < 0 and "no_such_directory" in e.value.args[0]
    with pytest.raises(DmsaError):
        dc.close_pcd()  # nothing is open
    dc.close()


# ---- 6. capacity too small ------------------------------------------------------------------------------------------------------------------------
def test_capacity_too_small_leaves_the_object_as_it_was(opt):
    from dmsa_lidar_slam_amd.api import DmsaError

    args = dict(lidar_to_imu=L2I, voxel_size=0.5, **GATES)
    dc, _ = _creator(opt, **args)
    fresh, _ = _creator(opt, **args)
    first, second = _scan(2000, 61), _scan(2500, 62)
    second[0][:300] = first[0][:300]  # voxels the first scan holds: the second scan's result depends on the set
    second[1][:300] = first[1][:300]
    dc.add_scan(*first), fresh.add_scan(*first)
    want, want_st = fresh.add_scan(*second)
    before = (dc.table_info()[1], dc.stats())  # (the table itself may grow before the scan is launched: more room, the same set)
    with pytest.raises(DmsaError) as e:
        dc.add_scan(*second, capacity=want.shape[0] - 1)
    assert e.value.status == -1 and dc.lastKept == want.shape[0] and dc.lastStats == want_st  # the count is still told
    assert (dc.table_info()[1], dc.stats()) == before
    got, got_st = dc.add_scan(*second, capacity=want.shape[0])  # exactly enough
    assert got_st == want_st and got.tobytes() == want.tobytes() and dc.stats() == fresh.stats() and dc.table_info() == fresh.table_info()
    third = _scan(1500, 63)
    assert dc.add_scan(*third)[0].tobytes() == fresh.add_scan(*third)[0].tobytes()
    dc.close(), fresh.close()


# ---- 7. the examples ------------------------------------------------------------------------------------------------------------------------------
def test_dense_cloud_demo_writes_what_its_statistics_report(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import dense_cloud_demo

    r = dense_cloud_demo.run(scans=8, workdir=str(tmp_path), rings=32, az_steps=256, num_iter=3)
    st = r["stats"]
    assert r["poses"] >= 3 and r["scans"] == 8 and st["points_in"] > 8 * 1000
    assert st["kept"] > 2000 and st["out_of_time"] > 0 and st["thinned"] > 0 and st["points_in"] == sum(v for k, v in st.items() if k != "points_in")
    head, body, size = _read_pcd(r["pcd"])
    assert int(head["POINTS"]) == body.shape[0] == r["points"] == st["kept"] and size == r["bytes"]
    assert np.isfinite(body).all()
