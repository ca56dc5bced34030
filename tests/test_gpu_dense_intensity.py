"""GPU tests of include/dmsa_dense_intensity.h (I1-I7) against tests/dense_intensity_model.py.

The intensity never decides anything (I2), so almost everywhere it is the point's GLOBAL INDEX as a float (exact below 2^24): the w of a
survivor names the input row it came from, and the model of the value is the model's list of surviving indices.  Coordinates, statistics and
every stage result are compared with a twin object without the switch, bit for bit.

Field decode: a packed 43-byte point with one field of each of the eight datatypes at odd offsets, against numpy's astype(float32) of a
structured view.  Files: every byte, header included.

Not tested here: messages beyond 2^32 bytes (refused by the message checks the decoder already had)."""
import os

import numpy as np
import pytest

import dense_carve_model as cm
import dense_intensity_model as im
import dense_normals_model as nm
import dense_outliers_model as om
import test_gpu_dense_cloud as base
import wire_util

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = [0, 1, 255, 256, 257]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def opt():
    from dmsa_lidar_slam_amd.api import DmsaOptimizer

    o = DmsaOptimizer(device=0)
    yield o
    o.close()


@pytest.fixture(scope="module")
def dec():
    from dmsa_lidar_slam_amd import wire_formats as wf

    d = wf.PointCloud2Decoder("unknown")
    yield d
    d.close()


def _pair(opt, s=base.S, p=base.P, q=base.Q, lidar_to_imu=None, retain=False, **gates):
    """(an intensity object, its twin without the switch, the model)"""
    from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator

    cfg = DenseCloudConfig(lidarToImu=np.eye(4, dtype=f32) if lidar_to_imu is None else lidar_to_imu, minRange=gates.get("min_range", 0.0),
                           maxRange=gates.get("max_range", 0.0), timeOffset=gates.get("time_offset", 0.0), maxPoseGap=gates.get("max_pose_gap", 0.0),
                           voxelSize=gates.get("voxel_size", 0.0))
    dc = DenseCloudCreator(s, p, q, cfg, optimizer=opt, retain=retain, intensity=True)
    twin = DenseCloudCreator(s, p, q, cfg, optimizer=opt, retain=retain)
    assert dc.intensity and not twin.intensity
    return dc, twin, im.IntensityModel(s, p, q, lidar_to_imu, **gates)


def _refused(call, text=None, status=-1):
    from dmsa_lidar_slam_amd.api import DmsaError

    with pytest.raises(DmsaError) as e:
        call()
    assert e.value.status == status and (text is None or text in e.value.args[0]), e.value.args[0]


# ---- 1. the field decode (I4) -------------------------------------------------------------------------------------------------------------------
# x y z and one field of each datatype, every one at an odd offset, 43 bytes per point
PACKED = np.dtype({"names": ["x", "y", "z", "i8", "u8", "i16", "u16", "i32", "u32", "f32", "f64"],
                   "formats": ["<f4", "<f4", "<f4", "i1", "u1", "<i2", "<u2", "<i4", "<u4", "<f4", "<f8"],
                   "offsets": [1, 5, 9, 13, 15, 17, 19, 21, 25, 29, 33], "itemsize": 43})
FLT_MAX = float(np.finfo(f32).max)
SPECIAL = {
    "i8": [-128, 127, 0, -1], "u8": [0, 255, 128], "i16": [-32768, 32767, -1], "u16": [0, 65535, 32768],
    "i32": [2**24 + 1, -(2**24 + 1), 2**24 + 3, -(2**24 + 3), 2**31 - 1, -(2**31), 0, 2**31 - 65],
    "u32": [2**24 + 1, 2**24 + 3, 2**32 - 1, 2**31, 2**32 - 128, 2**32 - 129, 0],                # ties go to even both ways
    "f64": [1e39, -1e39, 2.0**-150, -(2.0**-150), 1.5 * 2.0**-149, 2.0**-149, 1.0 + 2.0**-24, 1.0 + 3 * 2.0**-24, np.nextafter(1.0 + 2.0**-24, 2.0),
            FLT_MAX + 2.0**103, np.nextafter(FLT_MAX + 2.0**103, 0.0), np.nan, np.inf, -np.inf, 0.1, 5e-324, -0.0],
}
SPECIAL_F32_BITS = [0x00000001, 0x807FFFFF, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0x7F812345, 0x3F800000]  # denormals, -0, +-inf, NaNs, 1


def _packed_msg(n, seed=0):
    from dmsa_lidar_slam_amd.wire_formats import PointCloud2Msg

    rng = np.random.default_rng(seed)
    rec = np.zeros(n, PACKED)
    for name in ("x", "y", "z"):
        rec[name] = rng.normal(0, 20, n)
    for name in ("i8", "u8", "i16", "u16", "i32", "u32"):
        info = np.iinfo(rec.dtype[name])
        rec[name] = rng.integers(info.min, info.max, n, endpoint=True)
    rec["f64"] = rng.normal(0, 1, n) * 10.0 ** rng.uniform(-50, 45, n)
    bits = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)  # every kind of float32, NaNs among them
    for name, values in SPECIAL.items():
        k = min(n, len(values))
        rec[name][-k:] = values[:k] if n else []
    k = min(n, len(SPECIAL_F32_BITS))
    bits[n - k:] = SPECIAL_F32_BITS[:k]
    rec["f32"] = bits.view(f32)
    assert np.array_equal(rec["f32"].view(np.uint32), bits)
    offsets = np.array([PACKED.fields[name][1] for name in PACKED.names], np.uint32)
    data = np.frombuffer(rec.tobytes(), np.uint8).copy()
    assert data.shape[0] == 43 * n
    return PointCloud2Msg(height=1, width=n, point_step=43, field_offsets=offsets, data=data, stamp=base.T0), rec


@pytest.mark.parametrize("n", SIZES + [4099])
def test_decode_field_equals_numpys_conversion_for_every_datatype(dec, n):
    msg, rec = _packed_msg(n, seed=n)
    for datatype in range(1, 9):
        index = 2 + datatype
        got = dec.decode_field(msg, (index, datatype))
        want = im.field_as_float32(msg.data, n, 43, int(msg.field_offsets[index]), datatype)
        assert got.dtype == f32 and got.shape == (n,)
        with np.errstate(over="ignore", invalid="ignore"):
            assert np.array_equal(want.view(np.uint32), rec[PACKED.names[index]].astype(f32).view(np.uint32), equal_nan=False) or datatype == 7 or n == 0
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (datatype, np.flatnonzero(np.isnan(got) != nan)[:10])
        same = got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]
        assert same.all(), (datatype, [(float(a), float(b)) for a, b in zip(got[~nan][~same][:5], want[~nan][~same][:5])])
        if datatype == 7 and n >= 255:
            assert nan.sum() >= 2 and np.array_equal(got.view(np.uint32)[-8:-3], np.array(SPECIAL_F32_BITS[:5], np.uint32))
    if n >= 255:  # by name as well as by number
        assert np.array_equal(dec.decode_field(msg, (6, "uint16")), rec["u16"].astype(f32))


def test_decode_field_refusals(dec):
    from dmsa_lidar_slam_amd.api import DmsaError

    msg, _ = _packed_msg(16)
    assert dec.decode_field(msg, (10, 8)).shape == (16,)
    for field in ((11, 7), (2**31, 7), (10, 0), (10, 9), (3, 2**32 - 1)):  # index >= num_fields; a datatype outside 1..8
        with pytest.raises(DmsaError):
            dec.decode_field(msg, field)
    # a field that reaches beyond point_step: the same offset is fine for two bytes and refused for four and eight
    msg.field_offsets = np.append(msg.field_offsets, np.uint32(40)).astype(np.uint32)
    assert dec.decode_field(msg, (11, 4)).shape == (16,) and dec.decode_field(msg, (11, 1)).shape == (16,)
    for datatype in (5, 6, 7, 8):
        with pytest.raises(DmsaError):
            dec.decode_field(msg, (11, datatype))
    msg.field_offsets[11] = 2**32 - 1  # (offset + size does not wrap)
    with pytest.raises(DmsaError):
        dec.decode_field(msg, (11, 8))
    # ... and beyond data: one byte short of n points
    short, _ = _packed_msg(16)
    short.data = short.data[:-1]
    with pytest.raises(DmsaError):
        dec.decode_field(short, (3, 1))


# ---- 2. add_scan (I2, I3) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES + [65537])
def test_add_scan_carries_the_index_of_every_survivor(opt, n):
    dc, twin, model = _pair(opt, lidar_to_imu=base.L2I, voxel_size=2.0, **base.GATES)
    xyz, t = base._scan(n, 100 + n)
    if n == 1:
        xyz[0, :3], t[0] = [3.0, -4.0, 1.0], base.S[5] + 0.02
    xyz[:, 3] = np.arange(n, dtype=f32)
    kept, st = dc.add_scan(xyz, t)
    kept_t, st_t = twin.add_scan(xyz, t)
    ref, _, idx, ref_st = model.add_scan_indices(xyz, t, interpolate=dc.interpolate)
    assert st == st_t == ref_st, (st, st_t, ref_st)
    assert kept.shape == kept_t.shape == ref.shape and np.array_equal(_bits(kept[:, :3]), _bits(kept_t[:, :3])) and (kept_t[:, 3] == 1).all()
    assert np.array_equal(_bits(kept), _bits(ref)) and np.array_equal(kept[:, 3], idx.astype(f32))
    if n >= 255:
        assert min(st[k] for k in ("kept", "non_finite", "out_of_range", "out_of_time", "in_gap")) > 0
    if n == 65537:
        assert st["thinned"] > 1000 and idx.max() > 2**15
    if n == 1:
        assert st["kept"] == 1
    assert dc.stats() == twin.stats() and dc.table_info() == twin.table_info()
    dc.close(), twin.close()


def test_first_hit_of_a_voxel_nan_intensity_and_a_capacity_refusal(opt):
    s, p, q = base._still_trajectory()  # the identity pose: g = the point itself
    dc, twin, _ = _pair(opt, s, p, q, retain=True, voxel_size=0.5)
    t = lambda n: np.linspace(s[0] + 0.01, s[-1] - 0.01, n)
    one = np.array([[1.1, 1.1, 1.1, 10.0], [1.2, 1.2, 1.2, 11.0], [3.1, 3.1, 3.1, 0.0], [5.1, 5.1, 5.1, np.inf], [7.1, 7.1, 7.1, -0.0], [1.3, 1.1, 1.4, 12.0],
                    [np.nan, 0.0, 0.0, 13.0]], f32)
    one.view(np.uint32)[2, 3] = 0x7FC00123  # a NaN with a payload
    kept, st = dc.add_scan(one, t(7))
    assert np.array_equal(_bits(kept), _bits(one[[0, 2, 3, 4]]))  # two hits of one voxel inside a scan: the first hit's intensity; the NaN stays
    assert st == twin.add_scan(one, t(7))[1] and (st["kept"], st["thinned"], st["non_finite"]) == (4, 2, 1)  # a NaN intensity enters no counter
    # a capacity refusal enters nothing
    two = np.array([[1.4, 1.2, 1.3, 20.0], [9.1, 9.1, 9.1, 21.0], [11.1, 11.1, 11.1, 22.0], [3.2, 3.2, 3.2, 23.0]], f32)
    before = (dc.table_info()[1], dc.stats(), dc.retained()[0].tobytes())
    _refused(lambda: dc.add_scan(two, t(4), capacity=1), "capacity too small")
    assert dc.lastKept == 2 and (dc.table_info()[1], dc.stats(), dc.retained()[0].tobytes()) == before
    kept2, st2 = dc.add_scan(two, t(4), capacity=2)  # across scans: the voxels of 1.x and 3.x keep the first scan's intensities
    assert np.array_equal(_bits(kept2), _bits(two[[1, 2]])) and st2["thinned"] == 2
    g, o = dc.retained()
    assert np.array_equal(_bits(g), _bits(np.concatenate([one[[0, 2, 3, 4]], two[[1, 2]]]))) and (o[:, 3] == 1).all() and (o[:, :3] == 0).all()
    twin.add_scan(two, t(4))
    assert np.array_equal(_bits(twin.retained()[0][:, :3]), _bits(g[:, :3])) and (twin.retained()[0][:, 3] == 1).all()
    # I1: the switch is legal only before the first scan; twice is fine before it
    _refused(dc.with_intensity, "before the first scan")
    _refused(twin.with_intensity, "before the first scan")
    assert not twin.intensity
    dc.close(), twin.close()


# ---- 3. the fused path (I5) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sensor,field", [("hesai", "auto"), ("ouster", "auto"), ("velodyne", "auto"), ("livoxXYZRTLT_s", "auto"), ("ouster", (5, "uint16"))])
def test_add_pointcloud2_with_a_field_equals_decode_field_decode_add_scan(opt, sensor, field):
    from dmsa_lidar_slam_amd import wire_formats as wf
    from dmsa_lidar_slam_amd.dense_cloud import sensor_intensity_field

    args = dict(lidar_to_imu=base.L2I, min_range=1.5, max_range=60.0, voxel_size=0.5)
    a, twin, _ = _pair(opt, **args)
    b, plain, _ = _pair(opt, **args)
    plain.with_intensity()  # (an intensity object fed by the call without a field)
    d = wf.PointCloud2Decoder(sensor)
    named = sensor_intensity_field(sensor) if field == "auto" else field
    name = [f for f, _ in wire_util.LAYOUTS[sensor] if f not in wire_util._PADS][named[0]]
    assert name in ("intensity", "reflectivity")
    for k in range(2):
        msg, _ = wire_util.make_msg(sensor, 5000 + k, seed=k, stamp=base.T0 + 0.3 + 0.12 * k)
        xyz, st, _ = d.decode(msg)
        w = d.decode_field(msg, named)
        rec = np.frombuffer(msg.data.tobytes(), np.dtype(wire_util.LAYOUTS[sensor]))
        assert np.array_equal(_bits(w), _bits(rec[name].astype(f32))) and len(np.unique(w)) > 50
        rows = xyz.copy()
        assert (_bits(rows[:, 3]) == 0).all()  # the w the decoder writes: +0.0
        rows[:, 3] = w
        kept_a, st_a = a.add_scan(rows, st)
        kept_b, st_b = b.add_pointcloud2(msg, sensor, intensity_field=field)
        kept_t, st_t = twin.add_pointcloud2(msg, sensor)
        kept_p, st_p = plain.add_pointcloud2(msg, sensor)
        assert st_a == st_b == st_t == st_p and st_a["kept"] > 1000
        assert kept_a.tobytes() == kept_b.tobytes()
        assert np.array_equal(_bits(kept_b[:, :3]), _bits(kept_t[:, :3])) and (kept_t[:, 3] == 1).all()
        assert np.array_equal(_bits(kept_p[:, :3]), _bits(kept_t[:, :3])) and (_bits(kept_p[:, 3]) == 0).all()
    assert a.stats() == b.stats() and a.table_info() == b.table_info()
    empty, _ = wire_util.make_msg(sensor, 0)
    assert b.add_pointcloud2(empty, sensor, intensity_field=field)[1]["points_in"] == 0
    # a bad field enters nothing, like a bad stamp field
    before = (b.stats(), b.table_info())
    msg, _ = wire_util.make_msg(sensor, 64, seed=9, stamp=base.T0 + 0.6)
    for bad in ((len(msg.field_offsets), 7), (3, 0), (3, 9)):
        _refused(lambda: b.add_pointcloud2(msg, sensor, intensity_field=bad))
        assert b.lastKept == 0
    assert (b.stats(), b.table_info()) == before
    beyond, _ = wire_util.make_msg(sensor, 64, seed=9, stamp=base.T0 + 0.6)
    beyond.field_offsets[3] = beyond.point_step - 3  # four bytes from here reach beyond point_step
    _refused(lambda: b.add_pointcloud2(beyond, sensor, intensity_field=(3, 7)))
    assert b.add_pointcloud2(beyond, sensor, intensity_field=(3, 3), capacity=0, download=False)[1]["points_in"] == 64 and b.stats() != before[0]  # (two bytes fit)
    # an object without the switch refuses the call, with a named field and with the sensor's own
    _refused(lambda: twin.add_pointcloud2(msg, sensor, intensity_field=named), "carries no intensity")
    _refused(lambda: twin.add_pointcloud2(msg, sensor, intensity_field="auto"), "carries no intensity")
    d.close()
    for o in (a, b, twin, plain):
        o.close()


# ---- 4. the stages (I6) ------------------------------------------------------------------------------------------------------------------------
VOXEL = 0.1


def _trail():
    """The scene of tests/test_gpu_dense_carve.py: a wall 6 m in front of three origins and, in the first scan only, a blob half way."""
    rng = np.random.default_rng(11)
    scans = []
    for k in range(3):
        wall = np.c_[6.05 + 0.1 * k + rng.normal(0, 0.01, 700), rng.uniform(-1.5, 1.5, 700), rng.uniform(-1.0, 1.5, 700)]
        scans.append(wall if k else np.concatenate([np.c_[3.0 + rng.normal(0, 0.08, 300), rng.uniform(-0.3, 0.3, 300), rng.uniform(-0.2, 0.9, 300)], wall]))
    return scans, np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.25], [0.0, -0.5, 0.125]])


def test_stages_equal_the_twins_and_carry_the_index_through_both_removals(opt):
    from dmsa_lidar_slam_amd.dense_cloud import DenseCarveConfig

    scans, origins = _trail()
    pos = np.repeat(np.concatenate([origins, origins[-1:]]), 2, axis=0)
    quat = np.tile([0.0, 0.0, 0.0, 1.0], (8, 1))
    dc, twin, model = _pair(opt, base.S, pos, quat, retain=True, voxel_size=VOXEL)
    first, idx = 0, []
    for k, world in enumerate(scans):
        local = np.zeros((world.shape[0], 4), f32)
        local[:, :3] = (world - origins[k]).astype(f32)
        local[:, 3] = np.arange(first, first + world.shape[0], dtype=f32)  # the global index
        a, b = base.S[2 * k], base.S[2 * k + 1]
        t = np.linspace(a + 0.25 * (b - a), a + 0.75 * (b - a), world.shape[0])
        kept, _ = dc.add_scan(local, t)
        twin.add_scan(local, t)
        ref, _, kept_idx, _ = model.add_scan_indices(local, t, interpolate=dc.interpolate)
        assert np.array_equal(_bits(kept), _bits(ref))
        idx.append(first + kept_idx)
        first += world.shape[0]
    idx = np.concatenate(idx)
    g, o = dc.retained()
    gt, ot = twin.retained()
    assert np.array_equal(g[:, 3], idx.astype(f32)) and 1500 < idx.shape[0] <= first
    assert np.array_equal(_bits(g[:, :3]), _bits(gt[:, :3])) and np.array_equal(_bits(o), _bits(ot)) and (o[:, 3] == 1).all() and (gt[:, 3] == 1).all()
    # every stage result equals the twin's, bit for bit
    assert np.array_equal(dc.neighbour_moments(0.4), twin.neighbour_moments(0.4))
    assert np.array_equal(_bits(dc.compute_normals(0.4, 5)[0]), _bits(twin.compute_normals(0.4, 5)[0]))
    assert np.array_equal(_bits(dc.knn_mean_distance(0.4, 8)), _bits(twin.knn_mean_distance(0.4, 8)))
    (so, fo), (sot, fot) = dc.classify_outliers(0.4, 8, 1.0, download=True), twin.classify_outliers(0.4, 8, 1.0, download=True)
    assert so == sot and np.array_equal(fo, fot)
    py, cfg = DenseCarveConfig(), cm.Config()
    (sc, pc), (sct, pct) = dc.count_passes(py, download=True), twin.count_passes(py, download=True)
    assert sc == sct and np.array_equal(pc, pct)
    # remove_transients, then remove_outliers: the w column is the model's surviving indices
    want, want_stats = cm.count_passes(gt, o, cfg)
    assert np.array_equal(pc, want) and sc == want_stats and 0 < sc["transient"]
    keep = want < cfg.min_passes
    assert dc.remove_transients() == twin.remove_transients() == int(keep.sum())
    g2, o2 = dc.retained()
    g2t, _ = twin.retained()
    assert np.array_equal(g2[:, 3], idx[keep].astype(f32)) and np.array_equal(_bits(g2[:, :3]), _bits(g2t[:, :3])) and (o2[:, 3] == 1).all()
    flags, o_stats, _ = om.classify(g2t, 0.4, 8, 1.0)
    assert dc.classify_outliers(0.4, 8, 1.0) == twin.classify_outliers(0.4, 8, 1.0) == o_stats and 0 < o_stats["inliers"] < g2.shape[0]
    assert dc.remove_outliers() == twin.remove_outliers() == o_stats["inliers"]
    g3, o3 = dc.retained()
    g3t, o3t = twin.retained()
    assert np.array_equal(g3[:, 3], idx[keep][flags.astype(bool)].astype(f32)) and (o3[:, 3] == 1).all()
    assert np.array_equal(_bits(g3[:, :3]), _bits(g3t[:, :3])) and np.array_equal(_bits(o3), _bits(o3t))
    assert np.array_equal(_bits(dc.compute_normals(0.4, 5)[0]), _bits(twin.compute_normals(0.4, 5)[0]))
    dc.close(), twin.close()


# ---- 5. the files (I7) -------------------------------------------------------------------------------------------------------------------------
def test_three_scans_through_the_streaming_file(opt, tmp_path):
    from dmsa_lidar_slam_amd.dense_cloud import pcdHeaderXyzBinary, pcdHeaderXyziBinary

    dc, twin, _ = _pair(opt, lidar_to_imu=base.L2I, voxel_size=0.25, **base.GATES)
    dc.with_intensity()  # twice is fine
    path, path_t = tmp_path / "Dense.pcd", tmp_path / "Twin.pcd"
    dc.open_pcd(path), twin.open_pcd(path_t)
    _refused(twin.with_intensity, "before a file is open")
    kept, first = [], 0
    for n in (3000, 1, 5000):
        xyz, t = base._scan(n, 40 + n)
        xyz[:, 3] = np.arange(first, first + n, dtype=f32)
        first += n
        kept.append(dc.add_scan(xyz, t)[0])
        twin.add_scan(xyz, t)
    rows = np.concatenate(kept)
    points, size = dc.close_pcd()
    points_t, size_t = twin.close_pcd()
    raw = open(path, "rb").read()
    assert points == points_t == rows.shape[0] > 3000 and size == len(raw) == len(im.header_xyzi(0)) + 16 * points
    assert raw == im.header_xyzi(points).encode() + rows.tobytes() and pcdHeaderXyziBinary(points) == im.header_xyzi(points)  # every row's 16 bytes
    head, body, _, _ = im.read_pcd(path)
    assert head["FIELDS"] == "x y z intensity" and head["WIDTH"] == head["POINTS"] == "%012d" % points and len(np.unique(body[:, 3])) == points
    # the object without the switch writes 12-byte rows
    raw_t = open(path_t, "rb").read()
    assert size_t == len(raw_t) == len(pcdHeaderXyzBinary(0)) + 12 * points and raw_t == pcdHeaderXyzBinary(points).encode() + np.ascontiguousarray(rows[:, :3]).tobytes()
    # closing with zero points still leaves no file
    empty = tmp_path / "Empty.pcd"
    dc.open_pcd(empty)
    _refused(dc.close_pcd)
    assert not os.path.exists(empty)
    dc.close(), twin.close()


def test_the_files_of_the_store_have_four_and_eight_floats_per_row(opt, tmp_path):
    from dmsa_lidar_slam_amd.dense_cloud import pcdHeaderNormalsBinary, pcdHeaderXyziNormalsBinary

    s, p, q = base._still_trajectory()
    dc, twin, _ = _pair(opt, s, p, q, retain=True, voxel_size=0.1)
    rng = np.random.default_rng(5)
    xyz = np.zeros((6000, 4), f32)
    xyz[:, :3] = np.c_[rng.uniform(-2, 2, 6000), rng.uniform(-2, 2, 6000), 3.0 + rng.normal(0, 0.02, 6000)]
    xyz[:, 3] = np.arange(6000, dtype=f32)
    t = np.linspace(s[0], s[-1], 6000)
    dc.add_scan(xyz, t, download=False), twin.add_scan(xyz, t, download=False)
    g, _ = dc.retained()
    assert 1500 < g.shape[0] < 6000 and np.array_equal(_bits(g), _bits(xyz[g[:, 3].astype(np.int64)]))
    points, size = dc.save_pcd_retained(tmp_path / "Store.pcd")
    raw = open(tmp_path / "Store.pcd", "rb").read()
    assert (points, size) == (g.shape[0], len(raw)) and raw == im.header_xyzi(points).encode() + g.tobytes()
    normals, without = dc.compute_normals(0.3, 5)
    normals_t, without_t = twin.compute_normals(0.3, 5)
    assert np.array_equal(_bits(normals), _bits(normals_t)) and without == without_t < points
    points, size = dc.save_pcd_normals(tmp_path / "Normals.pcd")
    raw = open(tmp_path / "Normals.pcd", "rb").read()
    assert (points, size) == (g.shape[0], len(raw)) and raw == im.header_xyzi_normals(points).encode() + np.concatenate([g, normals], axis=1).tobytes()
    assert pcdHeaderXyziNormalsBinary(points) == im.header_xyzi_normals(points)
    points_t, size_t = twin.save_pcd_normals(tmp_path / "TwinNormals.pcd")  # 28-byte rows without the switch, as before
    raw_t = open(tmp_path / "TwinNormals.pcd", "rb").read()
    assert raw_t == pcdHeaderNormalsBinary(points).encode() + np.concatenate([g[:, :3], normals], axis=1).tobytes() and size_t == len(raw_t)
    dc.close(), twin.close()


def test_a_lattice_of_2_pow_20_plus_1_points_takes_the_store_file_across_a_chunk_edge(opt, tmp_path):
    """Every point in a voxel of its own, under the identity pose: the survivors are the input rows themselves, bit for bit, and the file of the
    store has one chunk of 2^20 rows and one of a single row."""
    from dmsa_lidar_slam_amd.dense_cloud import DenseCloudConfig, DenseCloudCreator

    n = 2**20 + 1
    i = np.arange(n)
    xyz = np.stack([(i % 128) + 0.25, ((i // 128) % 128) + 0.25, (i // 16384) + 0.25, i], axis=1).astype(f32)
    s, p, q = base._still_trajectory()
    dc = DenseCloudCreator(s, p, q, DenseCloudConfig(voxelSize=0.5), optimizer=opt, retain=True, intensity=True)
    dc.open_pcd(tmp_path / "Stream.pcd")
    _, st = dc.add_scan(xyz, np.linspace(s[0], s[-1], n), download=False)
    assert st["kept"] == n == dc.retained_count()
    assert dc.close_pcd() == (n, len(im.header_xyzi(0)) + 16 * n)
    points, size = dc.save_pcd_retained(tmp_path / "Store.pcd")
    want = im.header_xyzi(n).encode() + xyz.tobytes()
    assert (points, size) == (n, len(want))
    assert open(tmp_path / "Store.pcd", "rb").read() == want and open(tmp_path / "Stream.pcd", "rb").read() == want
    dc.close()


# ---- 6. the demo and the C++ driver -------------------------------------------------------------------------------------------------------------
def test_the_demo_and_the_cpp_driver_write_the_same_intensity_files(tmp_path):
    """The demo with every stage on: all four files carry the painted reflectance.  The C++ driver on the same recording with the same paint in
    its messages writes the same bytes, with the sensor's own field and with the field named."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples"))
    import dense_cloud_demo as demo
    from dmsa_lidar_slam_amd import raw_sequence as rs

    small = dict(rings=32, az_steps=256)
    r = demo.run(scans=6, workdir=str(tmp_path), num_iter=3, intensity=True, carve=True, outliers=(8, 1.0), normals=0.3, **small)
    rows = {}
    for key, fields in (("pcd", "x y z intensity"), ("carved_pcd", "x y z intensity"), ("clean_pcd", "x y z intensity"),
                        ("normals_pcd", "x y z intensity normal_x normal_y normal_z curvature")):
        head, body, _, _ = im.read_pcd(r[key])
        assert head["FIELDS"] == fields and int(head["POINTS"]) == body.shape[0] > 1000
        assert np.isin(body[:, 3], demo.REFLECTANCE).all() and len(np.unique(body[:, 3])) >= 4  # every row has a surface's value
        rows[key] = body
    # (the toy scene has next to nothing to carve: the carved store may be the whole one)
    assert rows["pcd"].shape[0] == r["stats"]["kept"] >= rows["carved_pcd"].shape[0] > rows["clean_pcd"].shape[0] == rows["normals_pcd"].shape[0]
    assert np.array_equal(_bits(rows["clean_pcd"]), _bits(rows["normals_pcd"][:, :4]))
    # the recording again with the paint in its messages
    painted, dump, k = demo.surface_reflectance(6, **small), str(tmp_path / "painted.raw"), 0
    writer = rs.RawWriter(dump)
    for kind, m in rs.RawReader(r["dump"]):
        assert kind == "pointcloud2"
        writer.writePointCloud2(demo.paint(m, painted[k]))
        k += 1
    writer.close()
    exe = os.path.join(root, "examples", "dense_cloud_from_raw")
    stages = ["--carve", "--outlier-k", "8", "--outlier-mul", "1.0", "--outlier-radius", "0.3"]
    for out, radius, flags, twin in (("stream.pcd", [], ["--intensity"], "pcd"), ("named.pcd", [], ["--intensity", "3:float32"], "pcd"),
                                     ("clean.pcd", [], stages + ["--intensity", "3:7"], "clean_pcd"), ("normals.pcd", ["0.3"], ["--intensity"] + stages, "normals_pcd")):
        p = subprocess.run([exe, dump, r["poses_file"], "ouster", str(tmp_path / out)] + radius + ["--voxel", "0.1", "--min-range", "0.5"] + flags,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "intensity: field 3, datatype 7" in p.stdout, p.stdout[-1000:] + p.stderr[-1000:]
        assert open(tmp_path / out, "rb").read() == open(r[twin], "rb").read(), out
    # the reflectivity of the same messages is a uint16 of zeros: named by hand, it gives +0.0 throughout
    p = subprocess.run([exe, dump, r["poses_file"], "ouster", str(tmp_path / "refl.pcd"), "--voxel", "0.1", "--min-range", "0.5", "--intensity", "5:uint16"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-1000:]
    body = im.read_pcd(tmp_path / "refl.pcd")[1]
    assert np.array_equal(_bits(body[:, :3]), _bits(rows["pcd"][:, :3])) and (_bits(body[:, 3]) == 0).all()
    # a sensor without a known field has to name it
    p = subprocess.run([exe, dump, r["poses_file"], "unknown", str(tmp_path / "no.pcd"), "--intensity"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "name it as INDEX:TYPE" in p.stderr and not (tmp_path / "no.pcd").exists()
