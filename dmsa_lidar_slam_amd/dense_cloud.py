"""Python mirror of include/dmsa_dense_cloud.h: the dense point cloud -- every raw point of every scan placed at the pose interpolated for
its own time stamp along a saved trajectory (the TUM lines of Poses.txt), gated, thinned to one point per voxel across the scans, and
written as a binary PCD.  The per-point work runs on the GPU (csrc/dense_cloud.hip); there is no CPU fallback.  The semantics (rules 1-7)
are stated in the header."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _capi as capi
from .api import DmsaError, DmsaOptimizer
from .wire_formats import PointCloud2Msg

STAT_NAMES = tuple(n for n, _ in capi.DenseStats._fields_)


@dataclass
class DenseCloudConfig:
    """dmsa_dense_config; the defaults are dmsa_default_dense_config's."""
    lidarToImu: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=np.float32))  # 4 x 4, as a matrix (stored column-major in C)
    minRange: float = 0.0
    maxRange: float = 0.0       # <= 0: no upper gate
    timeOffset: float = 0.0
    maxPoseGap: float = 0.0     # <= 0: every segment is interpolated across
    voxelSize: float = 0.0      # <= 0: no thinning

    def to_c(self) -> capi.DenseConfig:
        c = capi.DenseConfig()
        m = np.asarray(self.lidarToImu, np.float32)
        if m.shape != (4, 4):
            raise ValueError("lidarToImu must be 4 x 4")
        c.lidar_to_imu = (C.c_float * 16)(*[float(v) for v in m.T.reshape(-1)])
        c.min_range, c.max_range, c.time_offset, c.max_pose_gap, c.voxel_size = (float(np.float32(self.minRange)), float(np.float32(self.maxRange)),
                                                                                 float(self.timeOffset), float(self.maxPoseGap), float(np.float32(self.voxelSize)))
        return c


def _stats(s: capi.DenseStats) -> dict:
    return {n: int(getattr(s, n)) for n in STAT_NAMES}


def parse_tum_poses(text: bytes | str):
    """dmsa_parse_tum_poses: (stamps (n,), positions (n,3), quaternions (n,4) as x y z w) of the `stamp tx ty tz qx qy qz qw` lines; blank
    lines and # lines are skipped.  Host only.  A malformed line raises ValueError naming its line number."""
    lib = capi.load_library()
    raw = text.encode() if isinstance(text, str) else bytes(text)
    n, err = C.c_int64(0), C.create_string_buffer(256)
    null = capi.ptr(None, C.c_double)
    rc = lib.dmsa_parse_tum_poses(raw, len(raw), null, null, null, 0, C.byref(n), err, 256)  # the counting pass
    if rc != capi.DMSA_OK and err.value.startswith(b"line"):
        raise ValueError(err.value.decode())
    cnt = int(n.value)
    stamps, pos, quat = np.zeros(max(cnt, 1)), np.zeros((max(cnt, 1), 3)), np.zeros((max(cnt, 1), 4))
    rc = lib.dmsa_parse_tum_poses(raw, len(raw), capi.ptr(stamps, C.c_double), capi.ptr(pos, C.c_double), capi.ptr(quat, C.c_double), cnt, C.byref(n), err, 256)
    if rc != capi.DMSA_OK:
        raise ValueError(err.value.decode() or f"dmsa_parse_tum_poses failed with {rc}")
    return stamps[:cnt], pos[:cnt], quat[:cnt]


def pcdHeaderXyzBinary(n: int) -> str:
    """The header of the binary x y z PCD with width = n (the counts twelve digits wide; recalled from PCL's format description)."""
    lib = capi.load_library()
    buf = C.create_string_buffer(512)
    rc = lib.dmsa_pcd_header_xyz_binary(int(n), buf, 512)
    if rc < 0:
        raise DmsaError(f"dmsa_pcd_header_xyz_binary failed with {rc}")
    return buf.raw[:rc].decode()


def pcdHeaderNormalsBinary(n: int) -> str:
    """The header of the seven-field binary PCD (x y z normal_x normal_y normal_z curvature) with width = n: include/dmsa_dense_normals.h, N5."""
    lib = capi.load_library()
    buf = C.create_string_buffer(512)
    rc = lib.dmsa_pcd_header_normals_binary(int(n), buf, 512)
    if rc < 0:
        raise DmsaError(f"dmsa_pcd_header_normals_binary failed with {rc}")
    return buf.raw[:rc].decode()


def _header(call: str, n: int) -> str:
    lib = capi.load_library()
    buf = C.create_string_buffer(512)
    rc = getattr(lib, call)(int(n), buf, 512)
    if rc < 0:
        raise DmsaError(f"{call} failed with {rc}")
    return buf.raw[:rc].decode()


def pcdHeaderXyziBinary(n: int) -> str:
    """The header of the binary x y z intensity PCD with width = n: include/dmsa_dense_intensity.h, I7."""
    return _header("dmsa_pcd_header_xyzi_binary", n)


def pcdHeaderXyziNormalsBinary(n: int) -> str:
    """The header of the eight-field binary PCD (x y z intensity normal_x normal_y normal_z curvature) with width = n: I7."""
    return _header("dmsa_pcd_header_xyzi_normals_binary", n)


def pcdHeaderXyzLabelBinary(n: int, intensity: bool = False) -> str:
    """The header of the binary x y z label PCD (x y z intensity label with `intensity`) with width = n: include/dmsa_dense_clusters.h, C7."""
    lib = capi.load_library()
    buf = C.create_string_buffer(512)
    rc = lib.dmsa_pcd_header_xyz_label_binary(int(n), 1 if intensity else 0, buf, 512)
    if rc < 0:
        raise DmsaError(f"dmsa_pcd_header_xyz_label_binary failed with {rc}")
    return buf.raw[:rc].decode()


def pcdHeaderXyzDistanceBinary(n: int, intensity: bool = False) -> str:
    """The header of the binary x y z distance PCD (x y z intensity distance with `intensity`) with width = n: include/dmsa_dense_compare.h, D7."""
    lib = capi.load_library()
    buf = C.create_string_buffer(512)
    rc = lib.dmsa_pcd_header_xyz_distance_binary(int(n), 1 if intensity else 0, buf, 512)
    if rc < 0:
        raise DmsaError(f"dmsa_pcd_header_xyz_distance_binary failed with {rc}")
    return buf.raw[:rc].decode()


def read_pcd_xyz(path) -> np.ndarray:
    """dmsa_pcd_xyz_info / dmsa_pcd_xyz_read: the x y z of every row of a binary PCD as (n,3) float32 (include/dmsa_dense_compare.h, D8: every
    file this library writes).  Anything else raises DmsaError naming what was met."""
    lib = capi.load_library()
    n = C.c_int64(0)
    raw = str(path).encode()
    rc = lib.dmsa_pcd_xyz_info(raw, C.byref(n))
    if rc == capi.DMSA_OK:
        out = np.zeros((max(int(n.value), 1), 3), np.float32)
        rc = lib.dmsa_pcd_xyz_read(raw, capi.ptr(out, C.c_float), int(n.value), C.byref(n))
    if rc != capi.DMSA_OK:
        e = DmsaError(f"dmsa_pcd_xyz_read failed with {rc}: {lib.dmsa_pcd_xyz_last_error().decode()}")
        e.status = rc
        raise e
    return out[: int(n.value)]


def compare_summary(matched: int, s1: int, s2: int, within: int, queries: int, scale: float):
    """dmsa_dense_compare_summary: D5 of one direction on the host, from the exact sums of D4: (mean_m, rms_m, fraction_within).  Arguments out
    of range raise DmsaError."""
    lib = capi.load_library()
    m, r, f = C.c_double(0), C.c_double(0), C.c_double(0)
    rc = lib.dmsa_dense_compare_summary(int(matched), int(s1), int(s2), int(within), int(queries), float(scale), C.byref(m), C.byref(r), C.byref(f))
    if rc != capi.DMSA_OK:
        raise DmsaError(f"dmsa_dense_compare_summary failed with {rc}")
    return m.value, r.value, f.value


def _align_sums(words) -> dict:
    """A2's 25 words as Python ints: n, sp (3), sg (3) and spg (3 x 3, each hi * 2^32 + lo recombined)."""
    w = [int(v) for v in words]
    return dict(n=w[0], sp=w[1:4], sg=w[4:7], spg=[[(w[8 + 2 * (3 * a + b)] << 32) + w[7 + 2 * (3 * a + b)] for b in range(3)] for a in range(3)])


def align_sum_words(sums) -> list:
    """The 25 int64 words of include/dmsa_dense_align.h, A2, from a dict as align_sums() gives it (a list of 25 words passes through)."""
    if not isinstance(sums, dict):
        w = [int(v) for v in sums]
        if len(w) != capi.ALIGN_SUMS:
            raise ValueError("25 words are expected")
        return w
    w = [int(sums["n"])] + [int(v) for v in sums["sp"]] + [int(v) for v in sums["sg"]]
    for a in range(3):
        for b in range(3):
            v = int(sums["spg"][a][b])
            w += [v & 0xFFFFFFFF, v >> 32]
    return w


def align_solve(sums, scale_c: float = 1.0):
    """dmsa_dense_align_solve: A3-A4 on the host from the exact sums (a dict as align_sums() gives it, or the 25 words): (dT (3,4) float64,
    shift_m, rotation_rad).  scale_c = 1 leaves the translation and the shift in quantised units.  Sums outside A2's ranges raise DmsaError."""
    lib = capi.load_library()
    words = align_sum_words(sums)
    if any(not -(2**63) <= v < 2**63 for v in words):
        raise DmsaError("dmsa_dense_align_solve: a word does not fit 64 bits")
    arr = (C.c_int64 * capi.ALIGN_SUMS)(*words)
    dT = np.zeros((3, 4), np.float64)
    sh, rot = C.c_double(0), C.c_double(0)
    rc = lib.dmsa_dense_align_solve(arr, float(scale_c), capi.ptr(dT, C.c_double), C.byref(sh), C.byref(rot))
    if rc != capi.DMSA_OK:
        e = DmsaError(f"dmsa_dense_align_solve failed with {rc}")
        e.status = rc
        raise e
    return dT, sh.value, rot.value


def align_compose(step, transform) -> np.ndarray:
    """dmsa_dense_align_compose: A5, step o transform, both (3,4) float64."""
    lib = capi.load_library()
    d, t = np.ascontiguousarray(np.asarray(step, np.float64)[:3, :4]), np.ascontiguousarray(np.asarray(transform, np.float64)[:3, :4])
    out = np.zeros((3, 4), np.float64)
    if lib.dmsa_dense_align_compose(capi.ptr(d, C.c_double), capi.ptr(t, C.c_double), capi.ptr(out, C.c_double)) != capi.DMSA_OK:
        raise DmsaError("dmsa_dense_align_compose failed")
    return out


def _limbs_value(w) -> int:
    """P2's limb rule read back: sum limb_k * 2^(32 k)."""
    return sum(int(v) << (32 * k) for k, v in enumerate(w))


def _limbs_of(v: int, limbs: int) -> list:
    """P2's limb rule: the lower limbs masked, the top one shifted arithmetically."""
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(limbs - 1)] + [v >> (32 * (limbs - 1))]


def _align_plane_sums(words) -> dict:
    """P2's 64 words as Python ints: n, no_normal, sp (3), nn (6: xx xy xz yy yz zz), cn (3 x 3), cc (6), ne (3), ce (3), ee, the limbs recombined."""
    w = [int(v) for v in words]
    return dict(n=w[0], no_normal=w[1], sp=w[2:5], nn=w[5:11], cn=[[_limbs_value(w[11 + 2 * (3 * a + b):13 + 2 * (3 * a + b)]) for b in range(3)] for a in range(3)],
                cc=[_limbs_value(w[29 + 3 * k:32 + 3 * k]) for k in range(6)], ne=[_limbs_value(w[47 + 2 * a:49 + 2 * a]) for a in range(3)],
                ce=[_limbs_value(w[53 + 3 * a:56 + 3 * a]) for a in range(3)], ee=_limbs_value(w[62:64]))


def align_plane_sum_words(sums) -> list:
    """The 64 int64 words of include/dmsa_dense_align_plane.h, P2, from a dict as align_plane_sums() gives it (a list of 64 words passes through)."""
    if not isinstance(sums, dict):
        w = [int(v) for v in sums]
        if len(w) != capi.ALIGN_PLANE_SUMS:
            raise ValueError("64 words are expected")
        return w
    w = [int(sums["n"]), int(sums["no_normal"])] + [int(v) for v in sums["sp"]] + [int(v) for v in sums["nn"]]
    for row in sums["cn"]:
        for v in row:
            w += _limbs_of(int(v), 2)
    for v in sums["cc"]:
        w += _limbs_of(int(v), 3)
    for v in sums["ne"]:
        w += _limbs_of(int(v), 2)
    for v in sums["ce"]:
        w += _limbs_of(int(v), 3)
    return w + _limbs_of(int(sums["ee"]), 2)


def align_plane_solve(sums, scale_c: float = 1.0):
    """dmsa_dense_align_plane_solve: P3-P5 on the host from the exact sums (a dict as align_plane_sums() gives it, or the 64 words): (dT (3,4)
    float64, shift_m, rotation_rad, min_pivot, degenerate).  A degenerate system gives the identity, zeros and the pivot that failed.  scale_c =
    1 leaves the translation and the shift in quantised units.  Sums outside P2's ranges raise DmsaError."""
    lib = capi.load_library()
    words = align_plane_sum_words(sums)
    if any(not -(2**63) <= v < 2**63 for v in words):
        raise DmsaError("dmsa_dense_align_plane_solve: a word does not fit 64 bits")
    arr = (C.c_int64 * capi.ALIGN_PLANE_SUMS)(*words)
    dT = np.zeros((3, 4), np.float64)
    sh, rot, piv = C.c_double(0), C.c_double(0), C.c_double(0)
    rc = lib.dmsa_dense_align_plane_solve(arr, float(scale_c), capi.ptr(dT, C.c_double), C.byref(sh), C.byref(rot), C.byref(piv))
    if rc not in (capi.DMSA_OK, capi.ALIGN_PLANE_DEGENERATE):
        e = DmsaError(f"dmsa_dense_align_plane_solve failed with {rc}")
        e.status = rc
        raise e
    return dT, sh.value, rot.value, piv.value, rc == capi.ALIGN_PLANE_DEGENERATE


def write_transform(path, T):
    """A 3 x 4 transform as three lines of four %.17g values: every double survives the round trip."""
    t = np.asarray(T, np.float64)[:3, :4]
    if t.shape != (3, 4):
        raise ValueError("the transform must be 3x4 or 4x4")
    with open(path, "w") as f:
        for row in t:
            f.write(" ".join("%.17g" % v for v in row) + "\n")


def read_transform(path) -> np.ndarray:
    """The file write_transform() writes (and examples/dense_cloud_from_raw --align-out): twelve numbers, (3,4) float64."""
    with open(path) as f:
        vals = f.read().split()
    if len(vals) != 12:
        raise ValueError(f"{path}: {len(vals)} values, 12 are expected")
    return np.array([float(v) for v in vals], np.float64).reshape(3, 4)


def _compare_direction(d: capi.DenseCompareDirection) -> dict:
    out = {n: int(getattr(d, n)) for n in ("queries", "matched", "unmatched", "within", "s1", "s2")}
    out["histogram"] = [int(v) for v in d.histogram]
    out.update({n: float(getattr(d, n)) for n in ("mean_m", "rms_m", "fraction_within")})
    return out


def _compare_stats(st: capi.DenseCompareStats) -> dict:
    out = {n: int(getattr(st, n)) for n in ("rows", "ref_rows", "ref_invalid", "kept")}
    out.update({n: float(getattr(st, n)) for n in ("scale", "bin_width_m", "precision", "recall", "f_score")})
    out["accuracy"], out["completeness"] = _compare_direction(st.accuracy), _compare_direction(st.completeness)
    return out


def _field(field) -> capi.PointCloud2Field:
    """(index, datatype) with the datatype a sensor_msgs/PointField constant 1..8 or its name ("uint16", "float32", ...)."""
    index, datatype = field
    return capi.PointCloud2Field(int(index), int(capi.FIELD_DATATYPES.get(datatype, datatype)))


def sensor_intensity_field(sensor: str):
    """dmsa_sensor_intensity_field: (index, datatype) of the field that carries the intensity in the messages of `sensor` (recalled from the
    drivers' layouts); DmsaError for "sick" and "unknown", whose caller names the field."""
    if sensor not in capi.SENSORS:
        raise ValueError(f"unknown sensor type {sensor!r}; one of {sorted(capi.SENSORS)}")
    f = capi.PointCloud2Field()
    rc = capi.load_library().dmsa_sensor_intensity_field(capi.SENSORS[sensor], C.byref(f))
    if rc != capi.DMSA_OK:
        raise DmsaError(f"dmsa_sensor_intensity_field failed with {rc}: sensor {sensor!r} has no known intensity field, name it as (index, datatype)")
    return int(f.index), int(f.datatype)


def normal_from_moments(moments, view, min_neighbours: int = 0) -> np.ndarray:
    """dmsa_dense_normal_from_moments, row by row: N4 on the host through the header the device kernel compiles.  moments (n,10) int64,
    view (n,3) float32 = o - g; returns (n,4) float32 (nx, ny, nz, curvature), NaN rows where n < max(3, min_neighbours)."""
    lib = capi.load_library()
    m = np.ascontiguousarray(moments, np.int64).reshape(-1, 10)
    v = np.ascontiguousarray(view, np.float32).reshape(-1, 3)
    if m.shape[0] != v.shape[0]:
        raise ValueError("moments and view differ in length")
    out = np.zeros((m.shape[0], 4), np.float32)
    for i in range(m.shape[0]):
        rc = lib.dmsa_dense_normal_from_moments(m[i].ctypes.data_as(C.POINTER(C.c_int64)), v[i].ctypes.data_as(C.POINTER(C.c_float)), int(min_neighbours),
                                                out[i].ctypes.data_as(C.POINTER(C.c_float)))
        if rc != capi.DMSA_OK:
            raise DmsaError(f"dmsa_dense_normal_from_moments failed with {rc} (row {i})")
    return out


OUTLIER_STAT_NAMES = tuple(n for n, _ in capi.DenseOutlierStats._fields_)


def outlier_threshold(n_s: int, s1: int, s2: int, stddev_mul: float = 1.0):
    """dmsa_dense_outlier_threshold: O5 of include/dmsa_dense_outliers.h on the host, from the three exact sums of O4: (mean, stddev, T) in the
    units of q.  Arguments out of range raise DmsaError."""
    lib = capi.load_library()
    m, sd, t = C.c_double(0), C.c_double(0), C.c_double(0)
    rc = lib.dmsa_dense_outlier_threshold(int(n_s), int(s1), int(s2), float(np.float32(stddev_mul)), C.byref(m), C.byref(sd), C.byref(t))
    if rc != capi.DMSA_OK:
        raise DmsaError(f"dmsa_dense_outlier_threshold failed with {rc}")
    return m.value, sd.value, t.value


CARVE_STAT_NAMES = tuple(n for n, _ in capi.DenseCarveStats._fields_)
CLUSTER_STAT_NAMES = tuple(n for n, _ in capi.DenseClusterStats._fields_)


@dataclass
class DenseCarveConfig:
    """dmsa_dense_carve_config; the defaults are dmsa_default_dense_carve_config's (from a synthetic toy scene, not from recorded data)."""
    cell_size: float = 0.2
    rho: float = 0.1
    tan_half_angle: float = 0.052407779  # the float nearest tan 3 deg
    end_margin: float = 0.3
    start_margin: float = 0.5
    max_length: float = 30.0
    min_passes: int = 2

    def to_c(self) -> capi.DenseCarveConfig:
        f = [float(np.float32(v)) for v in (self.cell_size, self.rho, self.tan_half_angle, self.end_margin, self.start_margin, self.max_length)]
        return capi.DenseCarveConfig(*f, int(self.min_passes), 0)


def carve_walk(cell_size: float, o, g):
    """dmsa_dense_carve_walk: T2's skip test (without the length limit), T3 and T4 of include/dmsa_dense_carve.h for the ray o -> g on the host,
    through the header the device kernels compile.  Returns the traversed cells (n,3) int32 in walk order, or None for a skipped ray."""
    lib = capi.load_library()
    o, g = np.ascontiguousarray(o, np.float32).reshape(3), np.ascontiguousarray(g, np.float32).reshape(3)
    n = C.c_int64(0)
    rc = lib.dmsa_dense_carve_walk(float(np.float32(cell_size)), capi.ptr(o, C.c_float), capi.ptr(g, C.c_float), capi.ptr(None, C.c_int32), 0, C.byref(n))  # the counting pass
    if rc != capi.DMSA_OK:
        raise DmsaError(f"dmsa_dense_carve_walk failed with {rc}")
    if n.value < 0:
        return None
    cells = np.zeros((int(n.value), 3), np.int32)
    rc = lib.dmsa_dense_carve_walk(float(np.float32(cell_size)), capi.ptr(o, C.c_float), capi.ptr(g, C.c_float), capi.ptr(cells, C.c_int32), cells.shape[0], C.byref(n))
    if rc != capi.DMSA_OK or n.value != cells.shape[0]:
        raise DmsaError(f"dmsa_dense_carve_walk failed with {rc}")
    return cells


def carve_sees_through(cfg: DenseCarveConfig | None, o, g, p) -> bool:
    """dmsa_dense_carve_sees_through: T2's L and T5 for the ray o -> g and the point p, on the host.  A config T1 refuses raises DmsaError."""
    lib = capi.load_library()
    c = (cfg or DenseCarveConfig()).to_c()
    o, g, p = (np.ascontiguousarray(v, np.float32).reshape(3) for v in (o, g, p))
    rc = lib.dmsa_dense_carve_sees_through(C.byref(c), capi.ptr(o, C.c_float), capi.ptr(g, C.c_float), capi.ptr(p, C.c_float))
    if rc < 0:
        raise DmsaError(f"dmsa_dense_carve_sees_through failed with {rc}")
    return bool(rc)


OCCUPANCY_STAT_NAMES = tuple(n for n, _ in capi.DenseOccupancyStats._fields_)
OCCUPANCY_SLICE_NAMES = tuple(n for n, _ in capi.DenseOccupancySliceInfo._fields_)
OCCUPANCY_UNKNOWN, OCCUPANCY_FREE, OCCUPANCY_OCCUPIED = 0, 1, 2


@dataclass
class DenseOccupancyConfig:
    """dmsa_dense_occupancy_config; the defaults are dmsa_default_dense_occupancy_config's (from a synthetic toy scene, not from recorded data)."""
    cell_size: float = 0.2
    max_length: float = 30.0
    min_hits: int = 1
    min_passes: int = 2
    occ_num: int = 16
    occ_den: int = 1
    initial_slots: int = 0  # 0: automatic; else the first table size (a test forces rebuilds with it)

    def to_c(self) -> capi.DenseOccupancyConfig:
        return capi.DenseOccupancyConfig(float(np.float32(self.cell_size)), float(np.float32(self.max_length)), int(self.min_hits), int(self.min_passes), int(self.occ_num),
                                         int(self.occ_den), int(self.initial_slots))


def occupancy_state(cfg: DenseOccupancyConfig | None, hits: int, passes: int) -> int:
    """dmsa_dense_occupancy_state: M5 of include/dmsa_dense_occupancy.h on the host: 0 unknown, 1 free, 2 occupied.  A config M1 refuses raises
    DmsaError."""
    lib = capi.load_library()
    c = (cfg or DenseOccupancyConfig()).to_c()
    rc = lib.dmsa_dense_occupancy_state(C.byref(c), int(hits), int(passes))
    if rc < 0:
        raise DmsaError(f"dmsa_dense_occupancy_state failed with {rc}")
    return int(rc)


def pcdHeaderOccupancyBinary(n: int) -> str:
    """The header of the binary x y z hits passes state PCD with width = n: include/dmsa_dense_occupancy.h, M6."""
    return _header("dmsa_pcd_header_occupancy_binary", n)


def occupancy_map_pgm_header(width: int, height: int) -> str:
    """M7: the header of the PGM."""
    lib = capi.load_library()
    buf = C.create_string_buffer(64)
    rc = lib.dmsa_occupancy_map_pgm_header(int(width), int(height), buf, 64)
    if rc < 0:
        raise DmsaError(f"dmsa_occupancy_map_pgm_header failed with {rc}")
    return buf.raw[:rc].decode()


def occupancy_map_yaml(pgm_path, cell_size: float, cx_min: int, cy_min: int) -> str:
    """M7: the six lines of the YAML beside the PGM at `pgm_path` (its basename is the image)."""
    lib = capi.load_library()
    buf = C.create_string_buffer(4608)
    rc = lib.dmsa_occupancy_map_yaml(str(pgm_path).encode(), float(np.float32(cell_size)), int(cx_min), int(cy_min), buf, 4608)
    if rc < 0:
        raise DmsaError(f"dmsa_occupancy_map_yaml failed with {rc}")
    return buf.raw[:rc].decode()


SURFACE_STAT_NAMES = tuple(n for n, _ in capi.DenseSurfaceStats._fields_)
MESH_STAT_NAMES = tuple(n for n, _ in capi.DenseMeshStats._fields_)


@dataclass
class DenseSurfaceConfig:
    """dmsa_dense_surface_config; the defaults are dmsa_default_dense_surface_config's (placeholders from a synthetic toy scene, not from
    recorded data)."""
    cell_size: float = 0.2
    truncation: float = 0.6
    max_length: float = 30.0
    min_weight: int = 2
    initial_slots: int = 0  # 0: automatic; else the first table size (a test forces rebuilds with it)

    def to_c(self) -> capi.DenseSurfaceConfig:
        return capi.DenseSurfaceConfig(float(np.float32(self.cell_size)), float(np.float32(self.truncation)), float(np.float32(self.max_length)), int(self.min_weight),
                                       int(self.initial_slots))


def surface_samples(cfg: DenseSurfaceConfig | None, o, g):
    """dmsa_dense_surface_samples: S2-S4 of include/dmsa_dense_surface.h for the ray o -> g on the host, through the header the device kernels
    compile.  Returns (cells (n,3) int32 in walk order, q (n,) int32), or None for a skipped ray.  A config S1 refuses raises DmsaError."""
    lib = capi.load_library()
    c = (cfg or DenseSurfaceConfig()).to_c()
    o, g = np.ascontiguousarray(o, np.float32).reshape(3), np.ascontiguousarray(g, np.float32).reshape(3)
    n = C.c_int64(0)
    rc = lib.dmsa_dense_surface_samples(C.byref(c), capi.ptr(o, C.c_float), capi.ptr(g, C.c_float), capi.ptr(None, C.c_int32), capi.ptr(None, C.c_int32), 0, C.byref(n))
    if rc != capi.DMSA_OK:
        raise DmsaError(f"dmsa_dense_surface_samples failed with {rc}")
    if n.value < 0:
        return None
    k = int(n.value)
    cells, q = np.zeros((max(k, 1), 3), np.int32), np.zeros(max(k, 1), np.int32)
    rc = lib.dmsa_dense_surface_samples(C.byref(c), capi.ptr(o, C.c_float), capi.ptr(g, C.c_float), capi.ptr(cells, C.c_int32), capi.ptr(q, C.c_int32), k, C.byref(n))
    if rc != capi.DMSA_OK or n.value != k:
        raise DmsaError(f"dmsa_dense_surface_samples failed with {rc}")
    return cells[:k], q[:k]


def pcdHeaderTsdfBinary(n: int) -> str:
    """The header of the binary x y z tsdf weight PCD with width = n: include/dmsa_dense_surface.h, S7."""
    return _header("dmsa_pcd_header_tsdf_binary", n)


def plyHeaderMesh(vertices: int, triangles: int) -> str:
    """The header of the binary PLY of a mesh: include/dmsa_dense_surface.h, S9."""
    lib = capi.load_library()
    buf = C.create_string_buffer(512)
    rc = lib.dmsa_ply_header_mesh(int(vertices), int(triangles), buf, 512)
    if rc < 0:
        raise DmsaError(f"dmsa_ply_header_mesh failed with {rc}")
    return buf.raw[:rc].decode()


class DenseCloudCreator:
    """One trajectory, scans added in call order.  `optimizer`: share that DmsaOptimizer's context; otherwise a private one on `device`.
    `retain`: keep every survivor and its sensor origin in HBM (include/dmsa_dense_normals.h, N0) for retained() / compute_normals().
    `intensity`: the fourth float of every point row is its intensity, carried to retained() and to a fourth field of the files
    (include/dmsa_dense_intensity.h, I1-I7)."""

    def __init__(self, stamps, positions, quaternions_xyzw, config: DenseCloudConfig | None = None, device: int = 0, optimizer: DmsaOptimizer | None = None,
                 retain: bool = False, intensity: bool = False):
        self._lib = capi.load_library()
        self._dc = None
        self._own = None
        if optimizer is None:
            optimizer = self._own = DmsaOptimizer(device=device)  # raises without a device: there is no CPU fallback
        self._opt = optimizer
        self.config = config or DenseCloudConfig()
        s = np.ascontiguousarray(stamps, np.float64).reshape(-1)
        p = np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
        q = np.ascontiguousarray(quaternions_xyzw, np.float64).reshape(-1, 4)
        if not (s.shape[0] == p.shape[0] == q.shape[0]):
            raise ValueError("stamps, positions and quaternions differ in length")
        cfg, dc = self.config.to_c(), C.c_void_p()
        rc = self._lib.dmsa_dense_cloud_create(self._opt._ctx, C.byref(cfg), capi.ptr(s, C.c_double), capi.ptr(p, C.c_double), capi.ptr(q, C.c_double), s.shape[0],
                                               C.byref(dc))
        if rc != capi.DMSA_OK:
            msg = self._lib.dmsa_last_error(self._opt._ctx).decode()
            if self._own is not None:
                self._own.close()
            raise DmsaError(f"dmsa_dense_cloud_create failed with {rc}: {msg}")
        self._dc = dc
        self.numPoses = int(s.shape[0])
        if retain:
            self.retain()
        if intensity:
            self.with_intensity()

    @property
    def intensity(self) -> bool:
        """dmsa_dense_cloud_has_intensity."""
        return self._lib.dmsa_dense_cloud_has_intensity(self._dc) == 1

    def with_intensity(self):
        """I1: legal only before the first scan and before a file is open; calling it twice is fine."""
        self._check(self._lib.dmsa_dense_cloud_with_intensity(self._dc), "dmsa_dense_cloud_with_intensity")

    @classmethod
    def from_tum_file(cls, path, config: DenseCloudConfig | None = None, **kw):
        """The trajectory from a Poses.txt (TUM lines)."""
        with open(path, "rb") as f:
            stamps, pos, quat = parse_tum_poses(f.read())
        return cls(stamps, pos, quat, config, **kw)

    def close(self):
        if getattr(self, "_dc", None):
            if getattr(self._opt, "_ctx", None):  # (the object lives on the context: once that is gone it can only be dropped)
                self._lib.dmsa_dense_cloud_destroy(self._dc)
            self._dc = None
        if getattr(self, "_own", None) is not None:
            self._own.close()
            self._own = None

    __del__ = close

    def _check(self, rc, what):
        if rc != capi.DMSA_OK:
            e = DmsaError(f"{what} failed with {rc}: {self._lib.dmsa_last_error(self._opt._ctx).decode()}")
            e.status = rc
            raise e

    def interpolate(self, t):
        """Rules 3-4 for the stamps t: (pose12 (n,12) = R row-major | tr, segment (n,) = j, -1 out of time, -2 in a gap)."""
        t = np.ascontiguousarray(t, np.float64).reshape(-1)
        n = t.shape[0]
        pose, seg = np.zeros((max(n, 1), 12)), np.zeros(max(n, 1), np.int32)
        self._check(self._lib.dmsa_dense_cloud_interpolate(self._dc, capi.ptr(t, C.c_double), n, capi.ptr(pose, C.c_double), capi.ptr(seg, C.c_int32)),
                    "dmsa_dense_cloud_interpolate")
        return pose[:n], seg[:n]

    def _outputs(self, n, capacity, download):
        cap = n if capacity is None else int(capacity)
        out = np.zeros((max(cap, 1), 4), np.float32) if download else None
        return cap, out, C.c_int64(0), capi.DenseStats()

    def _result(self, rc, what, out, kept, st):
        self.lastKept, self.lastStats = int(kept.value), _stats(st)
        self._check(rc, what)
        return (out[: self.lastKept] if out is not None else None), self.lastStats

    def add_scan(self, xyz, stamps, capacity: int | None = None, download: bool = True):
        """One scan through rules 1-7: (kept points (m,4) float32 with w = 1 in input order -- None with download=False --, this call's
        statistics).  A `capacity` below m raises DmsaError (lastKept / lastStats still tell m) and leaves the object as it was.  On an
        intensity object the fourth float of an (n,4) row is the point's intensity and comes back as the survivor's w, bit for bit (I3)."""
        xyz = np.asarray(xyz, np.float32)
        if xyz.ndim != 2 or xyz.shape[1] not in (3, 4):
            raise ValueError("points must be (n,3) or (n,4)")
        if xyz.shape[1] == 3:
            xyz = np.concatenate([xyz, np.zeros((xyz.shape[0], 1), np.float32)], axis=1)
        xyz = np.ascontiguousarray(xyz)
        st = np.ascontiguousarray(stamps, np.float64).reshape(-1)
        n = xyz.shape[0]
        if st.shape[0] != n:
            raise ValueError("points and stamps differ in length")
        cap, out, kept, cs = self._outputs(n, capacity, download)
        rc = self._lib.dmsa_dense_cloud_add_scan(self._dc, capi.ptr(xyz, C.c_float), capi.ptr(st, C.c_double), n, capi.ptr(out, C.c_float), cap, C.byref(kept),
                                                 C.byref(cs))
        return self._result(rc, "dmsa_dense_cloud_add_scan", out, kept, cs)

    def add_pointcloud2(self, msg: PointCloud2Msg, sensor: str, delta_t_pcs: float = 0.0, capacity: int | None = None, download: bool = True,
                        intensity_field=None):
        """The same for one PointCloud2 message: decoded and placed on the device.  intensity_field = (index, datatype) or "auto" (the
        sensor's own: sensor_intensity_field) on an intensity object: that field of every point is its intensity (I4-I5); without it every
        point of an intensity object gets +0.0."""
        if sensor not in capi.SENSORS:
            raise ValueError(f"unknown sensor type {sensor!r}; one of {sorted(capi.SENSORS)}")
        n = int(msg.height) * int(msg.width)
        cm = msg.to_c(delta_t_pcs)
        cap, out, kept, cs = self._outputs(n, capacity, download)
        if intensity_field is None:
            rc = self._lib.dmsa_dense_cloud_add_pointcloud2(self._dc, C.byref(cm), capi.SENSORS[sensor], capi.ptr(out, C.c_float), cap, C.byref(kept), C.byref(cs))
            return self._result(rc, "dmsa_dense_cloud_add_pointcloud2", out, kept, cs)
        f = _field(sensor_intensity_field(sensor) if isinstance(intensity_field, str) and intensity_field == "auto" else intensity_field)
        rc = self._lib.dmsa_dense_cloud_add_pointcloud2_field(self._dc, C.byref(cm), capi.SENSORS[sensor], C.byref(f), capi.ptr(out, C.c_float), cap, C.byref(kept),
                                                              C.byref(cs))
        return self._result(rc, "dmsa_dense_cloud_add_pointcloud2_field", out, kept, cs)

    def stats(self) -> dict:
        """Counters of all successful calls so far."""
        s = capi.DenseStats()
        self._check(self._lib.dmsa_dense_cloud_stats(self._dc, C.byref(s)), "dmsa_dense_cloud_stats")
        return _stats(s)

    def reserve(self, points: int):
        self._check(self._lib.dmsa_dense_cloud_reserve(self._dc, int(points)), "dmsa_dense_cloud_reserve")

    def table_info(self):
        """(slots, occupied) of the voxel table."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_table_info(self._dc, C.byref(a), C.byref(b)), "dmsa_dense_cloud_table_info")
        return int(a.value), int(b.value)

    def open_pcd(self, path):
        self._check(self._lib.dmsa_dense_cloud_open_pcd(self._dc, str(path).encode()), "dmsa_dense_cloud_open_pcd")

    def close_pcd(self):
        """(points, bytes) of the file (12-byte x y z rows; 16-byte x y z intensity rows on an intensity object: I7).  Raises DmsaError when no point was written (the file is removed: PCL refuses an empty cloud)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_close_pcd(self._dc, C.byref(a), C.byref(b)), "dmsa_dense_cloud_close_pcd")
        return int(a.value), int(b.value)

    # ---- include/dmsa_dense_normals.h ----
    def retain(self):
        """N0: legal only before the first scan."""
        self._check(self._lib.dmsa_dense_cloud_retain(self._dc), "dmsa_dense_cloud_retain")

    def retained_count(self) -> int:
        t = C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_retained(self._dc, 0, 0, None, None, C.byref(t)), "dmsa_dense_cloud_retained")
        return int(t.value)

    def retained(self, first: int = 0, count: int | None = None):
        """Rows [first, first + count) of the store (count None: to its end): (xyz (m,4), origin (m,4)) float32, w = 1 -- on an
        intensity object the w of an xyz row is its intensity (I6); origins keep 1."""
        if count is None:
            count = self.retained_count() - int(first)
        xyz, org = np.zeros((max(count, 1), 4), np.float32), np.zeros((max(count, 1), 4), np.float32)
        self._check(self._lib.dmsa_dense_cloud_retained(self._dc, int(first), int(count), capi.ptr(xyz, C.c_float), capi.ptr(org, C.c_float), None),
                    "dmsa_dense_cloud_retained")
        return xyz[:count], org[:count]

    @staticmethod
    def _normals_cfg(radius, min_neighbours):
        return capi.DenseNormalsConfig(float(np.float32(radius)), int(min_neighbours))

    def neighbour_moments(self, radius: float, first: int = 0, count: int | None = None) -> np.ndarray:
        """N2-N3 for rows [first, first + count): (m,10) int64 = n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz."""
        cfg = self._normals_cfg(radius, 0)
        if count is None:
            count = self.retained_count() - int(first)
        out = np.zeros((max(count, 1), 10), np.int64)
        self._check(self._lib.dmsa_dense_cloud_neighbour_moments(self._dc, C.byref(cfg), int(first), int(count), capi.ptr(out, C.c_int64)),
                    "dmsa_dense_cloud_neighbour_moments")
        return out[:count]

    def compute_normals(self, radius: float = 0.3, min_neighbours: int = 5, download: bool = True):
        """N2-N4 for every retained row: ((total,4) float32 = nx, ny, nz, curvature -- None with download=False --, rows with fewer than
        max(3, min_neighbours) neighbours: their four values are NaN)."""
        cfg = self._normals_cfg(radius, min_neighbours)
        out = np.zeros((max(self.retained_count(), 1), 4), np.float32) if download else None
        total, without = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_compute_normals(self._dc, C.byref(cfg), capi.ptr(out, C.c_float), C.byref(total), C.byref(without)),
                    "dmsa_dense_cloud_compute_normals")
        return (out[: int(total.value)] if out is not None else None), int(without.value)

    def save_pcd_normals(self, path):
        """N5: (points, bytes) of the seven-field file (eight fields, with `intensity` after z, on an intensity object: I7).  Needs
        compute_normals() since the last added scan."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_save_pcd_normals(self._dc, str(path).encode(), C.byref(a), C.byref(b)), "dmsa_dense_cloud_save_pcd_normals")
        return int(a.value), int(b.value)

    # ---- include/dmsa_dense_outliers.h ----
    @staticmethod
    def _outlier_cfg(radius, k, stddev_mul):
        return capi.DenseOutlierConfig(float(np.float32(radius)), int(k), float(np.float32(stddev_mul)), 0)

    def knn_mean_distance(self, radius: float = 0.3, k: int = 8, first: int = 0, count: int | None = None) -> np.ndarray:
        """O2-O3 for rows [first, first + count): (m,) float32, the mean distance to the k nearest retained rows within `radius`; NaN = fewer
        than k such rows (isolated)."""
        cfg = self._outlier_cfg(radius, k, 0.0)
        if count is None:
            count = self.retained_count() - int(first)
        out = np.zeros(max(count, 1), np.float32)
        self._check(self._lib.dmsa_dense_cloud_knn_mean_distance(self._dc, C.byref(cfg), int(first), int(count), capi.ptr(out, C.c_float)),
                    "dmsa_dense_cloud_knn_mean_distance")
        return out[:count]

    def classify_outliers(self, radius: float = 0.3, k: int = 8, stddev_mul: float = 1.0, download: bool = False):
        """O2-O5 for every retained row: the statistics as a dict (rows, isolated, above_threshold, inliers, n_s, s1, s2, mean_m, stddev_m,
        threshold_m); with download=True (statistics, flags (rows,) uint8 with 1 = inlier).  The flags stay on the device for
        remove_outliers() until the next scan is added."""
        cfg = self._outlier_cfg(radius, k, stddev_mul)
        flags = np.zeros(max(self.retained_count(), 1), np.uint8) if download else None
        st = capi.DenseOutlierStats()
        self._check(self._lib.dmsa_dense_cloud_classify_outliers(self._dc, C.byref(cfg), capi.ptr(flags, C.c_uint8), C.byref(st)), "dmsa_dense_cloud_classify_outliers")
        stats = {n: (float if n.endswith("_m") else int)(getattr(st, n)) for n in OUTLIER_STAT_NAMES}
        return (stats, flags[: stats["rows"]]) if download else stats

    def remove_outliers(self) -> int:
        """O6: the store compacted to the inliers of the last classify_outliers(); returns the rows left.  Grid, normals and the classification
        are invalid afterwards; the voxel set and stats() are untouched."""
        kept = C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_remove_outliers(self._dc, C.byref(kept)), "dmsa_dense_cloud_remove_outliers")
        return int(kept.value)

    def save_pcd_retained(self, path):
        """(points, bytes) of the x y z binary PCD of the retained store as it stands (x y z intensity on an intensity object: I7)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_save_pcd_retained(self._dc, str(path).encode(), C.byref(a), C.byref(b)), "dmsa_dense_cloud_save_pcd_retained")
        return int(a.value), int(b.value)

    # ---- include/dmsa_dense_carve.h ----
    def carve_walk_rows(self, cfg: DenseCarveConfig | None = None, first: int = 0, count: int | None = None):
        """The stage call of T2-T4 for rows [first, first + count): (cells traversed (m,) int32 with -1 = skipped ray, the header's hash of the
        cell sequence (m,) uint64), as the device walks them."""
        c = (cfg or DenseCarveConfig()).to_c()
        if count is None:
            count = self.retained_count() - int(first)
        cells, hashes = np.zeros(max(count, 1), np.int32), np.zeros(max(count, 1), np.uint64)
        self._check(self._lib.dmsa_dense_cloud_carve_walk_rows(self._dc, C.byref(c), int(first), int(count), capi.ptr(cells, C.c_int32), capi.ptr(hashes, C.c_uint64)),
                    "dmsa_dense_cloud_carve_walk_rows")
        return cells[:count], hashes[:count]

    def count_passes(self, cfg: DenseCarveConfig | None = None, download: bool = False):
        """T2-T6 for every retained row: the statistics as a dict (rows, rays_walked, rays_skipped, cells_traversed, pair_tests, seen_through,
        transient, kept); with download=True (statistics, passes (rows,) uint32).  The flags stay on the device for remove_transients() until
        a scan is added or the store is compacted."""
        c = (cfg or DenseCarveConfig()).to_c()
        passes = np.zeros(max(self.retained_count(), 1), np.uint32) if download else None
        st = capi.DenseCarveStats()
        self._check(self._lib.dmsa_dense_cloud_count_passes(self._dc, C.byref(c), capi.ptr(passes, C.c_uint32), C.byref(st)), "dmsa_dense_cloud_count_passes")
        stats = {n: int(getattr(st, n)) for n in CARVE_STAT_NAMES}
        return (stats, passes[: stats["rows"]]) if download else stats

    def remove_transients(self) -> int:
        """T7: the store compacted to the rows the last count_passes() did not call transient; returns the rows left.  Grid, normals and both
        classifications are invalid afterwards; the voxel set and stats() are untouched."""
        kept = C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_remove_transients(self._dc, C.byref(kept)), "dmsa_dense_cloud_remove_transients")
        return int(kept.value)

    # ---- include/dmsa_dense_occupancy.h ----
    def build_occupancy(self, cfg: DenseOccupancyConfig | None = None) -> dict:
        """M2-M5 for every retained row: the statistics as a dict (rows, rays_walked, rays_skipped, cells_traversed, cells_out_of_range, cells,
        occupied, free, unknown, table_slots, table_builds).  The map stays on the device until a scan is added or the store is compacted."""
        c = (cfg or DenseOccupancyConfig()).to_c()
        st = capi.DenseOccupancyStats()
        self._check(self._lib.dmsa_dense_cloud_build_occupancy(self._dc, C.byref(c), C.byref(st)), "dmsa_dense_cloud_build_occupancy")
        return {n: int(getattr(st, n)) for n in OCCUPANCY_STAT_NAMES}

    def occupancy_count(self) -> int:
        t = C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_occupancy_cells(self._dc, 0, 0, None, None, None, None, C.byref(t)), "dmsa_dense_cloud_occupancy_cells")
        return int(t.value)

    def occupancy_cells(self, first: int = 0, count: int | None = None):
        """Cells [first, first + count) of M4's listing (count None: to its end): (cells (m,3) int32, hits (m,) uint32, passes (m,) uint32,
        state (m,) uint8)."""
        if count is None:
            count = self.occupancy_count() - int(first)
        k = max(count, 1)
        cells, hits, passes, state = np.zeros((k, 3), np.int32), np.zeros(k, np.uint32), np.zeros(k, np.uint32), np.zeros(k, np.uint8)
        self._check(self._lib.dmsa_dense_cloud_occupancy_cells(self._dc, int(first), int(count), capi.ptr(cells, C.c_int32), capi.ptr(hits, C.c_uint32),
                                                               capi.ptr(passes, C.c_uint32), capi.ptr(state, C.c_uint8), None), "dmsa_dense_cloud_occupancy_cells")
        return cells[:count], hits[:count], passes[:count], state[:count]

    def save_pcd_occupancy(self, path, min_state: int = 0) -> int:
        """M6: the rows written to the six-field file: the map cells whose state is >= min_state."""
        rows = C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_save_pcd_occupancy(self._dc, str(path).encode(), int(min_state), C.byref(rows)), "dmsa_dense_cloud_save_pcd_occupancy")
        return int(rows.value)

    def occupancy_slice(self, z_lo: float, z_hi: float):
        """M7: (info as a dict: width, height, cx_min, cy_min, origin_x, origin_y and the pixels of each value, pixels (height, width) uint8 with
        0 occupied, 254 free, 205 unknown; row 0 is the largest y)."""
        info = capi.DenseOccupancySliceInfo()
        lo, hi = float(np.float32(z_lo)), float(np.float32(z_hi))
        self._check(self._lib.dmsa_dense_cloud_occupancy_slice(self._dc, lo, hi, C.byref(info), None, 0), "dmsa_dense_cloud_occupancy_slice")
        pixels = np.zeros((info.height, info.width), np.uint8)
        self._check(self._lib.dmsa_dense_cloud_occupancy_slice(self._dc, lo, hi, C.byref(info), capi.ptr(pixels, C.c_uint8), pixels.size), "dmsa_dense_cloud_occupancy_slice")
        return {n: (float if n.startswith("origin") else int)(getattr(info, n)) for n in OCCUPANCY_SLICE_NAMES}, pixels

    def save_occupancy_map(self, pgm_path, yaml_path, z_lo: float, z_hi: float):
        """M7: map.pgm and map.yaml as the ROS map_server loads them."""
        self._check(self._lib.dmsa_dense_cloud_save_occupancy_map(self._dc, str(pgm_path).encode(), str(yaml_path).encode(), float(np.float32(z_lo)),
                                                                  float(np.float32(z_hi))), "dmsa_dense_cloud_save_occupancy_map")

    # ---- include/dmsa_dense_surface.h ----
    def build_surface(self, cfg: DenseSurfaceConfig | None = None) -> dict:
        """S2-S6 for every retained row: the statistics as a dict (rows, rays_walked, rays_skipped, cells_traversed, cells_out_of_range, cells,
        cells_valid, table_slots, table_builds).  The volume stays on the device until a scan is added or the store is compacted."""
        c = (cfg or DenseSurfaceConfig()).to_c()
        st = capi.DenseSurfaceStats()
        self._check(self._lib.dmsa_dense_cloud_build_surface(self._dc, C.byref(c), C.byref(st)), "dmsa_dense_cloud_build_surface")
        return {n: int(getattr(st, n)) for n in SURFACE_STAT_NAMES}

    def surface_count(self) -> int:
        t = C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_surface_cells(self._dc, 0, 0, None, None, None, C.byref(t)), "dmsa_dense_cloud_surface_cells")
        return int(t.value)

    def mesh_counts(self):
        """(vertices, triangles) of the extracted mesh."""
        v, t = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_mesh_vertices(self._dc, 0, 0, None, C.byref(v)), "dmsa_dense_cloud_mesh_vertices")
        self._check(self._lib.dmsa_dense_cloud_mesh_triangles(self._dc, 0, 0, None, C.byref(t)), "dmsa_dense_cloud_mesh_triangles")
        return int(v.value), int(t.value)

    def surface_cells(self, first: int = 0, count: int | None = None):
        """Cells [first, first + count) of S6's listing (count None: to its end): (cells (m,3) int32, sum (m,) int64, n (m,) uint32)."""
        if count is None:
            count = self.surface_count() - int(first)
        k = max(count, 1)
        cells, total, weight = np.zeros((k, 3), np.int32), np.zeros(k, np.int64), np.zeros(k, np.uint32)
        self._check(self._lib.dmsa_dense_cloud_surface_cells(self._dc, int(first), int(count), capi.ptr(cells, C.c_int32), capi.ptr(total, C.c_int64),
                                                             capi.ptr(weight, C.c_uint32), None), "dmsa_dense_cloud_surface_cells")
        return cells[:count], total[:count], weight[:count]

    def save_pcd_tsdf(self, path) -> int:
        """S7: the rows written to the x y z tsdf weight file: the cells of the volume."""
        rows = C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_save_pcd_tsdf(self._dc, str(path).encode(), C.byref(rows)), "dmsa_dense_cloud_save_pcd_tsdf")
        return int(rows.value)

    def extract_mesh(self, min_weight: int = 2) -> dict:
        """S8 of the built volume: the statistics as a dict (tetrahedra_meshed, vertices, triangles).  The mesh stays on the device and replaces
        the one of an earlier call."""
        st = capi.DenseMeshStats()
        self._check(self._lib.dmsa_dense_cloud_extract_mesh(self._dc, int(min_weight), C.byref(st)), "dmsa_dense_cloud_extract_mesh")
        return {n: int(getattr(st, n)) for n in MESH_STAT_NAMES}

    def mesh_vertices(self, first: int = 0, count: int | None = None):
        """Vertices [first, first + count) of the extracted mesh (count None: to its end): (m,3) float32."""
        if count is None:
            count = self.mesh_counts()[0] - int(first)
        xyz = np.zeros((max(count, 1), 3), np.float32)
        self._check(self._lib.dmsa_dense_cloud_mesh_vertices(self._dc, int(first), int(count), capi.ptr(xyz, C.c_float), None), "dmsa_dense_cloud_mesh_vertices")
        return xyz[:count]

    def mesh_triangles(self, first: int = 0, count: int | None = None):
        """Triangles [first, first + count) of the extracted mesh (count None: to its end): (m,3) int32 vertex indices."""
        if count is None:
            count = self.mesh_counts()[1] - int(first)
        tri = np.zeros((max(count, 1), 3), np.int32)
        self._check(self._lib.dmsa_dense_cloud_mesh_triangles(self._dc, int(first), int(count), capi.ptr(tri, C.c_int32), None), "dmsa_dense_cloud_mesh_triangles")
        return tri[:count]

    def save_ply_mesh(self, path):
        """S9: the extracted mesh as a binary little-endian PLY."""
        self._check(self._lib.dmsa_dense_cloud_save_ply_mesh(self._dc, str(path).encode()), "dmsa_dense_cloud_save_ply_mesh")

    # ---- include/dmsa_dense_clusters.h ----
    @staticmethod
    def _cluster_cfg(radius, min_size, max_size):
        return capi.DenseClusterConfig(float(np.float32(radius)), int(min_size), int(max_size), 0)

    def cluster_labels(self, radius: float = 0.3):
        """C2-C3 for every retained row: (label (rows,) int32 = the smallest row of the row's cluster, size (rows,) int32 = the rows of that
        cluster).  The labels stay on the device for save_pcd_labels() until a scan is added or the store is compacted."""
        cfg = self._cluster_cfg(radius, 1, 0)
        n = self.retained_count()
        label, size = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        self._check(self._lib.dmsa_dense_cloud_cluster_labels(self._dc, C.byref(cfg), capi.ptr(label, C.c_int32), capi.ptr(size, C.c_int32)),
                    "dmsa_dense_cloud_cluster_labels")
        return label[:n], size[:n]

    def classify_clusters(self, radius: float = 0.3, min_size: int = 50, max_size: int = 0, download: bool = False):
        """C2-C5 for every retained row: the statistics as a dict (rows, clusters, largest, kept_rows, kept_clusters, small_rows, large_rows);
        with download=True (statistics, flags (rows,) uint8 with 1 = kept).  The flags stay on the device for remove_clusters() until a scan
        is added or the store is compacted."""
        cfg = self._cluster_cfg(radius, min_size, max_size)
        flags = np.zeros(max(self.retained_count(), 1), np.uint8) if download else None
        st = capi.DenseClusterStats()
        self._check(self._lib.dmsa_dense_cloud_classify_clusters(self._dc, C.byref(cfg), capi.ptr(flags, C.c_uint8), C.byref(st)), "dmsa_dense_cloud_classify_clusters")
        stats = {n: int(getattr(st, n)) for n in CLUSTER_STAT_NAMES}
        return (stats, flags[: stats["rows"]]) if download else stats

    def remove_clusters(self) -> int:
        """C6: the store compacted to the rows the last classify_clusters() kept; returns the rows left.  Labels, grid, normals and every
        classification are invalid afterwards; the voxel set and stats() are untouched."""
        kept = C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_remove_clusters(self._dc, C.byref(kept)), "dmsa_dense_cloud_remove_clusters")
        return int(kept.value)

    def save_pcd_labels(self, path):
        """C7: (points, bytes) of the x y z label binary PCD of the store (x y z intensity label on an intensity object).  Needs
        cluster_labels() or classify_clusters() of the store as it stands."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_save_pcd_labels(self._dc, str(path).encode(), C.byref(a), C.byref(b)), "dmsa_dense_cloud_save_pcd_labels")
        return int(a.value), int(b.value)

    # ---- include/dmsa_dense_compare.h ----
    # (the defaults, ten voxels and one voxel of the demo's 0.1 m, come from no recorded data: placeholders like min_size above)
    @staticmethod
    def _compare_cfg(max_distance, tolerance, keep="near"):
        if keep not in capi.COMPARE_KEEP:
            raise ValueError(f"keep must be one of {sorted(capi.COMPARE_KEEP)}")
        return capi.DenseCompareConfig(float(np.float32(max_distance)), float(np.float32(tolerance)), capi.COMPARE_KEEP[keep], 0)

    def set_reference(self, xyz, transform=None):
        """D0: the reference cloud of this object, (n,k) float32 rows with k >= 3 of which x y z are read; transform = a 3x4 (or 4x4, its upper
        rows) rigid alignment into the map frame, applied on the device.  Replaces the reference; an empty array drops it."""
        xyz = np.asarray(xyz, np.float32)
        if xyz.ndim != 2 or (xyz.shape[0] > 0 and xyz.shape[1] < 3):
            raise ValueError("the reference must be (n,k) with k >= 3")
        xyz = np.ascontiguousarray(xyz)
        t = None if transform is None else np.ascontiguousarray(np.asarray(transform, np.float64)[:3, :4])
        if t is not None and t.shape != (3, 4):
            raise ValueError("the transform must be 3x4 or 4x4")
        self._check(self._lib.dmsa_dense_cloud_set_reference(self._dc, capi.ptr(xyz, C.c_float) if xyz.shape[0] else None, xyz.shape[0], max(xyz.shape[1], 3),
                                                             capi.ptr(t, C.c_double) if t is not None else None), "dmsa_dense_cloud_set_reference")

    def reference_count(self) -> int:
        total = C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_reference(self._dc, 0, 0, None, None, C.byref(total)), "dmsa_dense_cloud_reference")
        return int(total.value)

    def reference(self, first: int = 0, count: int | None = None):
        """Rows [first, first + count) of the reference as transformed: (xyz (count,3) float32, valid (count,) uint8)."""
        if count is None:
            count = self.reference_count() - first
        xyz, valid = np.zeros((max(count, 1), 3), np.float32), np.zeros(max(count, 1), np.uint8)
        self._check(self._lib.dmsa_dense_cloud_reference(self._dc, int(first), int(count), capi.ptr(xyz, C.c_float), capi.ptr(valid, C.c_uint8), None),
                    "dmsa_dense_cloud_reference")
        return xyz[:count], valid[:count]

    def _nearest(self, call, total, max_distance, first, count):
        if count is None:
            count = total() - first
        cfg = self._compare_cfg(max_distance, max_distance)
        dist, index = np.zeros(max(count, 1), np.float32), np.zeros(max(count, 1), np.int32)
        self._check(getattr(self._lib, call)(self._dc, C.byref(cfg), int(first), int(count), capi.ptr(dist, C.c_float), capi.ptr(index, C.c_int32)), call)
        return dist[:count], index[:count]

    def nearest_in_reference(self, max_distance: float = 1.0, first: int = 0, count: int | None = None):
        """D2-D3, ACCURACY: (dist (count,) float32, index (count,) int32) of store rows [first, first + count): the nearest valid reference row
        within max_distance (NaN and -1 without one)."""
        return self._nearest("dmsa_dense_cloud_nearest_in_reference", self.retained_count, max_distance, first, count)

    def nearest_in_store(self, max_distance: float = 1.0, first: int = 0, count: int | None = None):
        """D2-D3, COMPLETENESS: the same for reference rows [first, first + count) against the store (an invalid row: NaN and -1)."""
        return self._nearest("dmsa_dense_cloud_nearest_in_store", self.reference_count, max_distance, first, count)

    def compare(self, max_distance: float = 1.0, tolerance: float = 0.1) -> dict:
        """D2-D5, both directions over all rows: rows, ref_rows, ref_invalid, scale, bin_width_m, precision, recall, f_score and per direction
        ("accuracy", "completeness") queries, matched, unmatched, within, s1, s2, histogram (64 ints), mean_m, rms_m, fraction_within.  The
        accuracy distances stay on the device for save_pcd_distance()."""
        cfg = self._compare_cfg(max_distance, tolerance)
        st = capi.DenseCompareStats()
        self._check(self._lib.dmsa_dense_cloud_compare(self._dc, C.byref(cfg), C.byref(st)), "dmsa_dense_cloud_compare")
        return _compare_stats(st)

    def classify_by_reference(self, max_distance: float = 1.0, tolerance: float = 0.1, keep: str = "near", download: bool = False):
        """D6: keep="near" keeps the rows with a reference row within `tolerance`, keep="far" the others.  The statistics of the accuracy
        direction as compare() gives them plus `kept`; with download=True (statistics, flags (rows,) uint8).  The flags stay on the device for
        remove_by_reference()."""
        cfg = self._compare_cfg(max_distance, tolerance, keep)
        flags = np.zeros(max(self.retained_count(), 1), np.uint8) if download else None
        st = capi.DenseCompareStats()
        self._check(self._lib.dmsa_dense_cloud_classify_by_reference(self._dc, C.byref(cfg), capi.ptr(flags, C.c_uint8), C.byref(st)),
                    "dmsa_dense_cloud_classify_by_reference")
        stats = _compare_stats(st)
        return (stats, flags[: stats["rows"]]) if download else stats

    def remove_by_reference(self) -> int:
        """D6: the store compacted to the rows the last classify_by_reference() kept; returns the rows left.  The reference stays."""
        kept = C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_remove_by_reference(self._dc, C.byref(kept)), "dmsa_dense_cloud_remove_by_reference")
        return int(kept.value)

    def save_pcd_distance(self, path):
        """D7: (points, bytes) of the x y z distance binary PCD of the store (x y z intensity distance on an intensity object).  Needs compare()
        or classify_by_reference() of the store and the reference as they stand."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.dmsa_dense_cloud_save_pcd_distance(self._dc, str(path).encode(), C.byref(a), C.byref(b)), "dmsa_dense_cloud_save_pcd_distance")
        return int(a.value), int(b.value)

    # ---- include/dmsa_dense_align.h ----
    # (the defaults come from a synthetic room, not from recorded data: placeholders)
    def align_reference(self, xyz, transform=None, max_distance: float = 1.0, max_iterations: int = 30, min_pairs: int | None = None, stop_translation: float = 1e-4,
                        stop_rotation: float = 1e-5, metric: str = "point") -> dict:
        """A0-A8: the reference rows xyz ((n,k) float32, k >= 3) aligned to the store by ICP from `transform` (3x4 or 4x4; None: the identity).
        Returns transform (3,4) float64, iterations, stop ("CONVERGED", "MAX_ITERATIONS", "TOO_FEW_PAIRS"), scale_c, history (per iteration
        matched, unmatched, s2, rms_m, shift_m, rotation_rad) and sums (the last iteration's, as align_sums() gives them).  Afterwards the object
        holds what set_reference(xyz, transform=result) would have left.  min_pairs None: 3.
        metric="plane": P0-P9 of include/dmsa_dense_align_plane.h, the residual along the store's normals (compute_normals() first); stop may
        also be "DEGENERATE", a history entry also has used, no_normal, plane_rms_m and min_pivot, sums are as align_plane_sums() gives them,
        min_pairs None: 6."""
        if metric not in ("point", "plane"):
            raise ValueError("metric must be 'point' or 'plane'")
        plane = metric == "plane"
        if min_pairs is None:
            min_pairs = 6 if plane else 3
        xyz = np.asarray(xyz, np.float32)
        if xyz.ndim != 2 or xyz.shape[1] < 3:
            raise ValueError("the reference must be (n,k) with k >= 3")
        xyz = np.ascontiguousarray(xyz)
        t = None if transform is None else np.ascontiguousarray(np.asarray(transform, np.float64)[:3, :4])
        if t is not None and t.shape != (3, 4):
            raise ValueError("the transform must be 3x4 or 4x4")
        kinds = (capi.DenseAlignPlaneConfig, capi.DenseAlignPlaneReport, "dmsa_dense_cloud_align_reference_plane", capi.ALIGN_PLANE_STOP, _align_plane_sums) if plane else (
            capi.DenseAlignConfig, capi.DenseAlignReport, "dmsa_dense_cloud_align_reference", capi.ALIGN_STOP, _align_sums)
        fields = (float(np.float32(max_distance)), int(max_iterations), int(min_pairs), 0, float(stop_translation), float(stop_rotation))
        return self._align_reference(xyz, t, fields, *kinds)

    def _align_reference(self, xyz, t, cfg_fields, config_type, report_type, entry, stop_names, read_sums) -> dict:
        cfg, rep, out = config_type(*cfg_fields), report_type(), np.zeros((3, 4), np.float64)
        self._check(getattr(self._lib, entry)(self._dc, capi.ptr(xyz, C.c_float) if xyz.shape[0] else None, xyz.shape[0], xyz.shape[1],
                                              capi.ptr(t, C.c_double) if t is not None else None, C.byref(cfg), capi.ptr(out, C.c_double), C.byref(rep)), entry)
        history = [{name: (int if kind is C.c_int64 else float)(getattr(h, name)) for name, kind in type(h)._fields_} for h in rep.history[: rep.iterations]]
        return dict(transform=out, iterations=int(rep.iterations), stop=stop_names[rep.stop], scale_c=float(rep.scale_c), history=history, sums=read_sums(rep.sums))

    def _stage_sums(self, max_distance, with_d4, config_type, least_pairs, words, entry, read_sums):
        cfg = config_type(float(np.float32(max_distance)), 1, least_pairs, 0, 0.0, 0.0)
        sums = (C.c_int64 * words)()
        d4 = capi.DenseCompareDirection()
        self._check(getattr(self._lib, entry)(self._dc, C.byref(cfg), sums, C.byref(d4)), entry)
        return (read_sums(sums), _compare_direction(d4)) if with_d4 else read_sums(sums)

    def align_sums(self, max_distance: float = 1.0, with_d4: bool = False):
        """The stage call: A2's exact sums of the reference as it stands (set_reference) against the store, Python ints: n, sp, sg and spg (the
        nine cross sums recombined).  with_d4=True: (sums, D4's block of the same pairs as compare() gives a direction)."""
        return self._stage_sums(max_distance, with_d4, capi.DenseAlignConfig, 3, capi.ALIGN_SUMS, "dmsa_dense_cloud_align_sums", _align_sums)

    # ---- include/dmsa_dense_align_plane.h ----
    def align_plane_sums(self, max_distance: float = 1.0, with_d4: bool = False):
        """The stage call: P2's exact sums of the reference as it stands (set_reference) against the store and its normals (compute_normals),
        Python ints: n, no_normal, sp, nn, cn, cc, ne, ce, ee (the limbs recombined).  with_d4=True: (sums, D4's block of all matched pairs as
        compare() gives a direction)."""
        return self._stage_sums(max_distance, with_d4, capi.DenseAlignPlaneConfig, 6, capi.ALIGN_PLANE_SUMS, "dmsa_dense_cloud_align_plane_sums", _align_plane_sums)
