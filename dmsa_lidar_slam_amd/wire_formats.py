"""Python mirror of the data formats either side of the path over include/dmsa_wire_formats.h: the per-sensor
sensor_msgs/PointCloud2 decoding of dmsa_slam_ros::callbackPointCloud (src/dmsa_slam_ros.cpp:374-486) on the device, and the TUM pose
lines of OutputManagement (OutputManagement.h:80-182) on the host, and the node's PointCloud.pcd (io::savePCDFileASCII,
src/dmsa_slam_ros.cpp:286-291, :495-506): header on the host, rows formatted on the device."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi as capi
from .api import DmsaError, DmsaOptimizer


@dataclass
class PointCloud2Msg:
    """The parts of a sensor_msgs/PointCloud2 the callback reads."""
    height: int
    width: int
    point_step: int
    field_offsets: np.ndarray   # msg.fields[i].offset
    data: np.ndarray            # uint8 blob
    stamp: float                # msg.header.stamp.toSec()

    def to_c(self, delta_t_pcs: float = 0.0) -> capi.PointCloud2:
        self.field_offsets = np.ascontiguousarray(self.field_offsets, np.uint32)
        self.data = np.ascontiguousarray(self.data, np.uint8)
        m = capi.PointCloud2()
        m.height, m.width, m.point_step, m.num_fields = int(self.height), int(self.width), int(self.point_step), int(self.field_offsets.shape[0])
        m.field_offsets = capi.ptr(self.field_offsets, C.c_uint32)
        m.data, m.data_bytes = self.data.ctypes.data_as(C.POINTER(C.c_uint8)), int(self.data.shape[0])
        m.stamp_msg, m.delta_t_pcs = float(self.stamp), float(delta_t_pcs)
        return m


class PointCloud2Decoder:
    """callbackPointCloud (:374-486) for one config.sensor; keeps lastPcMsgStamp like the node (read by sensor "unknown" only)."""

    def __init__(self, sensor: str, device: int = 0):
        if sensor not in capi.SENSORS:
            raise ValueError(f"unknown sensor type {sensor!r}; one of {sorted(capi.SENSORS)}")
        self._lib = capi.load_library()
        self.sensor = sensor
        self.lastPcMsgStamp = -1.0
        ctx = C.c_void_p()
        rc = self._lib.dmsa_create(device, 0, C.byref(ctx))
        if rc != capi.DMSA_OK:
            raise DmsaError(f"dmsa_create failed with {rc}: the decoder runs on the GPU, there is no CPU fallback")
        self._ctx = ctx

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.dmsa_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def decode(self, msg: PointCloud2Msg):
        """Returns (xyz (n,4) float32 with w = 0, stamps (n,) float64, ids (n,) int32), or None for the first message of an "unknown"
        sensor (the node only records its stamp, :388-392)."""
        if self.sensor == "unknown" and self.lastPcMsgStamp < 0.0:
            self.lastPcMsgStamp = msg.stamp
            return None
        delta = msg.stamp - self.lastPcMsgStamp  # :394 (lastPcMsgStamp is never updated afterwards in the reference)
        n = int(msg.height) * int(msg.width)
        xyz, st, ids = np.zeros((max(n, 1), 4), np.float32), np.zeros(max(n, 1)), np.zeros(max(n, 1), np.int32)
        cm = msg.to_c(delta)
        rc = self._lib.dmsa_decode_pointcloud2(self._ctx, C.byref(cm), capi.SENSORS[self.sensor], capi.ptr(xyz, C.c_float), capi.ptr(st, C.c_double),
                                               capi.ptr(ids, C.c_int32))
        if rc != capi.DMSA_OK:
            raise DmsaError(f"dmsa_decode_pointcloud2 failed with {rc}: {self._lib.dmsa_last_error(self._ctx).decode()}")
        return xyz[:n], st[:n], ids[:n]

    def decode_field(self, msg: PointCloud2Msg, field) -> np.ndarray:
        """dmsa_decode_pointcloud2_field (include/dmsa_dense_intensity.h, I4-I5): one typed field of every point as (n,) float32, decoded on
        the device.  field = (index into field_offsets, datatype), the datatype a sensor_msgs/PointField constant 1..8 or its name."""
        index, datatype = field
        f = capi.PointCloud2Field(int(index), int(capi.FIELD_DATATYPES.get(datatype, datatype)))
        n = int(msg.height) * int(msg.width)
        out = np.zeros(max(n, 1), np.float32)
        cm = msg.to_c(0.0)
        rc = self._lib.dmsa_decode_pointcloud2_field(self._ctx, C.byref(cm), C.byref(f), capi.ptr(out, C.c_float))
        if rc != capi.DMSA_OK:
            raise DmsaError(f"dmsa_decode_pointcloud2_field failed with {rc}: {self._lib.dmsa_last_error(self._ctx).decode()}")
        return out[:n]


def addPoseToFile(stamp: float, pos, orient) -> str:
    """OutputManagement::addPoseToFile (:80-96): one TUM line `stamp tx ty tz qx qy qz qw`."""
    lib = capi.load_library()
    p, o = np.ascontiguousarray(pos, np.float64), np.ascontiguousarray(orient, np.float64)
    buf = C.create_string_buffer(512)
    n = lib.dmsa_format_tum_pose(float(stamp), capi.ptr(p, C.c_double), capi.ptr(o, C.c_double), buf, 512)
    if n < 0:
        raise DmsaError(f"dmsa_format_tum_pose failed with {n}")
    return buf.raw[:n].decode()


def composeNonKeyframePose(keyframePos, keyframeOrient, Translation, Orientation):
    """saveDensePoses :148-153: pose of a non-keyframe scan from its pose relative to a keyframe."""
    lib = capi.load_library()
    a = [np.ascontiguousarray(v, np.float64) for v in (keyframePos, keyframeOrient, Translation, Orientation)]
    gp, go = np.zeros(3), np.zeros(3)
    rc = lib.dmsa_compose_nonkeyframe_pose(*[capi.ptr(v, C.c_double) for v in a], capi.ptr(gp, C.c_double), capi.ptr(go, C.c_double))
    if rc != capi.DMSA_OK:
        raise DmsaError(f"dmsa_compose_nonkeyframe_pose failed with {rc}")
    return gp, go


# ---- PointCloud.pcd ------------------------------------------------------------------------------------------------------------------
def pcdHeaderPointNormal(n: int) -> str:
    """pcl::PCDWriter::generateHeader of a PointCloud<PointNormal> with width = n, height = 1 (as PCL 1.10 writes it; recalled)."""
    lib = capi.load_library()
    buf = C.create_string_buffer(512)
    rc = lib.dmsa_pcd_header_pointnormal(int(n), buf, 512)
    if rc < 0:
        raise DmsaError(f"dmsa_pcd_header_pointnormal failed with {rc}")
    return buf.raw[:rc].decode()


class _PcdSource:
    """What the PCD functions take as the cloud: a DmsaOptimizer whose keyframe problem is resident (points and normals stay in HBM), or
    numpy arrays -- xyz (n,3|4), normals (n,3|4), optional curvature (n,); a private context formats them."""

    def __init__(self, source, normals=None, curvature=None):
        self._own = None
        if isinstance(source, DmsaOptimizer):
            if normals is not None or curvature is not None:
                raise ValueError("a resident cloud brings its own normals; pass arrays only")
            self.opt, self.n = source, source._num_points()
            self.xyz = self.nrm = self.cur = None
        else:
            if normals is None:
                raise ValueError("a cloud given as arrays needs xyz and normals")
            self.xyz, self.nrm = self._rows4(source), self._rows4(normals)
            self.cur = None if curvature is None else np.ascontiguousarray(curvature, np.float32).reshape(-1)
            self.n = self.xyz.shape[0]
            if self.nrm.shape[0] != self.n or (self.cur is not None and self.cur.shape[0] != self.n):
                raise ValueError("xyz, normals and curvature differ in length")
            self.opt = self._own = DmsaOptimizer()  # raises without a device: the rows are formatted on the GPU, there is no CPU fallback

    @staticmethod
    def _rows4(a):
        a = np.asarray(a, np.float32)
        if a.ndim != 2 or a.shape[1] not in (3, 4):
            raise ValueError("expected an (n,3) or (n,4) array")
        if a.shape[1] == 3:
            a = np.concatenate([a, np.zeros((a.shape[0], 1), np.float32)], axis=1)
        return np.ascontiguousarray(a)

    def pointers(self, first=0, n=None):
        n = self.n if n is None else n
        if self.xyz is None:
            return capi.ptr(None, C.c_float), capi.ptr(None, C.c_float), capi.ptr(None, C.c_float), first
        sl = slice(first, first + n)  # a host array holds the rows of the call themselves
        self._keep = (self.xyz[sl], self.nrm[sl], None if self.cur is None else self.cur[sl])
        return capi.ptr(self._keep[0], C.c_float), capi.ptr(self._keep[1], C.c_float), capi.ptr(self._keep[2], C.c_float), 0

    def close(self):
        if self._own is not None:
            self._own.close()


def formatPcdRows(source, normals=None, curvature=None, first: int = 0, n: int | None = None) -> bytes:
    """Rows first .. first + n - 1 of the PCD body: `x y z normal_x normal_y normal_z curvature\\n`, every value as printf("%.8g")."""
    src = _PcdSource(source, normals, curvature)
    try:
        n = src.n - first if n is None else int(n)
        if first < 0 or n < 0 or first + n > src.n:
            raise ValueError("rows outside the cloud")
        px, pn, pc, f = src.pointers(first, n)
        cap = 105 * n
        buf = C.create_string_buffer(max(cap, 1))
        used = C.c_int64(0)
        src.opt._check(src.opt._lib.dmsa_format_pcd_rows(src.opt._ctx, px, pn, pc, f, n, buf, cap, C.byref(used)), "dmsa_format_pcd_rows")
        return buf.raw[: used.value]
    finally:
        src.close()


def savePCDFileASCII(path, source, normals=None, curvature=None, chunk_rows: int = 0) -> int:
    """pcl::io::savePCDFileASCII(path, cloud) for a PointCloud<PointNormal>; returns the size of the file in bytes.  `chunk_rows`: rows per
    device chunk (0 = the library's default)."""
    src = _PcdSource(source, normals, curvature)
    try:
        px, pn, pc, _ = src.pointers()
        written = C.c_int64(0)
        src.opt._check(src.opt._lib.dmsa_save_pcd_ascii_ex(src.opt._ctx, str(path).encode(), px, pn, pc, src.n, int(chunk_rows), C.byref(written)),
                       "dmsa_save_pcd_ascii")
        return int(written.value)
    finally:
        src.close()
