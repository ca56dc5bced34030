"""numpy model of I2-I7 of include/dmsa_dense_intensity.h on top of the existing models.

I3 / I6  IntensityModel: the DenseModel of tests/dense_cloud_model.py that also tells WHICH input rows survived.  The intensity never decides
         anything (I2), so the model of the value is an index: the survivor's w is the fourth float of input row kept_index, bit for bit.  The
         indices are recomputed here from the rules and checked against the rows the parent model returns.
I4       field_as_float32: numpy's astype(float32) of a structured view -- the C conversion under round-to-nearest-even.
I7       the two header texts, written out from the table of the header, and the rows of a file."""
import numpy as np

import dense_cloud_model as dm
import dense_normals_model as nm

f32 = np.float32
GRID = dm.GRID

# sensor_msgs/PointField datatype -> numpy type (little-endian)
DATATYPES = {1: "i1", 2: "u1", 3: "<i2", 4: "<u2", 5: "<i4", 6: "<u4", 7: "<f4", 8: "<f8"}


class IntensityModel(nm.RetainModel):
    """add_scan_indices: rules 1-7 as DenseModel.add_scan (and the origins of RetainModel), plus the input index of every survivor."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.ret_w = np.zeros(0, np.uint32)  # the bit patterns of the retained intensities

    def add_scan_indices(self, xyz, stamps, interpolate=None):
        """(kept (m,4) with w = the input's fourth float bit for bit, origins (m,4), input indices (m,), stats of the call)."""
        xyz = np.ascontiguousarray(xyz, f32)
        assert xyz.shape[1] == 4
        ti = np.asarray(stamps, np.float64).reshape(-1)
        seen = self.seen.copy()
        poses = {}

        def recording(t):
            pose, seg = (interpolate or self.interpolate)(t)
            poses["pose"], poses["seg"] = pose, seg
            return pose, seg

        g, o, st = self.add_scan_retained(xyz, ti, interpolate=recording)
        with np.errstate(all="ignore"):
            x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
            finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(ti)
            r = np.sqrt(x * x + (y * y + z * z))
            t = ti + self.time_offset
            live = np.flatnonzero(finite & (r > self.min_range) & ((self.max_range <= 0) | (r < self.max_range)) & (t >= self.s[0]) & (t <= self.s[-1]))
        live = live[poses["seg"] >= 0]
        pose = poses["pose"][poses["seg"] >= 0].astype(f32)
        rows = np.concatenate([pose[:, :9].reshape(-1, 3, 3), pose[:, 9:, None]], axis=2)
        px, py, pz = dm.apply_row3(self.l2i[:3], x[live], y[live], z[live])
        with np.errstate(all="ignore"):
            g_all = np.stack(dm.apply_row3(rows, px, py, pz), axis=1).astype(f32)
        keep = np.ones(live.shape[0], bool)
        if self.voxel > 0:
            with np.errstate(all="ignore"):
                c = np.floor(g_all / self.voxel)
                ok = ((c >= -GRID) & (c < GRID)).all(axis=1)
            ci = np.where(ok[:, None], c, 0).astype(np.int64) + GRID
            key = (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]
            first = np.zeros(key.shape[0], bool)
            idx_ok = np.flatnonzero(ok)
            first[idx_ok[np.unique(key[ok], return_index=True)[1]]] = True
            keep = ok & first & ~np.isin(key, seen)
        idx = live[keep]
        assert np.array_equal(g_all[keep].view(np.uint32), g[:, :3].view(np.uint32))  # the indices name the rows the parent model kept
        out = g.copy()
        out.view(np.uint32)[:, 3] = xyz.view(np.uint32)[idx, 3]
        self.ret_w = np.concatenate([self.ret_w, xyz.view(np.uint32)[idx, 3]])
        return out, o, idx, st


def field_as_float32(data, n, point_step, offset, datatype):
    """I4: the field of `datatype` at byte `offset` of each of the n points of the blob, as float32 by numpy's conversion."""
    blob = np.ascontiguousarray(data, np.uint8)[: n * point_step].reshape(n, point_step)
    dt = np.dtype(DATATYPES[datatype])
    raw = np.ascontiguousarray(blob[:, offset:offset + dt.itemsize]).view(dt).reshape(n)
    if datatype == 7:
        return raw.astype("<f4", copy=True)  # its bits pass through
    with np.errstate(over="ignore"):
        return raw.astype(f32)


def _header(fields, n):
    k = len(fields.split())
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS %s\nSIZE %s\nTYPE %s\nCOUNT %s\nWIDTH %012d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\n"
            "POINTS %012d\nDATA binary\n" % (fields, " ".join(["4"] * k), " ".join(["F"] * k), " ".join(["1"] * k), n, n))


def header_xyzi(n):
    return _header("x y z intensity", n)


def header_xyzi_normals(n):
    return _header("x y z intensity normal_x normal_y normal_z curvature", n)


def read_pcd(path):
    """(header dict, rows (points, fields) float32, the header's length, the file's size)"""
    raw = open(path, "rb").read()
    end = raw.index(b"DATA binary\n") + len(b"DATA binary\n")
    head = dict(line.split(" ", 1) for line in raw[:end].decode().splitlines()[1:])
    return head, np.frombuffer(raw[end:], "<f4").reshape(-1, len(head["FIELDS"].split())), end, len(raw)
