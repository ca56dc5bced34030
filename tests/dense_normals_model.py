"""numpy model of N0-N4 of include/dmsa_dense_normals.h, independent of any grid: brute-force float32 distances, np.rint, int64 sums.

N0  RetainModel: the DenseModel of tests/dense_cloud_model.py that also returns the sensor origin of every survivor.
N2  neighbour_mask: every pair tested with the stated float32 expression.
N3  moments: the ten int64 sums.
N4  is NOT modelled a second time: the library's host function dmsa_dense_normal_from_moments is checked against numpy.linalg.eigh in
    tests/test_dense_normals_cpu.py (eigh_normal below), and the GPU tests compare the device with that host function on the model's moments."""
import numpy as np

import dense_cloud_model as dm

f32 = np.float32
GRID = dm.GRID


class RetainModel(dm.DenseModel):
    """add_scan_retained: rules 1-7 as DenseModel.add_scan, plus the origin o = rule 5 for the sensor-frame point (0, 0, 0) with each survivor's pose."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.ret_g, self.ret_o = np.zeros((0, 4), f32), np.zeros((0, 4), f32)

    def add_scan_retained(self, xyz, stamps, interpolate=None):
        poses = {}

        def recording(t):
            pose, seg = (interpolate or self.interpolate)(t)
            poses["t"], poses["pose"], poses["seg"] = np.array(t, np.float64), pose, seg
            return pose, seg

        seen = self.seen.copy()
        g, st = self.add_scan(xyz, stamps, interpolate=recording)
        # the origins of every point that reached rule 5, then the same survivors picked again
        pose = poses["pose"][poses["seg"] >= 0].astype(f32)
        rows = np.concatenate([pose[:, :9].reshape(-1, 3, 3), pose[:, 9:, None]], axis=2)
        zero = np.zeros(pose.shape[0], f32)
        qx, qy, qz = dm.apply_row3(self.l2i[:3], zero, zero, zero)
        o = np.stack(dm.apply_row3(rows, qx, qy, qz) + [np.ones(pose.shape[0], f32)], axis=1).astype(f32)
        # the placed points again, to know which of them survived rule 6
        xyz = np.asarray(xyz, f32)
        ti = np.asarray(stamps, np.float64).reshape(-1)
        with np.errstate(all="ignore"):
            x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
            finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(ti)
            r = np.sqrt(x * x + (y * y + z * z))
            t = ti + self.time_offset
            live = np.flatnonzero(finite & (r > self.min_range) & ((self.max_range <= 0) | (r < self.max_range)) & (t >= self.s[0]) & (t <= self.s[-1]))
        assert np.array_equal(t[live], poses["t"])
        live = live[poses["seg"] >= 0]
        px, py, pz = dm.apply_row3(self.l2i[:3], x[live], y[live], z[live])
        with np.errstate(all="ignore"):
            g_all = np.stack(dm.apply_row3(rows, px, py, pz) + [np.ones(live.shape[0], f32)], axis=1).astype(f32)
        keep = np.ones(live.shape[0], bool)
        if self.voxel > 0:
            with np.errstate(all="ignore"):
                c = np.floor(g_all[:, :3] / self.voxel)
                ok = ((c >= -GRID) & (c < GRID)).all(axis=1)
            ci = np.where(ok[:, None], c, 0).astype(np.int64) + GRID
            key = (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]
            first = np.zeros(key.shape[0], bool)
            idx_ok = np.flatnonzero(ok)
            first[idx_ok[np.unique(key[ok], return_index=True)[1]]] = True
            keep = ok & first & ~np.isin(key, seen)
        assert np.array_equal(g_all[keep].view(np.uint32), g.view(np.uint32))
        self.ret_g, self.ret_o = np.concatenate([self.ret_g, g]), np.concatenate([self.ret_o, o[keep]])
        return g, o[keep], st


def scale_of(radius):
    """N3: frexpf(radius) = m * 2^e; scale = 2^(20 - e)."""
    _, e = np.frexp(f32(radius))
    return f32(2.0 ** (20 - int(e)))


def _deltas(g, rows):
    g = np.ascontiguousarray(np.asarray(g, f32)[:, :3])
    d = g[None, :, :] - g[rows, None, :]  # d = g_j - g_i, float32
    d2 = d[..., 0] * d[..., 0]
    d2 = d2 + d[..., 1] * d[..., 1]
    d2 = d2 + d[..., 2] * d[..., 2]
    return d, d2


def neighbour_mask(g, radius, rows=None):
    """(len(rows), n) bool: N2 for the query rows (default: all)."""
    n = np.asarray(g).shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    r = f32(radius)
    _, d2 = _deltas(g, rows)
    return d2 <= f32(r * r)


def moments(g, radius, rows=None, chunk=256):
    """(len(rows), 10) int64: n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz of N3."""
    n = np.asarray(g).shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    r, scale = f32(radius), scale_of(radius)
    out = np.zeros((rows.shape[0], 10), np.int64)
    for a in range(0, rows.shape[0], chunk):
        d, d2 = _deltas(g, rows[a : a + chunk])
        inside = d2 <= f32(r * r)
        with np.errstate(invalid="ignore", over="ignore"):
            q = np.where(inside[..., None], np.rint(d * scale), 0).astype(np.int64)
        x, y, z = q[..., 0], q[..., 1], q[..., 2]
        o = out[a : a + chunk]
        o[:, 0] = inside.sum(axis=1)
        for k, v in enumerate((x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
            o[:, 1 + k] = v.sum(axis=1)
    return out


def view_vectors(g, o):
    """w = o_i - g_i in float32."""
    return (np.asarray(o, f32)[:, :3] - np.asarray(g, f32)[:, :3]).astype(f32)


def eigh_normal(m):
    """float64 reference of N4 for one row of moments: (unit normal up to sign, curvature, eigenvalues ascending)."""
    m = [float(int(v)) for v in m]
    n, s = m[0], np.array(m[1:4])
    S = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]])
    cov = (S - np.outer(s, s) / n) / n
    w, v = np.linalg.eigh(cov)
    return v[:, 0], abs(w[0] / w.sum()), w
