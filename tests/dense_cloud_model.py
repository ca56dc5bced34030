"""numpy model of rules 1-7 of include/dmsa_dense_cloud.h: the yardstick of the GPU tests of the dense cloud (tests/test_gpu_dense_cloud.py).
Written from the header's statement of the rules, with numpy's own sin / arccos / arctan2: it shares no code with the library.
tests/test_dense_cloud_model.py holds it against scipy's Slerp."""
import numpy as np

f32 = np.float32
STAT_NAMES = ("points_in", "kept", "non_finite", "out_of_range", "out_of_time", "in_gap", "out_of_grid", "thinned")
GRID = 1 << 20


def normalise_xyzw(q):
    q = np.asarray(q, np.float64).reshape(-1, 4)
    return q / np.sqrt((q * q).sum(axis=1))[:, None]


def slerp_axis_angle(q1, q2, u):
    """Axis-angle (n,3) of slerp(q1, q2, u) for unit quaternions (n,4) in (w, x, y, z) order: the shorter arc (q2 negated when the dot
    product is negative), linear weights when the two are equal to within an ulp."""
    one = 1.0 - np.finfo(np.float64).eps
    d = (q1 * q2).sum(axis=1)
    ad = np.abs(d)
    lin = ad >= one
    th = np.arccos(np.minimum(ad, 1.0))
    sn = np.where(lin, 1.0, np.sin(th))
    s0 = np.where(lin, 1.0 - u, np.sin((1.0 - u) * th) / sn)
    s1 = np.where(lin, u, np.sin(u * th) / sn)
    s1 = np.where(d < 0.0, -s1, s1)
    q = s0[:, None] * q1 + s1[:, None] * q2
    n = np.sqrt((q[:, 1:] ** 2).sum(axis=1))
    angle = 2.0 * np.arctan2(n, np.abs(q[:, 0]))
    n = np.where(q[:, 0] < 0.0, -n, n)
    safe = np.where(n == 0.0, 1.0, n)
    return np.where((n == 0.0)[:, None], 0.0, q[:, 1:] / safe[:, None] * angle[:, None])


def so3_exp(w):
    """Rodrigues, (n,3) -> (n,9) row-major; the identity below 1e-5 rad."""
    th = np.sqrt((w * w).sum(axis=1))
    small = th < 1e-5
    tt = np.where(small, 1.0, th)
    s = np.sin(tt) / tt
    sh = np.sin(0.5 * tt)
    c = 2.0 * sh * sh / (tt * tt)
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    t2 = tt * tt
    R = np.stack([1.0 + c * (x * x - t2), c * x * y - s * z, c * x * z + s * y,
                  c * x * y + s * z, 1.0 + c * (y * y - t2), c * y * z - s * x,
                  c * x * z - s * y, c * y * z + s * x, 1.0 + c * (z * z - t2)], axis=1)
    R[small] = np.eye(3).reshape(-1)
    return R


def apply_row3(rows, x, y, z):
    """((c0*x + c1*y) + c2*z) + c3 per row in float32; rows: (3,4) or (n,3,4)."""
    rows = np.asarray(rows, f32)
    r = rows if rows.ndim == 3 else rows[None]
    return [((r[:, k, 0] * x + r[:, k, 1] * y) + r[:, k, 2] * z) + r[:, k, 3] for k in range(3)]


class DenseModel:
    def __init__(self, stamps, pos, quat_xyzw, lidar_to_imu=None, min_range=0.0, max_range=0.0, time_offset=0.0, max_pose_gap=0.0, voxel_size=0.0):
        self.s = np.asarray(stamps, np.float64)
        self.p = np.asarray(pos, np.float64).reshape(-1, 3)
        q = normalise_xyzw(quat_xyzw)
        self.q = np.concatenate([q[:, 3:], q[:, :3]], axis=1)  # (w, x, y, z)
        self.l2i = np.eye(4, dtype=f32) if lidar_to_imu is None else np.asarray(lidar_to_imu, f32)
        self.min_range, self.max_range, self.voxel = f32(min_range), f32(max_range), f32(voxel_size)
        self.time_offset, self.max_gap = float(time_offset), float(max_pose_gap)
        self.seen = np.zeros(0, np.int64)  # voxel keys of the scans so far
        self.total = dict.fromkeys(STAT_NAMES, 0)

    def interpolate(self, t):
        """(pose12 (n,12), segment (n,)): rules 3-4 for the stamps t as they are."""
        t = np.asarray(t, np.float64).reshape(-1)
        n, n_p = t.shape[0], self.s.shape[0]
        pose, seg = np.zeros((n, 12)), np.full(n, -1, np.int32)
        with np.errstate(invalid="ignore"):
            inside = (t >= self.s[0]) & (t <= self.s[-1])
        j = np.clip(np.searchsorted(self.s, t[inside], side="right") - 1, 0, n_p - 2)
        ds = self.s[j + 1] - self.s[j]
        gap = (ds > self.max_gap) if self.max_gap > 0.0 else np.zeros(j.shape, bool)
        seg[inside] = np.where(gap, -2, j)
        ok = np.flatnonzero(inside)[~gap]
        j, ds = j[~gap], ds[~gap]
        u = (t[ok] - self.s[j]) / ds
        pose[ok, :9] = so3_exp(slerp_axis_angle(self.q[j], self.q[j + 1], u))
        pose[ok, 9:] = self.p[j] + u[:, None] * (self.p[j + 1] - self.p[j])
        return pose, seg

    def add_scan(self, xyz, stamps, interpolate=None, commit=True):
        """(kept (m,4) float32 with w = 1, stats of the call).  `interpolate`: where the poses come from (default: this model's own) -- the
        bit-for-bit tests pass the device's stage call, so that what is compared is everything BUT the fp64 trigonometry."""
        interpolate = interpolate or self.interpolate
        xyz = np.asarray(xyz, f32)
        x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        ti = np.asarray(stamps, np.float64).reshape(-1)
        n = x.shape[0]
        st = dict.fromkeys(STAT_NAMES, 0)
        st["points_in"] = n
        with np.errstate(all="ignore"):
            finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(ti)
            r = np.sqrt(x * x + (y * y + z * z))
            in_range = (r > self.min_range) & ((self.max_range <= 0) | (r < self.max_range))
            t = ti + self.time_offset
            in_time = (t >= self.s[0]) & (t <= self.s[-1])
        st["non_finite"] = int((~finite).sum())
        st["out_of_range"] = int((finite & ~in_range).sum())
        st["out_of_time"] = int((finite & in_range & ~in_time).sum())
        live = np.flatnonzero(finite & in_range & in_time)
        pose, seg = interpolate(t[live])
        st["in_gap"] = int((seg == -2).sum())
        assert not (seg == -1).any()
        live, pose = live[seg >= 0], pose[seg >= 0].astype(f32)
        px, py, pz = apply_row3(self.l2i[:3], x[live], y[live], z[live])
        rows = np.concatenate([pose[:, :9].reshape(-1, 3, 3), pose[:, 9:, None]], axis=2)
        with np.errstate(all="ignore"):
            g = np.stack(apply_row3(rows, px, py, pz) + [np.ones(live.shape[0], f32)], axis=1).astype(f32)
        if self.voxel > 0:
            with np.errstate(all="ignore"):
                c = np.floor(g[:, :3] / self.voxel)
                ok = ((c >= -GRID) & (c < GRID)).all(axis=1)
            st["out_of_grid"] = int((~ok).sum())
            g, c = g[ok], c[ok].astype(np.int64) + GRID
            key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
            first = np.zeros(key.shape[0], bool)
            first[np.unique(key, return_index=True)[1]] = True  # the lowest index of every voxel of this scan
            keep = first & ~np.isin(key, self.seen)
            st["thinned"] = int((~keep).sum())
            g = g[keep]
            if commit:
                self.seen = np.concatenate([self.seen, key[keep]])
        st["kept"] = g.shape[0]
        assert st["points_in"] == sum(st[k] for k in STAT_NAMES[1:])
        if commit:
            for k in STAT_NAMES:
                self.total[k] += st[k]
        return g, st
