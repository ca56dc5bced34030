"""The independent model of include/dmsa_dense_compare.h, D0-D7: the yardstick of tests/test_gpu_dense_compare.py.

Candidates come from scipy's cKDTree.query_ball_point at 1.001 * max_distance in double (a superset: a pair whose float32 d2 passes is at
most max_distance * (1 + 2^-22) apart); each is re-tested with N2's float32 expression, and the winner is the smallest (d2, row).  q, the
sums, the histogram and the summary are Python ints and floats.  A brute-force twin (every pair) serves the small clouds.  Nothing here knows
of cells, tiles or waves."""
import math

import numpy as np
from scipy.spatial import cKDTree

f32 = np.float32
NAN_BITS = 0x7FC00000
BINS = 64


def r2_of(r):
    return f32(r) * f32(r)


def d2_to(s, q):
    """N2's expression with d = s - q for the rows s (m,3) and one query q (3,), every operation in float32."""
    s = np.asarray(s, f32).reshape(-1, 3)
    q = np.asarray(q, f32)
    dx, dy, dz = s[:, 0] - q[0], s[:, 1] - q[1], s[:, 2] - q[2]
    d2 = dx * dx
    d2 = d2 + dy * dy
    d2 = d2 + dz * dz
    return d2.astype(f32)


def transform(xyz, T):
    """D0: rule 5's form with the twelve values of T cast to float32."""
    xyz = np.asarray(xyz, f32)[:, :3]
    if T is None:
        return xyz.copy()
    c = np.asarray(T, np.float64)[:3, :4].astype(f32)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.stack([((c[a, 0] * x + c[a, 1] * y).astype(f32) + c[a, 2] * z).astype(f32) + c[a, 3] for a in range(3)], axis=1).astype(f32)


def valid_rows(xyz, voxel):
    """D0: finite and inside rule 6's grid."""
    xyz = np.asarray(xyz, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor((xyz / f32(voxel)).astype(f32))
        ok = np.isfinite(xyz).all(axis=1) & (c >= -(2.0**20)).all(axis=1) & (c < 2.0**20).all(axis=1)
    return ok.astype(np.uint8)


def nearest(queries, s, max_distance, s_valid=None, q_valid=None, brute=False):
    """D2 for every query against the rows of s with s_valid set: (key_d2 (n,) float32 with NaN = no candidate, index (n,) int32 in the row
    numbers of s, -1 = none).  Queries with q_valid == 0 get NaN and -1."""
    queries, s = np.asarray(queries, f32)[:, :3], np.asarray(s, f32)[:, :3]
    rows = np.arange(s.shape[0]) if s_valid is None else np.flatnonzero(np.asarray(s_valid))
    pts = s[rows]
    r2 = r2_of(max_distance)
    n = queries.shape[0]
    d2_out, index = np.full(n, np.nan, f32), np.full(n, -1, np.int32)
    live = np.ones(n, bool) if q_valid is None else np.asarray(q_valid).astype(bool)
    tree = None if brute or pts.shape[0] == 0 else cKDTree(pts.astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in np.flatnonzero(live):
            if pts.shape[0] == 0:
                continue
            cand = np.arange(pts.shape[0]) if tree is None else np.asarray(sorted(tree.query_ball_point(queries[i].astype(np.float64), 1.001 * float(f32(max_distance)))), np.int64)
            if cand.size == 0:
                continue
            d2 = d2_to(pts[cand], queries[i])
            ok = d2 <= r2
            if not ok.any():
                continue
            cand, d2 = cand[ok], d2[ok]
            low = d2.min()
            d2_out[i], index[i] = low, rows[cand[d2 == low].min()]
    return d2_out, index


def dist_of(d2):
    """D2: sqrtf of the winner's d2, the quiet NaN 0x7FC00000 where there is none."""
    d2 = np.asarray(d2, f32)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(d2).astype(f32)
    d[np.isnan(d2)] = np.array([NAN_BITS], np.uint32).view(f32)[0]
    return d


def scale_of(max_distance):
    _, e = math.frexp(float(f32(max_distance)))
    return 2.0 ** (18 - e), e


def summary(matched, s1, s2, within, queries, scale):
    """D5 of one direction."""
    mean = float(s1) / float(matched) / scale if matched else 0.0
    rms = math.sqrt(float(s2) / float(matched)) / scale if matched else 0.0
    return mean, rms, (float(within) / float(queries) if queries else 0.0)


def direction(d2, counted, max_distance, tolerance):
    """D4-D5 of one direction from the winners' d2 (NaN = unmatched) of the queries with counted set."""
    scale, _ = scale_of(max_distance)
    d2 = np.asarray(d2, f32)
    counted = np.asarray(counted).astype(bool)
    got = counted & ~np.isnan(d2)
    q = [int(v) for v in np.rint(dist_of(d2[got]) * f32(scale)).astype(np.int64)]
    hist = [0] * BINS
    for v in q:
        hist[min(v >> 12, BINS - 1)] += 1
    out = dict(queries=int(counted.sum()), matched=len(q), unmatched=int((counted & np.isnan(d2)).sum()), within=int((d2[got] <= r2_of(tolerance)).sum()),
               s1=sum(q), s2=sum(v * v for v in q), histogram=hist)
    out["mean_m"], out["rms_m"], out["fraction_within"] = summary(out["matched"], out["s1"], out["s2"], out["within"], out["queries"], scale)
    return out


def _empty_direction():
    return dict(queries=0, matched=0, unmatched=0, within=0, s1=0, s2=0, histogram=[0] * BINS, mean_m=0.0, rms_m=0.0, fraction_within=0.0)


def compare(store, ref, ref_valid, max_distance=1.0, tolerance=0.1, brute=False):
    """dmsa_dense_cloud_compare as DenseCloudCreator.compare() returns it, plus the four arrays (d2 and index per direction)."""
    store, ref = np.asarray(store, f32)[:, :3], np.asarray(ref, f32)[:, :3]
    scale, e = scale_of(max_distance)
    a_d2, a_idx = nearest(store, ref, max_distance, s_valid=ref_valid, brute=brute)
    c_d2, c_idx = nearest(ref, store, max_distance, q_valid=ref_valid, brute=brute)
    acc = direction(a_d2, np.ones(store.shape[0], bool), max_distance, tolerance)
    com = direction(c_d2, ref_valid, max_distance, tolerance)
    p, r = acc["fraction_within"], com["fraction_within"]
    out = dict(rows=store.shape[0], ref_rows=ref.shape[0], ref_invalid=int(ref.shape[0] - np.asarray(ref_valid).astype(bool).sum()), kept=0, scale=scale,
               bin_width_m=2.0 ** (e - 6), precision=p, recall=r, f_score=(2.0 * p * r / (p + r) if p + r > 0.0 else 0.0), accuracy=acc, completeness=com)
    return out, (a_d2, a_idx, c_d2, c_idx)


def classify(store, ref, ref_valid, max_distance, tolerance, keep="near", brute=False):
    """D6 as classify_by_reference(download=True) returns it: (stats, flags), plus the accuracy d2."""
    store, ref = np.asarray(store, f32)[:, :3], np.asarray(ref, f32)[:, :3]
    scale, e = scale_of(max_distance)
    d2, _ = nearest(store, ref, max_distance, s_valid=ref_valid, brute=brute)
    with np.errstate(invalid="ignore"):
        confirmed = ~np.isnan(d2) & (d2 <= r2_of(tolerance))
    flags = (confirmed if keep == "near" else ~confirmed).astype(np.uint8)
    acc = direction(d2, np.ones(store.shape[0], bool), max_distance, tolerance)
    out = dict(rows=store.shape[0], ref_rows=ref.shape[0], ref_invalid=int(ref.shape[0] - np.asarray(ref_valid).astype(bool).sum()), kept=int(flags.sum()), scale=scale,
               bin_width_m=2.0 ** (e - 6), precision=acc["fraction_within"], recall=0.0, f_score=0.0, accuracy=acc, completeness=_empty_direction())
    return out, flags, d2


# ---- D7 ------------------------------------------------------------------------------------------------------------------------------------------------
def header(n, intensity=False):
    k = 5 if intensity else 4
    fields = "x y z intensity distance" if intensity else "x y z distance"
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS " + fields + "\nSIZE" + " 4" * k + "\nTYPE" + " F" * k + "\nCOUNT" + " 1" * k +
            "\nWIDTH %012d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %012d\nDATA binary\n" % (n, n))


def file_bytes(g, dist, intensity=False):
    """The file of D7 for the store rows g (n,4) and their distances."""
    g = np.asarray(g, f32)
    n = g.shape[0]
    body = np.zeros((n, 5 if intensity else 4), "<f4")
    body[:, :3] = g[:, :3]
    if intensity:
        body[:, 3] = g[:, 3]
    body[:, -1] = np.asarray(dist, f32)
    return header(n, intensity).encode() + body.tobytes()
