"""numpy model of O2-O5 of include/dmsa_dense_outliers.h, independent of any grid: brute-force float32 distances (the _deltas of
tests/dense_normals_model.py), the diagonal out, np.sort, a chained float32 sum, np.rint, Python-int sums, O5 in Python floats.

O2  every pair tested with N2's float32 expression; row i is not its own candidate (by index: a second row at the same place is).
O3  knn_mean_distance: the k smallest d2 of the candidates; sqrt of each, added in ascending order in float32, divided by float32(k).
O4  quantise / sums: q_i = rint(m_i * 2^(18 - e)); n_s, S1, S2 as Python integers.
O5  threshold: IEEE double arithmetic through Python floats, one operation per statement.
O6  classify: the flags; the filtered cloud is g[flags]."""
import math

import numpy as np

import dense_normals_model as nm

f32 = np.float32
QNAN_BITS = 0x7FC00000


def scale_of(radius):
    """O4: frexpf(radius) = m * 2^e; scale = 2^(18 - e)."""
    _, e = np.frexp(f32(radius))
    return f32(2.0 ** (18 - int(e)))


def knn_mean_distance(g, radius, k, rows=None, chunk=256):
    """(len(rows),) float32: m_i of O3, NaN (the quiet NaN 0x7FC00000) for an isolated row."""
    n = np.asarray(g).shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    r = f32(radius)
    r2 = f32(r * r)
    out = np.zeros(rows.shape[0], f32)
    for a in range(0, rows.shape[0], chunk):
        sel = rows[a : a + chunk]
        _, d2 = nm._deltas(g, sel)
        with np.errstate(invalid="ignore"):
            d2 = np.where(d2 <= r2, d2, f32(np.inf)).astype(f32)
        d2[np.arange(sel.shape[0]), sel] = f32(np.inf)  # j != i, by index
        if n < k + 1:
            d2 = np.concatenate([d2, np.full((sel.shape[0], k + 1 - n), np.inf, f32)], axis=1)
        part = np.sort(d2, axis=1)[:, :k]
        ok = np.isfinite(part[:, k - 1])
        root = np.sqrt(np.where(ok[:, None], part, f32(0))).astype(f32)
        acc = root[:, 0].copy()
        for u in range(1, k):
            acc = (acc + root[:, u]).astype(f32)
        m = (acc / f32(k)).astype(f32)
        m[~ok] = np.uint32(QNAN_BITS).view(f32)
        out[a : a + chunk] = m
    return out


def quantise(m, radius):
    """O4: q (int64, -1 for an isolated row)."""
    m = np.asarray(m, f32)
    iso = np.isnan(m)
    q = np.rint(np.where(iso, f32(0), m) * scale_of(radius)).astype(np.int64)
    q[iso] = -1
    return q


def sums(q):
    """(n_s, S1, S2) as Python integers."""
    live = [int(v) for v in np.asarray(q)[np.asarray(q) >= 0]]
    return len(live), sum(live), sum(v * v for v in live)


def threshold(n_s, s1, s2, stddev_mul):
    """O5: (mean, stddev, T) as Python floats (IEEE double, every operation rounded on its own)."""
    if n_s == 0:
        return 0.0, 0.0, 0.0
    n, a, b = float(n_s), float(s1), float(s2)
    mean = a / n
    var = 0.0
    if n_s >= 2:
        sq = a * a
        part = sq / n
        diff = b - part
        var = diff / float(n_s - 1)
        if var < 0.0:
            var = 0.0
    sd = math.sqrt(var)
    return mean, sd, mean + float(f32(stddev_mul)) * sd


def classify(g, radius, k, stddev_mul, chunk=256):
    """(flags (n,) uint8 with 1 = inlier, statistics as the dict DenseCloudCreator.classify_outliers returns, m (n,) float32)."""
    m = knn_mean_distance(g, radius, k, chunk=chunk)
    q = quantise(m, radius)
    n_s, s1, s2 = sums(q)
    mean, sd, t = threshold(n_s, s1, s2, stddev_mul)
    flags = ((q >= 0) & (q.astype(np.float64) <= t)).astype(np.uint8)
    scale = float(scale_of(radius))
    n = int(q.shape[0])
    isolated = int((q < 0).sum())
    stats = dict(rows=n, isolated=isolated, above_threshold=n - isolated - int(flags.sum()), inliers=int(flags.sum()), n_s=n_s, s1=s1, s2=s2, mean_m=mean / scale,
                 stddev_m=sd / scale, threshold_m=t / scale)
    return flags, stats, m
