"""Model of C2-C7 of include/dmsa_dense_clusters.h, independent of any grid and of any union-find.

C2  adjacent_pairs: candidates from scipy.spatial.cKDTree at 1.001 * radius in double (a superset: float32 rounding moves a distance by parts
    in 10^7, not in 10^3), each re-tested with N2's float32 expression, operation for operation, against float32(r * r).  So it scales to
    10^6 rows.  adjacent_pairs_brute tests every pair (the _deltas of tests/dense_normals_model.py) for the small clouds.
C3  labels: scipy.sparse.csgraph.connected_components, then the smallest row and the number of rows per component.
C4  keep, C5 classify: numpy comparisons and Python-int counts.
C7  file_bytes: the header written out here, and the rows as little-endian records."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

import dense_normals_model as nm

f32 = np.float32


def r2_of(radius):
    r = f32(radius)
    return f32(r * r)


def _d2(g, i, j):
    """N2's float32 expression for the pairs (i, j): d = g_j - g_i."""
    g = np.ascontiguousarray(np.asarray(g, f32)[:, :3])
    d = g[j] - g[i]
    d2 = d[:, 0] * d[:, 0]
    d2 = d2 + d[:, 1] * d[:, 1]
    d2 = d2 + d[:, 2] * d[:, 2]
    return d2


def adjacent_pairs(g, radius):
    """(m,2) int64, i < j, sorted: the pairs of C2."""
    xyz = np.asarray(g, f32)[:, :3].astype(np.float64)
    if xyz.shape[0] < 2:
        return np.zeros((0, 2), np.int64)
    cand = cKDTree(xyz).query_pairs(1.001 * float(f32(radius)), output_type="ndarray").astype(np.int64).reshape(-1, 2)
    cand = np.stack([cand.min(axis=1), cand.max(axis=1)], axis=1)
    pairs = cand[_d2(g, cand[:, 0], cand[:, 1]) <= r2_of(radius)]
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]


def adjacent_pairs_brute(g, radius, chunk=256):
    """The same from every pair of rows."""
    n = np.asarray(g).shape[0]
    out = []
    for a in range(0, n, chunk):
        rows = np.arange(a, min(a + chunk, n))
        _, d2 = nm._deltas(g, rows)
        i, j = np.nonzero(d2 <= r2_of(radius))
        i = i + a
        out.append(np.stack([i[i < j], j[i < j]], axis=1))
    pairs = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))].astype(np.int64)


def labels_of_pairs(n, pairs):
    """C3: (label (n,) int32, size (n,) int32)."""
    graph = coo_matrix((np.ones(pairs.shape[0], np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    count, comp = connected_components(graph, directed=False)
    first = np.full(count, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return first[comp].astype(np.int32), np.bincount(comp, minlength=count)[comp].astype(np.int32)


def labels(g, radius, brute=False):
    pairs = adjacent_pairs_brute(g, radius) if brute else adjacent_pairs(g, radius)
    return labels_of_pairs(np.asarray(g).shape[0], pairs)


def keep(size, min_size, max_size=0):
    """C4: (n,) uint8."""
    size = np.asarray(size)
    return ((size >= min_size) & ((max_size == 0) | (size <= max_size))).astype(np.uint8)


def classify(g, radius, min_size, max_size=0, brute=False):
    """(flags (n,) uint8 with 1 = kept, statistics as the dict DenseCloudCreator.classify_clusters returns, label, size)."""
    label, size = labels(g, radius, brute)
    flags = keep(size, min_size, max_size)
    n = int(label.shape[0])
    head = label == np.arange(n)
    small = size < min_size
    large = (size > max_size) if max_size != 0 else np.zeros(n, bool)
    stats = dict(rows=n, clusters=int(head.sum()), largest=int(size.max()) if n else 0, kept_rows=int(flags.sum()), kept_clusters=int((head & (flags == 1)).sum()),
                 small_rows=int(small.sum()), large_rows=int(large.sum()))
    return flags, stats, label, size


def header(n, intensity=False):
    """C7."""
    extra = ("intensity ", "4 ", "F ", "1 ") if intensity else ("", "", "", "")
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z %slabel\nSIZE 4 4 4 %s4\nTYPE F F F %sU\nCOUNT 1 1 1 %s1\n" % extra +
            "WIDTH %012d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %012d\nDATA binary\n" % (n, n))


def row_dtype(intensity=False):
    names = ["x", "y", "z"] + (["intensity"] if intensity else []) + ["label"]
    return np.dtype([(k, "<u4" if k == "label" else "<f4") for k in names])


def file_bytes(g, label, intensity=False):
    """C7: the whole file of the store g (n,4) with its labels."""
    g = np.asarray(g, f32)
    rows = np.zeros(g.shape[0], row_dtype(intensity))
    rows["x"], rows["y"], rows["z"], rows["label"] = g[:, 0], g[:, 1], g[:, 2], np.asarray(label).astype(np.uint32)
    if intensity:
        rows["intensity"] = g[:, 3]
    return header(g.shape[0], intensity).encode() + rows.tobytes()


def read_file(path, intensity=False):
    """(header text, rows as a structured array, file size)."""
    raw = open(path, "rb").read()
    end = raw.index(b"DATA binary\n") + len(b"DATA binary\n")
    return raw[:end].decode(), np.frombuffer(raw[end:], row_dtype(intensity)), len(raw)
