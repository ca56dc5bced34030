"""The independent model of include/dmsa_dense_surface.h (S2-S9), the yardstick of tests/test_dense_surface_cpu.py and
tests/test_gpu_dense_surface.py.

S2 on the ray of tests/dense_carve_model.py, S3 in np.float32 one operation at a time, the walk on that model's axis set-up (T3 in np.float64,
T4 in Python ints), S4 in np.float32 on the arrays of a ray's cells (each numpy operation rounds every element on its own), the fusion in a dict
from cell to [sum, n] of Python ints, S7 and the vertex positions in np.float64 with one rounding to float32, S8 on corner masks in Python.  The
orientation of every (tetrahedron, inside set) case is derived here from S8's rule with integer numpy arrays.  Nothing here shares code with
the library.  The checks a closed mesh has to pass (edges, Euler characteristic, volume) are here too, for the model's meshes and the
device's."""
import itertools
from dataclasses import dataclass

import numpy as np

import dense_carve_model as cm

f32 = np.float32
f64 = np.float64
BIAS = 1 << 20
STAT_NAMES = ("rows", "rays_walked", "rays_skipped", "cells_traversed", "cells_out_of_range", "cells", "cells_valid")  # without the table's two
MESH_STAT_NAMES = ("tetrahedra_meshed", "vertices", "triangles")
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))  # xyz, xzy, yxz, yzx, zxy, zyx


@dataclass
class Config:
    cell_size: float = 0.2
    truncation: float = 0.6
    max_length: float = 30.0
    min_weight: int = 2
    initial_slots: int = 0

    def refused(self):
        """S1, the part that needs no store (cell_size: finite and > 0 only)."""
        c, t, length, s = f32(self.cell_size), f32(self.truncation), f32(self.max_length), int(self.initial_slots)
        with np.errstate(all="ignore"):
            return (not np.isfinite(c) or not c > 0 or not np.isfinite(t) or not t >= c or not t <= f32(f32(16.0) * c) or not np.isfinite(length) or not length > 0
                    or not 1 <= int(self.min_weight) <= 2**20 or not (s == 0 or (64 <= s <= 2**31 and s & (s - 1) == 0)))


def key_of(cell):
    return ((cell[0] + BIAS) << 42) | ((cell[1] + BIAS) << 21) | (cell[2] + BIAS)


# ---- S2-S3 ----
def segment(o, g, cfg):
    """None for a ray that S2 skips; else (a, b, d, L): the ends of the integrated segment, the ray's direction and length."""
    o, g = np.asarray(o, f32)[:3], np.asarray(g, f32)[:3]
    d, l2, length = cm.ray(o, g)
    if l2 == 0 or length > f32(cfg.max_length):
        return None
    trunc = f32(cfg.truncation)
    with np.errstate(all="ignore"):
        f = f32(trunc / length)
        p = [f32(f * d[a]) for a in range(3)]
        b = [f32(g[a] + p[a]) for a in range(3)]
        a = [f32(g[k] - p[k]) for k in range(3)] if length > trunc else [f32(o[k]) for k in range(3)]
    return a, b, d, length


def walk_segment(cell_size, a, b):
    """T3 / T4 for the segment a -> b (no test of its length): the traversed cells in order, or None where T2's third case refuses it."""
    c = f64(f32(cell_size))
    ax = [cm._axis(f32(a[k]), f32(b[k]), c) for k in range(3)]
    if any(v is None for v in ax):
        return None
    cells = [tuple(v["cell"] for v in ax)]
    while any(v["left"] > 0 for v in ax):
        live = [v for v in ax if v["left"] > 0]
        best = live[0]
        for v in live[1:]:
            if v["n"] * best["d"] < best["n"] * v["d"]:
                best = v
        for v in [v for v in live if v["n"] * best["d"] == best["n"] * v["d"]]:
            v["cell"] += v["sign"]
            v["n"] += cm.W
            v["left"] -= 1
        cells.append(tuple(v["cell"] for v in ax))
        assert len(cells) <= 3 * cm.MAX_EXTENT + 1
    assert cells[-1] == tuple(v["end"] for v in ax)
    return cells


# ---- S4 ----
def centre(c, cell_size):
    return f32((f64(int(c)) + f64(0.5)) * f64(f32(cell_size)))


def sample_q(g, d, length, cells, cfg):
    """q of the (k,3) cells for the ray ending at g with direction d and length L: (k,) int64."""
    g = np.asarray(g, f32)
    cell, trunc = f64(f32(cfg.cell_size)), f32(cfg.truncation)
    m = ((np.asarray(cells, np.int64).astype(f64) + f64(0.5)) * cell).astype(f32)
    with np.errstate(all="ignore"):
        u = [g[a] - m[:, a] for a in range(3)]
        s = u[0] * d[0]
        s = s + u[1] * d[1]
        s = s + u[2] * d[2]
        s = s / length
        s = np.minimum(np.maximum(s, -trunc), trunc)
        r = (s / trunc) * f32(32768.0)
        assert s.dtype == f32 and r.dtype == f32
        return np.rint(r).astype(np.int64)


def samples(o, g, cfg):
    """S2-S4 for one ray: None if it is skipped, else (cells inside the range (k,3) int32 in walk order, q (k,) int32, traversed, out of range)."""
    seg = segment(o, g, cfg)
    if seg is None:
        return None
    a, b, d, length = seg
    path = walk_segment(cfg.cell_size, a, b)
    if path is None:
        return None
    inside = [c for c in path if all(-BIAS <= v < BIAS for v in c)]
    cells = np.array(inside, np.int32).reshape(len(inside), 3)
    q = sample_q(np.asarray(g, f32)[:3], d, length, cells, cfg).astype(np.int32) if inside else np.zeros(0, np.int32)
    return cells, q, len(path), len(path) - len(inside)


# ---- S5-S6 ----
def accumulate(g, o, cfg):
    """(dict cell -> [sum, n], dict of the five walk statistics)."""
    g, o = np.ascontiguousarray(g[:, :3], f32), np.ascontiguousarray(o[:, :3], f32)
    field = {}
    walked = skipped = traversed = outside = 0
    for r in range(g.shape[0]):
        got = samples(o[r], g[r], cfg)
        if got is None:
            skipped += 1
            continue
        cells, q, n_path, n_out = got
        walked, traversed, outside = walked + 1, traversed + n_path, outside + n_out
        for cell, v in zip(map(tuple, cells.tolist()), q.tolist()):
            e = field.setdefault(cell, [0, 0])
            e[0] += v
            e[1] += 1
    return field, dict(rows=g.shape[0], rays_walked=walked, rays_skipped=skipped, cells_traversed=traversed, cells_out_of_range=outside)


def listing(field):
    """(cells (m,3) int32, sum (m,) int64, n (m,) uint32) in ascending key order."""
    cells = sorted(field, key=key_of)
    m = len(cells)
    return (np.array(cells, np.int32).reshape(m, 3), np.array([field[c][0] for c in cells], np.int64).reshape(m), np.array([field[c][1] for c in cells], np.uint32).reshape(m))


def build(g, o, cfg):
    """(the listing, the seven statistics the library is compared in)."""
    field, stats = accumulate(g, o, cfg)
    lst = listing(field)
    stats.update(cells=int(lst[2].size), cells_valid=int((lst[2] >= int(cfg.min_weight)).sum()))
    return lst, stats


# ---- S7 ----
def pcd_header(n):
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z tsdf weight\nSIZE 4 4 4 4 4\nTYPE F F F F U\nCOUNT 1 1 1 1 1\n"
            f"WIDTH {n:012d}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n:012d}\nDATA binary\n")


ROW = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("tsdf", "<f4"), ("weight", "<u4")])


def tsdf(total, n, truncation):
    return f32(((f64(int(total)) / f64(int(n))) / f64(32768.0)) * f64(f32(truncation)))


def pcd_bytes(lst, cfg):
    cells, total, n = lst
    rows = np.zeros(n.size, ROW)
    for a, name in enumerate("xyz"):
        rows[name] = [centre(c, cfg.cell_size) for c in cells[:, a]]
    rows["tsdf"] = [tsdf(s, w, cfg.truncation) for s, w in zip(total, n)]
    rows["weight"] = n
    return pcd_header(n.size).encode() + rows.tobytes()


# ---- S8 ----
def _offset(mask):
    return np.array([mask & 1, mask >> 1 & 1, mask >> 2 & 1], np.int64)


def chain_of(t):
    a, b, _ = PERMS[t]
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def case_triangles(inside):
    """The triangles of a tetrahedron whose inside chain positions are `inside` (a sorted tuple), before orientation: a list of triangles,
    each three edges (pairs of chain positions)."""
    outside = tuple(p for p in range(4) if p not in inside)
    if len(inside) in (0, 4):
        return []
    if len(inside) == 2:
        (A, B), (Cc, D) = inside, outside
        return [[(A, Cc), (A, D), (B, D)], [(A, Cc), (B, D), (B, Cc)]]
    alone = inside[0] if len(inside) == 1 else outside[0]
    return [[(alone, x) for x in range(4) if x != alone]]


def _derive_orientation():
    """flip[(t, inside)] = one bool per triangle of the case: S8's rule in doubled lattice coordinates, crossings at the edge midpoints."""
    flip = {}
    for t in range(6):
        corner = [2 * _offset(m) for m in chain_of(t)]
        for k in range(1, 4):
            for inside in itertools.combinations(range(4), k):
                outside = [p for p in range(4) if p not in inside]
                # (centroid of the outside corners - centroid of the inside ones) times both counts: an integer vector
                towards = len(inside) * sum(corner[p] for p in outside) - len(outside) * sum(corner[p] for p in inside)
                bits = []
                for tri in case_triangles(inside):
                    v = [(corner[i] + corner[j]) // 2 for i, j in tri]  # (doubled corners are even: the midpoint is an integer)
                    dot = int(np.dot(np.cross(v[1] - v[0], v[2] - v[0]), towards))
                    assert dot != 0
                    bits.append(dot < 0)
                flip[(t, inside)] = bits
    return flip


ORIENTATION = _derive_orientation()


def mesh(lst, cfg, min_weight):
    """(vertices (V,3) float32, triangles (F,3) int32, the three statistics) of S8."""
    cells, total, n = lst
    m = n.size
    index = {tuple(c): j for j, c in enumerate(cells.tolist())}
    valid = n >= int(min_weight)
    inside_node = valid & (total < 0)
    meshed = 0
    tris = []  # per triangle three vertex ids (lower node, class)
    for j in range(m):
        if not valid[j]:
            continue
        base = cells[j].astype(np.int64)
        node = [index.get(tuple((base + _offset(mask)).tolist()), -1) for mask in range(8)]
        ok = [at >= 0 and bool(valid[at]) for at in node]
        for t in range(6):
            chain = chain_of(t)
            if not all(ok[mask] for mask in chain):
                continue
            meshed += 1
            inside = tuple(p for p in range(4) if inside_node[node[chain[p]]])
            for tri, flip in zip(case_triangles(inside), ORIENTATION.get((t, inside), [])):
                ids = []
                for i, k in tri:
                    lo, hi = min(i, k), max(i, k)
                    assert chain[lo] & chain[hi] == chain[lo]
                    ids.append((node[chain[lo]], chain[hi] & ~chain[lo]))
                tris.append([ids[0], ids[2], ids[1]] if flip else ids)
    used = sorted({v for tri in tris for v in tri})
    place = {v: i for i, v in enumerate(used)}
    c = f64(f32(cfg.cell_size))
    xyz = np.zeros((len(used), 3), f32)
    for i, (lower, cls) in enumerate(used):
        off = _offset(cls)
        upper = index[tuple((cells[lower].astype(np.int64) + off).tolist())]
        m0, m1 = f64(int(total[lower])) / f64(int(n[lower])), f64(int(total[upper])) / f64(int(n[upper]))
        t = m0 / (m0 - m1)
        for a in range(3):
            xyz[i, a] = f32(((f64(int(cells[lower, a])) + f64(0.5)) + t * f64(int(off[a]))) * c)
    faces = np.array([[place[v] for v in tri] for tri in tris], np.int32).reshape(len(tris), 3)
    return xyz, faces, dict(tetrahedra_meshed=meshed, vertices=len(used), triangles=len(tris))


# ---- S9 ----
def ply_header(vertices, triangles):
    return (f"ply\nformat binary_little_endian 1.0\nelement vertex {vertices}\nproperty float x\nproperty float y\nproperty float z\nelement face {triangles}\n"
            "property list uchar int vertex_indices\nend_header\n")


FACE = np.dtype([("count", "u1"), ("i", "<i4", (3,))])


def ply_bytes(xyz, faces):
    rows = np.zeros(faces.shape[0], FACE)
    rows["count"], rows["i"] = 3, faces
    assert FACE.itemsize == 13
    return ply_header(xyz.shape[0], faces.shape[0]).encode() + np.ascontiguousarray(xyz, "<f4").tobytes() + rows.tobytes()


# ---- what a closed, consistently oriented mesh satisfies ----
def closed_manifold(faces):
    """True iff every directed edge of the triangles occurs exactly once and its reverse exactly once."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    directed = e[:, 0] * (1 << 32) + e[:, 1]
    mirrored = e[:, 1] * (1 << 32) + e[:, 0]
    return bool(np.unique(directed).size == directed.size and np.array_equal(np.sort(directed), np.sort(mirrored)))


def euler_characteristic(n_vertices, faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64), axis=1)
    return int(n_vertices) - int(np.unique(e, axis=0).shape[0]) + int(faces.shape[0])


def volume_towards(xyz, faces, sensor):
    """The volume enclosed on the side the normals point to, the sensor's: the sum over the triangles of N . (sensor - v0) / 6 with
    N = (v1 - v0) x (v2 - v0).  Positive iff the triangles face `sensor` on balance; for a closed mesh it does not depend on `sensor`, only its
    sign on which side the normals are."""
    v = np.asarray(xyz, f64)
    v0, v1, v2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float((np.cross(v1 - v0, v2 - v0) * (np.asarray(sensor, f64) - v0)).sum() / 6.0)
