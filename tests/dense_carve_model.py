"""The independent model of include/dmsa_dense_carve.h (T2-T7), the yardstick of tests/test_dense_carve_cpu.py and tests/test_gpu_dense_carve.py.

T3 in np.float64, T4 in Python ints, T5 in np.float32 one operation at a time, T6 in Python-int counts.  The only structure is a dict from
cell to rows.  `sees_through` is T5 on scalars; `count_passes` runs the same operations on the float32 arrays of a cell's rows at once (each
numpy operation rounds every element on its own, like the scalar one): tests/test_dense_carve_cpu.py checks the two against each other."""
import math
from dataclasses import dataclass

import numpy as np

f32 = np.float32
f64 = np.float64
UNIT, W, MAX_EXTENT, BIAS = 1024, 2048, 2048, 1 << 20
HASH_SEED, HASH_MUL, M64 = 0xCBF29CE484222325, 0x100000001B3, (1 << 64) - 1
STAT_NAMES = ("rows", "rays_walked", "rays_skipped", "cells_traversed", "pair_tests", "seen_through", "transient", "kept")


@dataclass
class Config:
    cell_size: float = 0.2
    rho: float = 0.1
    tan_half_angle: float = 0.052407779
    end_margin: float = 0.3
    start_margin: float = 0.5
    max_length: float = 30.0
    min_passes: int = 2

    def refused(self):
        """T1, the part that needs no store."""
        v = [f32(x) for x in (self.rho, self.end_margin, self.start_margin, self.max_length)]
        t = f32(self.tan_half_angle)
        return (not all(np.isfinite(x) for x in v) or not v[0] > 0 or not v[1] > 0 or not v[2] >= 0 or not v[3] > 0 or not (t > 0 and t <= 1)
                or not 1 <= int(self.min_passes) <= 2**20)


# ---- T2 ----
def ray(o, g):
    """(d (3,) float32, L2, L)."""
    o, g = np.asarray(o, f32), np.asarray(g, f32)
    with np.errstate(all="ignore"):
        d = [f32(g[a] - o[a]) for a in range(3)]
        l2 = f32(d[0] * d[0])
        l2 = f32(l2 + f32(d[1] * d[1]))
        l2 = f32(l2 + f32(d[2] * d[2]))
        return d, l2, f32(np.sqrt(l2))


# ---- T3 / T4 ----
def _axis(a, b, c):
    with np.errstate(all="ignore"):
        pa, pb = f64(a) / c, f64(b) / c
    if not abs(pa) < 2.0**31 or not abs(pb) < 2.0**31:
        return None
    fa, fb = int(math.floor(pa * f64(1024.0))), int(math.floor(pb * f64(1024.0)))
    xa, xb = 2 * fa + 1, 2 * fb + 1
    ca, cb = fa >> 10, fb >> 10
    if abs(cb - ca) > MAX_EXTENT:
        return None
    sign = (xb > xa) - (xb < xa)
    inside = xa - W * ca
    assert 0 < inside < W and inside % 2 == 1
    return dict(n=W - inside if sign > 0 else inside, d=abs(xb - xa), cell=ca, left=abs(cb - ca), sign=sign, end=cb)


def walk(cell_size, o, g, max_length=None):
    """The traversed cells of the ray o -> g, in order, as a list of (x, y, z); None for a skipped ray (max_length None: no length limit)."""
    _, l2, length = ray(o, g)
    if l2 == 0 or (max_length is not None and length > f32(max_length)):
        return None
    c = f64(f32(cell_size))
    ax = [_axis(f32(o[a]), f32(g[a]), c) for a in range(3)]
    if any(a is None for a in ax):
        return None
    cells = [tuple(a["cell"] for a in ax)]
    while any(a["left"] > 0 for a in ax):
        live = [a for a in ax if a["left"] > 0]
        best = live[0]
        for a in live[1:]:
            if a["n"] * best["d"] < best["n"] * a["d"]:
                best = a
        for a in [a for a in live if a["n"] * best["d"] == best["n"] * a["d"]]:  # every axis tied for the smallest
            a["cell"] += a["sign"]
            a["n"] += W
            a["left"] -= 1
        cells.append(tuple(a["cell"] for a in ax))
        assert len(cells) <= 3 * MAX_EXTENT + 1
    assert cells[-1] == tuple(a["end"] for a in ax)
    return cells


def hash_of(cells):
    h = HASH_SEED
    for cell in cells:
        for v in cell:
            h = ((h ^ ((v + BIAS) & M64)) * HASH_MUL) & M64
    return h


def cell_of(p, cell_size):
    c = f64(f32(cell_size))
    return tuple(int(math.floor(f64(f32(v)) / c)) for v in p[:3])


# ---- T5 ----
def pair_terms(o, g, p):
    """T5's intermediate values on scalars: dict(L, rem, perp2, s)."""
    d, _, length = ray(o, g)
    g, p = np.asarray(g, f32), np.asarray(p, f32)
    with np.errstate(all="ignore"):
        u = [f32(g[a] - p[a]) for a in range(3)]
        rem = f32(u[0] * d[0])
        rem = f32(rem + f32(u[1] * d[1]))
        rem = f32(rem + f32(u[2] * d[2]))
        rem = f32(rem / length)
        u2 = f32(u[0] * u[0])
        u2 = f32(u2 + f32(u[1] * u[1]))
        u2 = f32(u2 + f32(u[2] * u[2]))
        perp2 = f32(u2 - f32(rem * rem))
        s = f32(length - rem)
    return dict(L=length, rem=rem, perp2=perp2, s=s)


def sees_through(cfg, o, g, p):
    _, l2, length = ray(o, g)
    if l2 == 0 or length > f32(cfg.max_length):
        return False
    t = pair_terms(o, g, p)
    with np.errstate(all="ignore"):
        rho2 = f32(f32(cfg.rho) * f32(cfg.rho))
        w = f32(f32(cfg.tan_half_angle) * t["rem"])
        w2 = f32(w * w)
        return bool(t["s"] >= f32(cfg.start_margin) and t["rem"] >= f32(cfg.end_margin) and t["perp2"] <= rho2 and t["perp2"] <= w2)


def _sees_through_rows(cfg, d, length, g, pts):
    """T5 for the rows pts (m,3) float32 at once: (m,) bool."""
    with np.errstate(all="ignore"):
        ux, uy, uz = g[0] - pts[:, 0], g[1] - pts[:, 1], g[2] - pts[:, 2]
        rem = ux * d[0]
        rem = rem + uy * d[1]
        rem = rem + uz * d[2]
        rem = rem / length
        u2 = ux * ux
        u2 = u2 + uy * uy
        u2 = u2 + uz * uz
        perp2 = u2 - rem * rem
        s = length - rem
        w = f32(cfg.tan_half_angle) * rem
        assert rem.dtype == f32 and perp2.dtype == f32 and s.dtype == f32 and w.dtype == f32
        return (s >= f32(cfg.start_margin)) & (rem >= f32(cfg.end_margin)) & (perp2 <= f32(f32(cfg.rho) * f32(cfg.rho))) & (perp2 <= w * w)


# ---- T2-T6 ----
def walk_rows(g, o, cfg):
    """The stage call: (cells traversed (n,) int32 with -1 = skipped, hash (n,) uint64 with 0 for a skipped ray)."""
    n = g.shape[0]
    cells, hashes = np.zeros(n, np.int32), np.zeros(n, np.uint64)
    for r in range(n):
        path = walk(cfg.cell_size, o[r, :3], g[r, :3], cfg.max_length)
        cells[r], hashes[r] = (-1, 0) if path is None else (len(path), hash_of(path))
    return cells, hashes


def count_passes(g, o, cfg):
    """(passes (n,) uint32, the eight statistics as a dict of ints)."""
    g, o = np.ascontiguousarray(g[:, :3], f32), np.ascontiguousarray(o[:, :3], f32)
    n = g.shape[0]
    grid = {}
    for j in range(n):
        grid.setdefault(cell_of(g[j], cfg.cell_size), []).append(j)
    grid = {c: np.array(rows, np.int64) for c, rows in grid.items()}
    passes = [0] * n
    walked = skipped = traversed = tests = 0
    for r in range(n):
        path = walk(cfg.cell_size, o[r], g[r], cfg.max_length)
        if path is None:
            skipped += 1
            continue
        walked += 1
        traversed += len(path)
        d, _, length = ray(o[r], g[r])
        for cell in path:
            if not all(-BIAS <= v < BIAS for v in cell) or cell not in grid:
                continue
            rows = grid[cell]
            rows = rows[rows != r]
            tests += int(rows.size)
            for j in rows[_sees_through_rows(cfg, d, length, g[r], g[rows])]:
                passes[int(j)] += 1
    transient = sum(1 for v in passes if v >= int(cfg.min_passes))
    stats = dict(rows=n, rays_walked=walked, rays_skipped=skipped, cells_traversed=traversed, pair_tests=tests, seen_through=sum(passes), transient=transient,
                 kept=n - transient)
    return np.array(passes, np.uint32), stats
