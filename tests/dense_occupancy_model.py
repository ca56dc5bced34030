"""The independent model of include/dmsa_dense_occupancy.h (M2-M7), the yardstick of tests/test_dense_occupancy_cpu.py and
tests/test_gpu_dense_occupancy.py.

M2-M3 on the walk of tests/dense_carve_model.py (T3 in np.float64, T4 in Python ints), the counts in a dict from cell to [hits, passes], M5 in
Python ints (unbounded: no product can wrap), M6's coordinate in np.float64 with one rounding to float32, M7 in a dict from column to a set of
states.  Nothing here shares code with the library."""
import math
import os
from dataclasses import dataclass

import numpy as np

import dense_carve_model as cm

f32 = np.float32
f64 = np.float64
BIAS = 1 << 20
UNKNOWN, FREE, OCCUPIED = 0, 1, 2
STAT_NAMES = ("rows", "rays_walked", "rays_skipped", "cells_traversed", "cells_out_of_range", "cells", "occupied", "free", "unknown")  # without the table's two
PIXEL = {OCCUPIED: 0, FREE: 254, UNKNOWN: 205}


@dataclass
class Config:
    cell_size: float = 0.2
    max_length: float = 30.0
    min_hits: int = 1
    min_passes: int = 2
    occ_num: int = 16
    occ_den: int = 1
    initial_slots: int = 0

    def rule_refused(self):
        """M1, the four integers of M5."""
        return not all(1 <= int(v) <= 2**20 for v in (self.min_hits, self.min_passes, self.occ_num, self.occ_den))

    def refused(self):
        """M1, the part that needs no store."""
        length, s = f32(self.max_length), int(self.initial_slots)
        return not np.isfinite(length) or not length > 0 or self.rule_refused() or not (s == 0 or (64 <= s <= 2**31 and s & (s - 1) == 0))


# ---- M5 ----
def state(cfg, hits, passes):
    hits, passes = int(hits), int(passes)
    if hits >= int(cfg.min_hits) and passes * int(cfg.occ_den) <= hits * int(cfg.occ_num):
        return OCCUPIED
    return FREE if passes >= int(cfg.min_passes) else UNKNOWN


def key_of(cell):
    return ((cell[0] + BIAS) << 42) | ((cell[1] + BIAS) << 21) | (cell[2] + BIAS)


# ---- M2-M3 ----
def accumulate(g, o, cfg):
    """(dict cell -> [hits, passes], dict of the five walk statistics)."""
    g, o = np.ascontiguousarray(g[:, :3], f32), np.ascontiguousarray(o[:, :3], f32)
    counts = {}
    walked = skipped = traversed = outside = 0
    for r in range(g.shape[0]):
        path = cm.walk(cfg.cell_size, o[r], g[r], cfg.max_length)
        if path is None:
            skipped += 1
            continue
        walked += 1
        traversed += len(path)
        for i, cell in enumerate(path):
            if not all(-BIAS <= v < BIAS for v in cell):
                outside += 1
                continue
            counts.setdefault(cell, [0, 0])[0 if i == len(path) - 1 else 1] += 1
    return counts, dict(rows=g.shape[0], rays_walked=walked, rays_skipped=skipped, cells_traversed=traversed, cells_out_of_range=outside)


# ---- M4-M5 ----
def listing(counts, cfg):
    """(cells (m,3) int32, hits (m,) uint32, passes (m,) uint32, state (m,) uint8) in ascending key order."""
    cells = sorted(counts, key=key_of)
    m = len(cells)
    hits = np.array([counts[c][0] for c in cells], np.uint32).reshape(m)
    passes = np.array([counts[c][1] for c in cells], np.uint32).reshape(m)
    states = np.array([state(cfg, counts[c][0], counts[c][1]) for c in cells], np.uint8).reshape(m)
    return np.array(cells, np.int32).reshape(m, 3), hits, passes, states


def build(g, o, cfg):
    """(the listing, the nine statistics the library is compared in)."""
    counts, stats = accumulate(g, o, cfg)
    lst = listing(counts, cfg)
    st = lst[3]
    stats.update(cells=len(st), occupied=int((st == OCCUPIED).sum()), free=int((st == FREE).sum()), unknown=int((st == UNKNOWN).sum()))
    return lst, stats


# ---- M6 ----
def centre(c, cell_size):
    return f32((f64(int(c)) + f64(0.5)) * f64(f32(cell_size)))


def pcd_header(n):
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z hits passes state\nSIZE 4 4 4 4 4 4\nTYPE F F F U U U\nCOUNT 1 1 1 1 1 1\n"
            f"WIDTH {n:012d}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n:012d}\nDATA binary\n")


ROW = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("hits", "<u4"), ("passes", "<u4"), ("state", "<u4")])


def pcd_rows(lst, cfg, min_state=0):
    cells, hits, passes, states = lst
    take = np.flatnonzero(states >= min_state)
    rows = np.zeros(take.size, ROW)
    for a, name in enumerate("xyz"):
        rows[name] = [centre(cells[j, a], cfg.cell_size) for j in take]
    rows["hits"], rows["passes"], rows["state"] = hits[take], passes[take], states[take]
    return rows


def pcd_bytes(lst, cfg, min_state=0):
    rows = pcd_rows(lst, cfg, min_state)
    return pcd_header(rows.size).encode() + rows.tobytes()


# ---- M7 ----
def slab(z_lo, z_hi, cell_size):
    c = f64(f32(cell_size))
    return int(math.floor(f64(f32(z_lo)) / c)), int(math.floor(f64(f32(z_hi)) / c))


def slice_of(lst, cfg, z_lo, z_hi):
    """None where the slab has no column or the image is too large; else (info dict, pixels (height, width) uint8)."""
    cells, _, _, states = lst
    lo, hi = slab(z_lo, z_hi, cfg.cell_size)
    columns = {}
    for (x, y, z), s in zip(cells.tolist(), states.tolist()):
        if lo <= z <= hi:
            columns.setdefault((x, y), set()).add(s)
    if not columns:
        return None
    xs, ys = [k[0] for k in columns], [k[1] for k in columns]
    x_min, y_min, y_max = min(xs), min(ys), max(ys)
    width, height = max(xs) - x_min + 1, y_max - y_min + 1
    if width * height > 2**28:
        return None
    pixels = np.full((height, width), PIXEL[UNKNOWN], np.uint8)
    for (x, y), seen in columns.items():
        pixels[y_max - y, x - x_min] = PIXEL[OCCUPIED] if OCCUPIED in seen else PIXEL[FREE] if FREE in seen else PIXEL[UNKNOWN]
    c = f64(f32(cfg.cell_size))
    info = dict(width=width, height=height, cx_min=x_min, cy_min=y_min, origin_x=float(f64(x_min) * c), origin_y=float(f64(y_min) * c),
                occupied=int((pixels == 0).sum()), free=int((pixels == 254).sum()), unknown=int((pixels == 205).sum()))
    return info, pixels


def pgm_bytes(pixels):
    return f"P5\n{pixels.shape[1]} {pixels.shape[0]}\n255\n".encode() + np.ascontiguousarray(pixels).tobytes()


def yaml_text(pgm_path, cell_size, cx_min, cy_min):
    c = f64(f32(cell_size))
    return (f"image: {os.path.basename(str(pgm_path))}\nresolution: {float(c):.9g}\norigin: [{float(f64(cx_min) * c):.9g}, {float(f64(cy_min) * c):.9g}, 0]\n"
            "negate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n")
