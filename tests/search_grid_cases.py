"""Clouds for the keyframe search grid (helper of tests/test_search_grid_cases.py and tests/test_gpu_search_grid.py; no GPU import).

sp_build_grid_device (csrc/next_rows_api.cpp) builds one uniform cell grid for addStaticPoints, getOverlap, updateNormals and
addNewKeyframeCloud; its kernels are in csrc/static_kernels.hip.  A mistake in them faults nothing: it drops a static point or picks a wrong
neighbour.  Here

  radius_exists, knn   are plain numpy statements of the two operations, independent of any grid: chunked brute force on the float32 distance
                       ((0 + dx*dx) + dy*dy) + dz*dz, every product and sum rounded on its own;
  grid_rule            restates how the build sizes its grid (bounds, cells of 1.001 r, key width, depth limit) -- used ONLY to prove which
                       path a case takes (64-bit keys, run lengths, ring distances), never to compute an expected answer;
  the constructors     return a Case: arrays plus the facts the case was built to have.  tests/test_search_grid_cases.py re-derives every
                       fact; the GPU tests then hold the kernels to the model on the same arrays.
"""
import functools
import itertools
import os
import re
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PATTERNS = {
    "kMaxNeighbours": r"constexpr int kMaxNeighbours = (\d+);",  # the API admits k = 1 .. 8
    "kMaxRings": r"constexpr int kMaxRings = (\d+);",            # beyond it a k-NN query falls back to an exhaustive pass
    "wave_query_shift": r"if \(nq <= \(\(int64_t\)1 << (\d+)\) \|\| n >= 4 \* nq\)",  # a wave per query up to here, a thread per query beyond
}


def constants():
    with open(os.path.join(ROOT, "dmsa_lidar_slam_amd", "csrc", "static_kernels.hip")) as f:
        text = f.read()
    out = {}
    for name, pat in _PATTERNS.items():
        m = re.search(pat, text)
        assert m is not None, f"{name}: `{pat}` not found in csrc/static_kernels.hip -- the constant moved, follow it here"
        out[name] = int(m.group(1))
    return out


_C = constants()
K_MAX = _C["kMaxNeighbours"]
K_MAX_RINGS = _C["kMaxRings"]
WAVE_QUERY_LIMIT = 1 << _C["wave_query_shift"]
R = F32(0.3)              # radius / cell hint of the small cases
BAD_ROWS = np.array([[np.nan, 0, 0, 1], [0, np.inf, 0, 1], [0, 0, -np.inf, 1], [np.nan, np.nan, np.nan, 1]], F32)


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
def finite_rows(a):
    return np.isfinite(np.asarray(a)[:, :3]).all(axis=1)


def sq_dist(q, c):
    """(nq, n) float32: ((0 + dx*dx) + dy*dy) + dz*dz of flann::L2_Simple, one rounding per operation (numpy never fuses)."""
    q, c = np.asarray(q, F32), np.asarray(c, F32)
    d = np.zeros((q.shape[0], c.shape[0]), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            t = q[:, None, a] - c[None, :, a]
            d = d + t * t
    return d


def radius_exists(cloud, query, r, chunk=1024):
    """flag[i]: some finite cloud row lies within float32(r) * float32(r) of query i.  Non-finite rows never match and are never matched."""
    cloud, query = np.asarray(cloud, F32), np.asarray(query, F32)
    r2 = F32(r) * F32(r)
    c = cloud[finite_rows(cloud)]
    qf = np.flatnonzero(finite_rows(query))
    out = np.zeros(query.shape[0], bool)
    if c.shape[0] == 0:
        return out
    for b in range(0, qf.shape[0], chunk):
        rows = qf[b:b + chunk]
        out[rows] = (sq_dist(query[rows], c) <= r2).any(axis=1)
    return out


def knn(cloud, k, chunk=256):
    """(n, k) int32: for every finite row the first min(k, num_finite) rows by ascending (float32 distance, row index), itself included,
    padded with -1; all -1 for a non-finite row."""
    cloud = np.asarray(cloud, F32)
    fin = np.flatnonzero(finite_rows(cloud))
    out = np.full((cloud.shape[0], k), -1, np.int32)
    want = min(k, fin.shape[0])
    if want == 0:
        return out
    c = cloud[fin]
    idx = fin.astype(np.uint64)[None, :]
    for b in range(0, fin.shape[0], chunk):
        d = np.ascontiguousarray(sq_dist(c[b:b + chunk], c))
        # distances are +0, positive or +inf: their bit patterns order like the floats, so (bits << 32 | index) orders like the pair
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx
        if want < fin.shape[0]:
            key = np.partition(key, want - 1, axis=1)[:, :want]
        key = np.sort(key, axis=1)
        out[fin[b:b + chunk], :want] = (key & np.uint64(0xFFFFFFFF)).astype(np.int32)
    return out


def kth_tie(cloud, k):
    """Per finite row: is the k-th place tied with the (k+1)-th, so that only the row index decides who is in the list?"""
    cloud = np.asarray(cloud, F32)
    c = cloud[finite_rows(cloud)]
    if c.shape[0] <= k:
        return np.zeros(c.shape[0], bool)
    d = np.sort(sq_dist(c, c), axis=1)
    return d[:, k - 1] == d[:, k]


# ---- the grid rule (proves the path; never an expected answer) -------------------------------------------------------------------------
@dataclass
class GridRule:
    lo: np.ndarray        # (3,) float64: float bounds of the finite rows
    hi: np.ndarray
    inv: float            # 1 / (1.001 * float32(r)) in double
    ext: np.ndarray       # (3,) (hi - lo) * inv
    too_deep: bool        # DMSA_ERR_DEPTH: ext >= 2097150 on an axis
    dims: tuple           # (nx, ny, nz), None when too_deep or no finite row
    cells: int            # nx * ny * nz as a Python integer
    key64: bool           # cells > 2^31: the all-ones marker needs one value more than the largest code
    cell: float           # edge of a cell, 1.001 * float32(r)

    def coord(self, pts):
        """(n, 3) float64 grid coordinates (p - lo) * inv, unclamped: floor() of it is the cell a QUERY is looked up in."""
        return (np.asarray(pts, F32)[:, :3].astype(np.float64) - self.lo) * self.inv

    def cell_of(self, pts):
        """(n, 3) int64 cell of CLOUD rows (clamped like k_cell_codes; rows must be finite)."""
        v = np.floor(self.coord(pts)).astype(np.int64)
        return np.clip(v, 0, np.asarray(self.dims, np.int64) - 1)

    def code(self, pts):
        """(n,) uint64 cell codes ix + nx (iy + ny iz)."""
        c = self.cell_of(pts).astype(np.uint64)
        nx, ny = np.uint64(self.dims[0]), np.uint64(self.dims[1])
        return c[:, 0] + nx * (c[:, 1] + ny * c[:, 2])


def grid_rule(cloud, r):
    cloud = np.asarray(cloud, F32)
    c = cloud[finite_rows(cloud)][:, :3]
    cell = 1.001 * float(F32(r))
    inv = 1.0 / cell
    if c.shape[0] == 0:
        z = np.zeros(3)
        return GridRule(z, z, inv, z, False, (1, 1, 1), 1, False, cell)
    lo, hi = c.min(axis=0).astype(np.float64), c.max(axis=0).astype(np.float64)
    ext = (hi - lo) * inv
    if (ext >= 2097150.0).any():
        return GridRule(lo, hi, inv, ext, True, None, 0, False, cell)
    dims = tuple(int(np.floor(e)) + 1 for e in ext)
    cells = dims[0] * dims[1] * dims[2]
    return GridRule(lo, hi, inv, ext, False, dims, cells, cells > (1 << 31), cell)


def sorted_layout(cloud, rule):
    """What the build's stable sort leaves: (row order, sorted codes); non-finite rows carry the all-ones marker and come last."""
    cloud = np.asarray(cloud, F32)
    fin = finite_rows(cloud)
    codes = np.full(cloud.shape[0], np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    codes[fin] = rule.code(cloud[fin])
    order = np.argsort(codes, kind="stable")
    return order, codes[order]


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    cloud: np.ndarray   # (n, 4) float32
    query: np.ndarray   # (m, 4) float32
    r: np.float32       # radius of the radius test = cell hint of the normals
    facts: dict = field(default_factory=dict)

    @property
    def rule(self):
        return grid_rule(self.cloud, self.r)


def _rows(xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return np.concatenate([xyz, np.ones((xyz.shape[0], 1))], axis=1).astype(F32)


def with_bad_rows(cloud):
    """NaN and inf rows at the front, in the middle and at the end of the index order."""
    h = cloud.shape[0] // 2
    return np.concatenate([BAD_ROWS[:2], cloud[:h], BAD_ROWS[2:], cloud[h:], BAD_ROWS[[1, 0]]]).astype(F32)


def _queries_around(cloud, r, rng, count, uniform_lo, uniform_hi):
    """Queries displaced from cloud rows by 0 .. 2 r in random directions (hits and misses), a few uniform ones, non-finite and huge ones."""
    c = cloud[finite_rows(cloud)][:, :3].astype(np.float64)
    pick = c[rng.integers(0, c.shape[0], count)]
    d = rng.normal(size=(count, 3))
    d *= (rng.uniform(0.0, 2.0, count) * float(r) / np.linalg.norm(d, axis=1))[:, None]
    uni = rng.uniform(uniform_lo, uniform_hi, (count // 10, 3))
    odd = np.array([[1e30, 0, 0, 1], [0, -1e30, 0, 1], [0, 0, 3e38, 1], [np.nan, 0, 0, 1], [0, np.inf, 0, 1]], F32)
    return np.concatenate([_rows(pick + d), _rows(uni), odd, _rows(c[:3])])


def _wide(name, dims, r, seed, alias=False, clusters=60):
    """Tight clusters (a 4 x 4 x 3 lattice of half-cell spacing each) spread over a box of `dims` cells, pinned by two corner rows."""
    r = F32(r)
    c = 1.001 * float(r)
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, np.int64)
    top = (dims - 0.5) * c
    cells = np.stack([rng.integers(2, dims[a] - 3, clusters) for a in range(3)], axis=1)
    a = np.argmax(dims)
    if dims[a] > (1 << 20):  # the slab: half of the clusters beyond cell 2^20 of the long axis
        cells[: clusters // 2, a] = rng.integers((1 << 20) + 1, dims[a] - 3, clusters // 2)
    if alias:  # two clusters whose first cells differ by exactly 2^32 in the code
        iz, rem = divmod(1 << 32, int(dims[0] * dims[1]))
        iy, ix = divmod(rem, int(dims[0]))
        cells[0] = [100, 100, 100]
        cells[1] = cells[0] + [ix, iy, iz]
        assert (cells[1] < dims - 3).all()
    lat = np.array(list(itertools.product(range(4), range(4), range(3))), np.float64) * 0.5
    pts = [(cc + 0.1 + lat + rng.uniform(0.0, 0.1, lat.shape)) * c for cc in cells]
    xyz = np.concatenate([np.zeros((1, 3)), np.concatenate(pts), top[None, :]])
    xyz = xyz[rng.permutation(xyz.shape[0])]
    cloud = with_bad_rows(_rows(xyz))
    query = _queries_around(cloud, r, rng, 1500, -2.0 * c, top + 2.0 * c)
    return Case(name, cloud, query, r, {"dims": tuple(int(d) for d in dims), "alias": alias})


def occupied_alias_pair(case):
    """Two occupied cell codes equal modulo 2^32 (None if there is none): a key cut to 32 bits would merge their cells."""
    codes = np.unique(case.rule.code(case.cloud[finite_rows(case.cloud)]))
    low = codes & np.uint64(0xFFFFFFFF)
    order = np.argsort(low, kind="stable")
    same = np.flatnonzero(low[order][1:] == low[order][:-1])
    if same.shape[0] == 0:
        return None
    return int(codes[order][same[0]]), int(codes[order][same[0] + 1])


def wide32_edge():
    return _wide("wide32_edge", (1290, 1290, 1290), 0.5, 1)       # 1290^3 = 2 146 689 000 < 2^31: the last 32-bit grid


def wide64_band():
    return _wide("wide64_band", (1500, 1500, 1500), 0.5, 2)       # 2^31 < 3.375e9 < 2^32: 64 bits only because of the marker


def wide64():
    return _wide("wide64", (2000, 2000, 2000), 0.5, 3, alias=True)  # 8e9 > 2^32, two occupied codes 2^32 apart


def wide64_slab():
    return _wide("wide64_slab", (1_200_000, 64, 64), 1.0, 4)      # one axis beyond 2^20 cells, 4.9e9 cells


def too_deep(deep=True):
    """Two finite rows 2097150 cells (deep) or a little less (not deep: the longest axis the build accepts) apart along y."""
    r = F32(0.5)
    c = 1.001 * float(r)
    far = 2097150.5 * c if deep else 2097149.0 * c
    cloud = np.concatenate([BAD_ROWS[:1], _rows([[0, 0, 0], [0, far, 0]])])
    assert ((float(cloud[2, 1]) - 0.0) / c >= 2097150.0) == deep
    query = _rows([[0, 0.2, 0], [0, far, 0.4], [0, far / 2, 0], [0.6, 0, 0]])
    return Case("too_deep" if deep else "deepest", cloud, query, r, {"deep": deep})


def boundary_pair(p, r, axis=0, sign=-1.0):
    """Two queries on the line through p along `axis`: the farthest float whose distance to p is still <= r^2 and the next float
    beyond it (the pair of test_radius_boundary_inclusive, found by walking the query instead of the point)."""
    p = np.asarray(p, F32)
    r2 = F32(r) * F32(r)
    away = F32(sign * np.inf)

    def dist(x):
        t = F32(x) - p[axis]
        return F32(t * t)  # the other two terms are 0 + 0 * 0

    x = F32(float(p[axis]) + sign * float(F32(r)))
    while dist(x) > r2:
        x = np.nextafter(x, p[axis])
    while dist(np.nextafter(x, away)) <= r2:
        x = np.nextafter(x, away)
    q_in, q_out = p.copy(), p.copy()
    q_in[axis], q_out[axis] = x, np.nextafter(x, away)
    q_in[3] = q_out[3] = 1.0
    return q_in, q_out


RUN_LENGTHS = (63, 64, 65, 127, 128, 129)
RUN_TAILS = ("cell", "end", "marker")


def runs(m, near="last", tail="cell"):
    """Cell (2, 1, 1) of a 3 x 2 x (2 or 3) grid holds exactly m rows; only one of them, the last (or first) in index order, is within r
    of the query pair in cell (1, 1, 1).  tail: the run is followed by another cell's row / ends at n / is followed by marker rows."""
    c = 1.001 * float(R)
    rng = np.random.default_rng(1000 * m + 10 * RUN_TAILS.index(tail) + (near == "last"))
    hit = _rows([[2.3 * c, 1.5 * c, 1.5 * c]])
    far = _rows(np.stack([rng.uniform(2.55 * c, 2.9 * c, m - 1), rng.uniform(1.05 * c, 1.95 * c, m - 1), rng.uniform(1.05 * c, 1.95 * c, m - 1)], axis=1))
    anchors = [[0, 0, 0]] + ([[0.5 * c, 0.5 * c, 2.5 * c]] if tail == "cell" else [])
    cloud = np.concatenate([_rows(anchors)] + ([far, hit] if near == "last" else [hit, far]))
    if tail == "marker":
        cloud = with_bad_rows(cloud)
    q_in, q_out = boundary_pair(hit[0], R)
    other = _rows([far[0, :3], [0.1 * c, 0.1 * c, 0.1 * c], [1.5 * c, 0.2 * c, 0.2 * c]])  # a far row itself: hit; beside the anchor: hit; nowhere: miss
    query = np.concatenate([q_in[None], q_out[None], other])
    return Case(f"runs_{m}_{near}_{tail}", cloud, query, R, {"m": m, "near": near, "tail": tail, "hit": hit[0], "expect": [True, False, True, True, False]})


OFFSETS = tuple(o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0))


def neighbour(o, inside=True):
    """3 x 3 x 3 cells pinned by eight corner rows; the query is the centre of the middle cell; exactly one further row lies in neighbour
    cell `o`: within r (inside) or, in the twin cloud, just beyond r in the same cell."""
    c = 1.001 * float(R)
    top = 2.95 * c
    corners = np.array(list(itertools.product((0.0, top), repeat=3)))
    q = np.full(3, 1.5 * c)
    o = np.asarray(o, np.float64)
    t = 0.52 * c if inside else 1.01 * float(R) / np.linalg.norm(o)
    cloud = _rows(np.concatenate([corners[:4], (q + o * t)[None], corners[4:]]))
    return Case(f"neighbour_{'in' if inside else 'out'}_{int(o[0])}_{int(o[1])}_{int(o[2])}", cloud, _rows([q]), R,
                {"offset": tuple(int(v) for v in o), "inside": inside, "row": 4})


def margin():
    """5 x 5 x 5 cells pinned by eight corner rows, one row in the middle of every face.  Queries 0-1, 1-2 and more than 2 cells outside
    every face, each facing the face's row (`with`) or away from every row; the eight outer corners; |x| = 1e30."""
    c = 1.001 * float(R)
    n, top = 5, 4.95 * c
    corners = np.array(list(itertools.product((0.0, top), repeat=3)))
    faces, rows, band, facing = [], [], [], []
    for a in range(3):
        for side in (0, 1):
            f = np.full(3, 2.5 * c)
            f[a] = top if side else 0.0
            faces.append(f)
            # grid coordinate along the axis: bands (-1, 0), (-2, -1], <= -2 below; [n, n + 1), [n + 1, n + 2), >= n + 2 above
            for b, v in ((0, -0.4), (1, -1.5), (1, -1.99), (2, -2.01), (2, -2.5)) if side == 0 else ((0, n + 0.3), (1, n + 1.5), (1, n + 1.99), (2, n + 2.01), (2, n + 2.5)):
                for face_on in (True, False):
                    p = np.full(3, 2.5 * c if face_on else 1.2 * c)
                    p[a] = v * c
                    rows.append(p), band.append(b), facing.append(face_on)
    for corner in itertools.product((-0.4 * c, (n + 0.3) * c), repeat=3):
        rows.append(np.array(corner)), band.append(0), facing.append(True)
    huge = []
    for a in range(3):
        for s in (1e30, -1e30):
            p = np.full(3, 2.5 * c)
            p[a] = s
            huge.append(p)
    huge += [np.full(3, 1e30), np.array([3e38, -3e38, 2.5 * c])]
    band += [2] * len(huge)
    facing += [False] * len(huge)
    cloud = _rows(np.concatenate([corners, np.array(faces)]))
    return Case("margin", cloud, _rows(np.array(rows + huge)), R, {"band": np.array(band), "facing": np.array(facing), "n_axis": n})


def lattice_ties(k):
    """A shuffled 7 x 7 x 7 integer lattice scaled by 0.25: distances are exact, so most k-th places are exact ties, and the index order has
    nothing to do with the spatial or the sorted order.  Ten sites are doubled (ties at distance 0); for k = 1 every site is, since only a
    coincident row can tie with a row's own distance 0.  Queries: the 9 x 9 x 9 lattice around it at r = 0.25 (outer faces: d == r^2)."""
    rng = np.random.default_rng(7)
    site = (np.array(list(itertools.product(range(7), repeat=3)), np.float64) - 3.0) * 0.25
    xyz = np.concatenate([site, site if k == 1 else site[rng.choice(343, 10, replace=False)]])
    cloud = with_bad_rows(_rows(xyz[rng.permutation(xyz.shape[0])]))
    query = _rows((np.array(list(itertools.product(range(9), repeat=3)), np.float64) - 4.0) * 0.25)
    return Case("lattice_ties_doubled" if k == 1 else "lattice_ties", cloud, query, F32(0.25), {"k": k})


def isolated_in_crowd():
    """4000 rows in a cube of 8 cells (every k <= 8 search ends within two rings) and 40 rows on a coarse lattice 12 cells apart and at
    least 12 cells from the crowd (they walk past ring 6 into the exhaustive pass), shuffled together with NaN rows."""
    c = 1.001 * float(R)
    rng = np.random.default_rng(11)
    crowd = rng.uniform(0.0, 8.0 * c, (4000, 3))
    coarse = np.array(list(itertools.product(range(4), repeat=3)), np.float64)
    lone = (20.0 + 12.0 * coarse[rng.choice(64, 40, replace=False)]) * c + rng.uniform(0.0, 0.5 * c, (40, 3))
    bad = np.tile(BAD_ROWS, (3, 1))
    cloud = np.concatenate([_rows(crowd), _rows(lone), bad])
    kind = np.concatenate([np.zeros(4000, int), np.ones(40, int), np.full(bad.shape[0], 2)])
    perm = rng.permutation(cloud.shape[0])
    cloud, kind = cloud[perm], kind[perm]
    d = rng.normal(size=(40, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    query = np.concatenate([_rows(lone + 0.9 * float(R) * d), _rows(lone + 1.1 * float(R) * d), _rows(crowd[:400] + 0.5 * c)])
    return Case("isolated_in_crowd", cloud.astype(F32), query, R, {"kind": kind})


FEW = (1, 2, 3, 5)


def few_finite(f):
    """f finite rows among 20 NaN rows: want = min(k, num_finite) < k for every k above f."""
    pts = _rows([[0, 0, 0], [0.1, 0, 0], [0, 0.2, 0], [0.05, 0.05, 0.3], [0.3, 0.3, 0.3]])[:f]
    cloud = np.tile(BAD_ROWS[:1], (20 + f, 1))
    at = [3, 4, 11, 19, 24][:f]
    cloud[at] = pts
    query = _rows([[0.05, 0, 0], [0, 0.45, 0], [5, 5, 5], [0.3, 0.3, 0.45]])
    return Case(f"few_finite_{f}", cloud, query, R, {"f": f, "at": at})


DEGENERATE = ("identical", "planar", "planar_negzero")


def degenerate(kind):
    """identical: 1000 equal rows (extent 0, one cell, one run).  planar: z = 0 exactly (nz = 1).  planar_negzero: z = -0.0f on every
    other row of the same cloud -- equal as numbers, different under float_to_ordered."""
    c = 1.001 * float(R)
    if kind == "identical":
        p = np.array([1.5, -2.25, 0.75])
        cloud = np.tile(_rows([p]), (1000, 1))
        q_in, q_out = boundary_pair(cloud[0], R, axis=1, sign=1.0)
        query = np.concatenate([cloud[:1], q_in[None], q_out[None], _rows([p + [0, 0, 1.5 * c], p - [2.5 * c, 0, 0], p + [0.1, 0.1, 0.1]])])
        return Case("degenerate_identical", cloud, query, R, {"kind": kind, "expect": [True, True, False, False, False, True]})
    rng = np.random.default_rng(5)
    g = np.array(list(itertools.product(range(30), repeat=2)), np.float64) * 0.1 + rng.uniform(0.0, 0.05, (900, 2))
    cloud = with_bad_rows(_rows(np.concatenate([g, np.zeros((900, 1))], axis=1)[rng.permutation(900)]))
    if kind == "planar_negzero":
        cloud[::2, 2] = np.where(np.isfinite(cloud[::2, 2]), F32(-0.0), cloud[::2, 2])
    base = cloud[finite_rows(cloud)][:200, :3].astype(np.float64)
    dz = np.array([0.29, -0.29, 0.31, -0.31, 0.7, -0.7])
    query = np.concatenate([_rows(base + [0, 0, z]) for z in dz] + [_rows(base[:20] + [0.02, 0.01, 0.0])])
    return Case(f"degenerate_{kind}", cloud, query, R, {"kind": kind})


# ---- registries ----------------------------------------------------------------------------------------------------------------------------
WIDE = ("wide32_edge", "wide64_band", "wide64", "wide64_slab")
RUNS = tuple(f"runs_{m}_{near}_{tail}" for m in RUN_LENGTHS for near in ("last", "first") for tail in RUN_TAILS)
NEIGHBOUR = tuple(f"neighbour_{w}_{o[0]}_{o[1]}_{o[2]}" for o in OFFSETS for w in ("in", "out"))
KNN = ("lattice_ties", "lattice_ties_doubled", "isolated_in_crowd") + tuple(f"few_finite_{f}" for f in FEW) + tuple(f"degenerate_{d}" for d in DEGENERATE) + ("wide64",)
RADIUS = WIDE + RUNS + NEIGHBOUR + ("margin", "deepest") + KNN[:-1]
K_VALUES = (1, 2, 3, 6, 8)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of that name, built once and shared (treat the arrays as read-only)."""
    if name in WIDE:
        out = {"wide32_edge": wide32_edge, "wide64_band": wide64_band, "wide64": wide64, "wide64_slab": wide64_slab}[name]()
    elif name.startswith("runs_"):
        _, m, near, tail = name.split("_")
        out = runs(int(m), near, tail)
    elif name.startswith("neighbour_"):
        _, w, x, y, z = name.split("_")
        out = neighbour((int(x), int(y), int(z)), w == "in")
    elif name.startswith("few_finite_"):
        out = few_finite(int(name.rsplit("_", 1)[1]))
    elif name.startswith("degenerate_"):
        out = degenerate(name.split("_", 1)[1])
    else:
        out = {"margin": margin, "too_deep": too_deep, "deepest": lambda: too_deep(False), "lattice_ties": lambda: lattice_ties(6),
               "lattice_ties_doubled": lambda: lattice_ties(1), "isolated_in_crowd": isolated_in_crowd}[name]()
    assert out.name == name, (out.name, name)
    for a in (out.cloud, out.query):
        a.setflags(write=False)
    return out


def knn_case_for(name, k):
    """lattice_ties is the one case whose cloud depends on k."""
    return "lattice_ties_doubled" if name == "lattice_ties" and k == 1 else name


@functools.lru_cache(maxsize=None)
def model_flags(name):
    c = case(name)
    out = radius_exists(c.cloud, c.query, c.r)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model_knn(name):
    """Neighbour lists for k = 8; the list for a smaller k is its prefix (ascending (distance, index) both ways)."""
    out = knn(case(name).cloud, K_MAX)
    out.setflags(write=False)
    return out


def tiled(a, count):
    """The rows of `a` repeated in order up to `count` rows (queries and their flags tile alike)."""
    return np.resize(a, (count,) + a.shape[1:])
