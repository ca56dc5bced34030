"""Clouds whose Gaussians have PRESCRIBED member counts (helper of tests/test_size_edge_cloud.py and tests/test_gpu_size_edges.py).

The kernels behind buildGaussians / evalResiduals branch on exact member counts (acceptance at min_num_points_per_set, the three
size classes of k_size_classes and fit_task, 64 lanes, the chunk of the latency tier, Eigen's depth blocks kc, the constants of the
splitSet search).  A scene produces whatever counts it produces; here every count is constructed: one tight cluster per count, the
centres on a lattice several coarse cells apart in the empty space beside the scene, so that every cluster is exactly one leaf at
both resolutions.  The count list is read from the constants in the sources (`constants()`), every boundary with its neighbours.
"""
import os
import re

import numpy as np

from dmsa_lidar_slam_amd import synth
from dmsa_lidar_slam_amd.problems import DmsaOptimSettings, MapManagement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmsa_lidar_slam_amd", "csrc")

# what the sources call the boundaries: (file, regular expression with one group)
_PATTERNS = {
    "kSmallMax": ("serial_kernels.hip", r"constexpr int kSmallMax = (\d+);"),
    "small_default": ("serial_kernels.hip", r"int serial_small_threshold\(\) \{ return (\d+); \}"),
    "long_chunk": ("serial_kernels.hip", r"#define DMSA_LONG_CHUNK (\d+)"),
    "long_log2": ("serial_kernels.hip", r"#define DMSA_LONG_LOG2 (\d+)"),
    "kBL": ("serial_kernels.hip", r"constexpr int kBL = (\d+);"),
    "helpers": ("serial_kernels.h", r"int helpers = (\d+);"),
    "fit_chunk_per_wave": ("dmsa_kernels.hip", r"CH = (\d+) \* kFitWaves"),
    "kSplitChunk": ("dmsa_kernels.hip", r"constexpr int kSplitChunk = (\d+);"),
    "kSplitMaxChunks": ("dmsa_kernels.hip", r"constexpr int kSplitMaxChunks = (\d+);"),
    "kSplitBigLeaf": ("dmsa_kernels.hip", r"constexpr int kSplitBigLeaf = (\d+);"),
}
FIT_WAVES = (1, 4, 16)           # FitGroup<1> / <4> / <16>: the fit's short / middle / long class (static_asserts of k_gauss_fit_all)
SMALL_RULE = (32, 256)           # the built-in rule of voxelize_driver.cpp besides "nobody"
EIGEN_L1 = (32 * 1024, 48 * 1024)
MIN_POINTS = 10                  # min_num_points_per_set of both shipped settings
MAX_COUNT = 8193                 # one past the largest long_log2 boundary the switch matrix moves to (2^13)


def constants():
    out = {}
    text = {}
    for name, (fname, pat) in _PATTERNS.items():
        if fname not in text:
            with open(os.path.join(CSRC, fname)) as f:
                text[fname] = f.read()
        m = re.search(pat, text[fname])
        assert m is not None, f"{name}: `{pat}` not found in csrc/{fname} -- the boundary moved, follow it here"
        out[name] = int(m.group(1))
    return out


def eigen_kc(orc):
    """Eigen's depth block kc of centered^T * centered for both L1 sizes (680 / 1016), from the oracle's own blocking rule."""
    kc = []
    try:
        for l1 in EIGEN_L1:
            orc.set_eigen_l1_bytes(l1)
            kc.append(orc.eigen_gemm_kc(1 << 20))
    finally:
        orc.set_eigen_l1_bytes(EIGEN_L1[0])
    return tuple(kc)


def boundaries(orc):
    """{constant: the counts that straddle it}: the FIRST count of the pair / triple lies on the lower side."""
    c = constants()
    kc = eigen_kc(orc)
    b = {}
    b["min_num_points_per_set (>= 10)"] = [MIN_POINTS - 1, MIN_POINTS, MIN_POINTS + 1]
    for ns in sorted(set(SMALL_RULE + (c["small_default"], c["kSmallMax"]))):
        b[f"small tier n <= {ns}"] = [ns - 1, ns, ns + 1]
    b["64 lanes"] = [63, 64, 65]
    b[f"DMSA_LONG_CHUNK {c['long_chunk']} (parallel second pass above)"] = [c["long_chunk"] - 1, c["long_chunk"], c["long_chunk"] + 1]
    k = 5
    while (1 << k) <= MAX_COUNT:  # chain bins (floor(log2 n), next bit): an edge at every 2^k and every 3 * 2^(k-1)
        b[f"chain bin edge 2^{k}"] = [(1 << k) - 1, 1 << k, (1 << k) + 1]
        if 3 << (k - 1) <= MAX_COUNT and k < 13:
            b[f"chain bin edge 3*2^{k - 1}"] = [(3 << (k - 1)) - 1, 3 << (k - 1), (3 << (k - 1)) + 1]
        k += 1
    for ll in (9, 10, 11, c["long_log2"], 13):  # the built-in latency-tier boundary and the ones the long_log2 switch moves it to
        b[f"latency tier n >= 2^{ll}"] = [(1 << ll) - 1, 1 << ll, (1 << ll) + 1]
    for w in FIT_WAVES:  # fit chunks of 256 x waves members: the end of the first and of the second chunk
        ch = c["fit_chunk_per_wave"] * w
        for mult in (1, 2):
            if mult * ch + 1 <= MAX_COUNT:
                b[f"fit chunk {mult} x {ch} ({w} waves)"] = [mult * ch - 1, mult * ch, mult * ch + 1]
    h = c["helpers"]  # helper slices of a long Gaussian: counts that are not a multiple of the helper count, around the tier boundary
    b[f"{h} helper workgroups per long Gaussian"] = [(1 << c["long_log2"]) + 1, (1 << c["long_log2"]) + h - 1, (1 << 13) - 1, (1 << 13) + 1]
    for l1, v in zip(EIGEN_L1, kc):
        b[f"Eigen kc = {v} (L1 {l1})"] = [v - 1, v, v + 1, 2 * v, 2 * v + 1]
    return b


def count_list(orc):
    counts = sorted({n for v in boundaries(orc).values() for n in v})
    assert counts[0] == MIN_POINTS - 1 and counts[-1] == MAX_COUNT
    return counts


SHAPES = ("isotropic", "planar", "linear")


def _cluster(rng, n, half, kind, above):
    """n points around 0 within +-half.  `above`: the extended axes get a variance of ~0.58 (half)^2, above limitCovariance's 1e-4 clamp
    for half = fine / 16 of a 0.15 m grid (2.0e-4); else +-half / 4: variance 7e-6, below it.  Squeezed axes: +-0.5 mm."""
    ext = 3 if kind == "isotropic" else 2 if kind == "planar" else 1
    if above:
        u = rng.uniform(0.5, 1.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3)) * half
    else:
        u = rng.uniform(-0.25 * half, 0.25 * half, (n, 3))
    u[:, ext:] = rng.uniform(-5e-4, 5e-4, (n, 3 - ext))
    # squeezed axes rotate through x, y, z with the kind, so that a plane is not always z = const
    return np.roll(u, ext, axis=1)


def centres(num, coarse, x0=40.0, z=10.0):
    i = np.arange(num)
    return np.stack([x0 + 4 * coarse * (i % 8), 4 * coarse * (i // 8), np.full(num, z)], axis=-1)


def cluster_points(counts, min_grid_size, settings, seed=0):
    """(points n x 3 float32, ring ids, offsets len(counts) + 1): cluster i = points[off[i]:off[i + 1]], shape and scale cycling with i."""
    rng = np.random.default_rng(seed)
    fine, coarse = settings.grid_size_1_factor * min_grid_size, settings.grid_size_2_factor * min_grid_size
    ctr = centres(len(counts), coarse)
    pts, ids, off = [], [], [0]
    for i, n in enumerate(counts):
        u = _cluster(rng, n, fine / 16.0, SHAPES[i % 3], above=(i // 3) % 2 == 0)
        pts.append((ctr[i] + u).astype(np.float32))
        ids.append(np.arange(n) % 5)  # at least two distinct ring ids in every cluster: a leaf with one id is rejected
        off.append(off[-1] + n)
    return np.concatenate(pts), np.concatenate(ids).astype(np.int32), np.array(off, np.int64)


def window(counts, seed=0):
    """A small sliding window whose static points are the clusters: (problem, settings, cluster offsets into the static points)."""
    prob = synth.window_problem(seed=3, scans=2, rings=16, az_steps=128, num_static=0)
    s = DmsaOptimSettings.sliding_window()
    pts, ids, off = cluster_points(counts, prob.minGridSize, s, seed)
    static = np.zeros((pts.shape[0], prob.staticPoints.shape[1]), np.float32)
    static[:, :3] = pts
    prob.staticPoints = static
    prob.staticRingIds = ids.astype(prob.staticRingIds.dtype)
    return prob, s, off


def global_points(orc, prob, params=None, table=None):
    """The oracle's float global points of a window (scan points through the pose table, then the static points) and their ring ids."""
    if table is None:
        table, _ = orc.window_pose_table(prob)
    g = orc.transform_points(table, prob.localPoints, prob.tformIdPerPoint)
    return np.concatenate([g, prob.staticPoints]).astype(np.float32), np.concatenate([prob.ringIds, prob.staticRingIds])


def check_clusters(G, first, off, counts, min_points=MIN_POINTS):
    """The CONDITION of every test on these clouds: cluster i (points first + off[i] .. first + off[i + 1]) is, with exactly its members, a
    Gaussian at both resolutions if counts[i] >= min_points and at none otherwise; no Gaussian holds cluster points and anything else
    (nothing merged, nothing cut by a cell edge).  Returns {cluster index: its Gaussians' indices}."""
    seg, memb = np.asarray(G.seg_offset), np.asarray(G.members)
    found = {i: [] for i in range(len(counts))}
    for g in range(G.M):
        m = memb[seg[g]:seg[g + 1]]
        if m.max() < first or m.min() >= first + off[-1]:  # a Gaussian of the scene (or of the points behind the clusters)
            assert m.size >= min_points
            continue
        assert m.min() >= first, f"Gaussian {g} mixes scene points and cluster points"
        i = int(np.searchsorted(off, m[0] - first, side="right") - 1)
        want = np.arange(first + off[i], first + off[i + 1])
        assert np.array_equal(m, want), f"Gaussian {g} holds {m.size} members of the cluster of {counts[i]} (cut by a cell edge or merged with a neighbour)"
        found[i].append(g)
    for i, n in enumerate(counts):
        assert len(found[i]) == (2 if n >= min_points else 0), f"the cluster of {n} members came out as {len(found[i])} Gaussians"
    return found


KEY_FIRST = 12  # index of the first cluster point of a keyframes() cloud


# ---- keyframe clouds for the splitSet search ------------------------------------------------------------------------------------------
def split_leaves():
    """(leaf population, members whose normal points the other way): the populations straddle kSplitChunk, the 64-aligned chunk width behind
    it, kSplitBigLeaf and kSplitChunk x kSplitMaxChunks -- the partner range from which k_split_tasks widens its chunks beyond kSplitChunk
    (and the next width, 64 partners more); the smallest leaves split into halves of min - 1, min, min + 1 and min + 2 members, which pins
    the strict '>' on the halves (create_gaussian_sets)."""
    c = constants()
    m = MIN_POINTS
    leaves = [(2 * m - 1, m - 1), (2 * m, m), (2 * m + 1, m), (2 * m + 1, m + 1), (2 * m + 2, m + 1), (2 * m + 3, m + 2), (2 * m + 3, m + 1), (2 * m + 1, m - 1),
              (2 * m + 4, m + 2)]
    ch, big, lim = c["kSplitChunk"], c["kSplitBigLeaf"], c["kSplitChunk"] * c["kSplitMaxChunks"]
    minority = [m - 1, m, m + 1, m + 2]
    k = 0
    for L in (63, 64, 65, ch - 1, ch, ch + 1, ch + 63, ch + 64, ch + 65, 2 * ch - 1, 2 * ch, 2 * ch + 1, big - 1, big, big + 1):
        leaves.append((L, minority[k % 4] if k % 2 == 0 else L // 3))
        k += 1
    for L in (lim - 64, lim, lim + 1, lim + 65):
        leaves.append((L, minority[k % 4] if k % 2 == 0 else L // 3))
        k += 1
    return leaves


def keyframes(case, seed=0):
    """Three keyframes at (nearly) identical poses whose points are one cluster per split_leaves() entry; frame 0 is the identity, so its
    points are global.  Normals: +z for the majority, -z for the prescribed minority --
      noisy         both with noise (no ties), the minority anywhere in the leaf
      duplicates    exact +-z (every opposite pair ties at |n_a + n_c| = 0), the minority anywhere
      flipped_tail  the minority is the END of the leaf's member list (the minimal pairs sit at the end)
    Returns (problem, settings, offsets, leaves)."""
    rng = np.random.default_rng({"noisy": 11, "duplicates": 12, "flipped_tail": 13}[case] + 100 * seed)
    s = DmsaOptimSettings.keyframe_map()
    g = 0.25
    leaves = split_leaves()
    counts = [L for L, _ in leaves]
    pts, ids, off = cluster_points(counts, g, s, seed=seed + 1)
    pts[:, 0] -= np.float32(40.0)  # no scene here: the lattice starts at the origin
    n = pts.shape[0]
    nrm = np.zeros((n, 3), np.float32)
    nrm[:, 2] = 1.0
    for i, (L, k) in enumerate(leaves):
        a = int(off[i])
        where = np.arange(L - k, L) if case == "flipped_tail" else np.sort(rng.choice(L, k, replace=False))
        nrm[a + where, 2] = -1.0
    if case != "duplicates":
        nrm += rng.normal(0, 0.05 if case == "noisy" else 0.02, (n, 3)).astype(np.float32)
        nrm = (nrm / np.linalg.norm(nrm.astype(np.float64), axis=1)[:, None]).astype(np.float32)
    frames = 3
    # PCL anchors the voxel lattice at the FIRST point: twelve points far away lead frame 0 (the identity: the clusters behind them keep their
    # coordinates bit for bit), so that no cluster sits on the lattice's origin; frames 1 and 2 hold twelve far-away points each
    far = np.array([[-30.13, -30.21, 5.17]], np.float32) + rng.uniform(-0.01, 0.01, (3 * KEY_FIRST, 3)).astype(np.float32)
    far[KEY_FIRST:, 0] -= 10.0
    far[2 * KEY_FIRST:, 1] -= 10.0
    up = np.tile(np.array([[0, 0, 1]], np.float32), (KEY_FIRST, 1))
    far_ids = np.arange(KEY_FIRST, dtype=np.int32) % 5
    pts = np.concatenate([far[:KEY_FIRST], pts, far[KEY_FIRST:]]).astype(np.float32)
    nrm = np.concatenate([up, nrm, up, up])
    ids = np.concatenate([far_ids, ids, far_ids, far_ids])
    n += KEY_FIRST
    frame_off = np.array([0, n, n + KEY_FIRST, n + 2 * KEY_FIRST], np.int64)
    rel_o = np.zeros((frames, 3))
    rel_t = np.zeros((frames, 3))
    rel_t[1:] = rng.normal(0, 1e-3, (frames - 1, 3))
    prob = MapManagement(relOrientations=rel_o, relTranslations=rel_t, frameOffsets=frame_off, localPoints=pts, localNormals=nrm, ringIds=ids, minGridSize=g)
    return prob, s, off, leaves


def keyframe_global(orc, prob):
    """The oracle's float global points and normals of a keyframe set (normals rotated in the x0 + (x1 + x2) order, as the library does)."""
    f = np.float32
    tab = orc.keyframe_pose_table(prob)
    rows = np.repeat(np.arange(prob.numFrames, dtype=np.int32), np.diff(prob.frameOffsets))
    g = orc.transform_points(tab, prob.localPoints, rows)
    R = tab.reshape(-1, 3, 4)[rows][:, :, :3]
    t = (R * prob.localNormals[:, None, :3]).astype(f)
    nr = (t[:, :, 0] + (t[:, :, 1] + t[:, :, 2]).astype(f)).astype(f)
    return tab, g, np.concatenate([nr, np.zeros((nr.shape[0], 1), f)], axis=1)


def check_split(G, G_nosplit, off, leaves, min_points=MIN_POINTS):
    """Condition of the splitSet tests: without the split every leaf population is one Gaussian at both resolutions; with it, every leaf
    came out as exactly its halves above min_points (strict), twice."""
    check_clusters(G_nosplit, KEY_FIRST, off, [L for L, _ in leaves], min_points)
    seg, memb = np.asarray(G.seg_offset), np.asarray(G.members)
    sizes = {i: [] for i in range(len(leaves))}
    for g in range(G.M):
        m = memb[seg[g]:seg[g + 1]]
        if m.max() < KEY_FIRST or m.min() >= KEY_FIRST + off[-1]:
            continue
        i = int(np.searchsorted(off, m[0] - KEY_FIRST, side="right") - 1)
        assert m.min() >= KEY_FIRST + off[i] and m.max() < KEY_FIRST + off[i + 1]
        sizes[i].append(m.size)
    for i, (L, k) in enumerate(leaves):
        want = sorted(2 * [h for h in (L - k, k) if h > min_points])
        assert sorted(sizes[i]) == want, f"leaf of {L} members with {k} opposite normals: Gaussians of {sorted(sizes[i])} members, expected {want}"
