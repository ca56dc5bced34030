"""The independent model of include/dmsa_dense_align.h, A0-A8: the yardstick of tests/test_gpu_dense_align.py.

The pairs come from dense_compare_model.nearest (cKDTree candidates re-tested in float32, the winner by (d2, row)); quantisation and sums are
Python ints of any size; M is Python ints; the solve is pure-Python floats, operation for operation as A3 states (a Python float operation is
one IEEE double operation, rounded on its own; float(int) rounds to nearest even); composition and stopping are A5 and A6.  Nothing here
knows of cells, waves or the two-word form of a sum."""
import math

import numpy as np

import dense_compare_model as dm

f32 = np.float32
STOPS = ("CONVERGED", "MAX_ITERATIONS", "TOO_FEW_PAIRS")
IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def scale_c_of(voxel):
    _, e = math.frexp(float(f32(voxel)))
    return 2.0 ** (10 - e)


def quantise(xyz, scale_c):
    """A2: rintf(p * scale_c) per coordinate, the product in float32 (exact: a power of two), as Python ints."""
    q = np.rint((np.asarray(xyz, f32) * f32(scale_c)).astype(f32)).astype(np.int64)
    return [[int(v) for v in row] for row in q.reshape(-1, 3)]


def sums_of_pairs(P, G):
    """A2 over the quantised pairs (lists of int triples): n, sp, sg, spg as Python ints."""
    out = dict(n=len(P), sp=[0, 0, 0], sg=[0, 0, 0], spg=[[0, 0, 0] for _ in range(3)])
    for p, g in zip(P, G):
        for a in range(3):
            out["sp"][a] += p[a]
            out["sg"][a] += g[a]
            for b in range(3):
                out["spg"][a][b] += p[a] * g[b]
    return out


def pair_sums(store, ref, ref_valid, max_distance, voxel):
    """A1-A2 of the reference as it stands: (sums, d2 of the completeness direction, index)."""
    store, ref = np.asarray(store, f32)[:, :3], np.asarray(ref, f32)[:, :3]
    d2, idx = dm.nearest(ref, store, max_distance, q_valid=ref_valid)
    got = np.flatnonzero(idx >= 0)
    sc = scale_c_of(voxel)
    return sums_of_pairs(quantise(ref[got], sc), quantise(store[idx[got]], sc)), d2, idx


def _jacobi_quaternion(S):
    A = [[0.0] * 4 for _ in range(4)]
    A[0][0] = (S[0][0] + S[1][1]) + S[2][2]
    A[1][1] = (S[0][0] - S[1][1]) - S[2][2]
    A[2][2] = (S[1][1] - S[0][0]) - S[2][2]
    A[3][3] = (S[2][2] - S[0][0]) - S[1][1]
    A[0][1] = A[1][0] = S[1][2] - S[2][1]
    A[0][2] = A[2][0] = S[2][0] - S[0][2]
    A[0][3] = A[3][0] = S[0][1] - S[1][0]
    A[1][2] = A[2][1] = S[0][1] + S[1][0]
    A[1][3] = A[3][1] = S[2][0] + S[0][2]
    A[2][3] = A[3][2] = S[1][2] + S[2][1]
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(16):
        off = ((((A[0][1] * A[0][1] + A[0][2] * A[0][2]) + A[0][3] * A[0][3]) + A[1][2] * A[1][2]) + A[1][3] * A[1][3]) + A[2][3] * A[2][3]
        if off == 0.0:
            break
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                root = abs(theta) + math.sqrt(theta * theta + 1.0)
                t = -1.0 / root if theta < 0.0 else 1.0 / root
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                A[p][p] = A[p][p] - t * apq
                A[q][q] = A[q][q] + t * apq
                A[p][q] = A[q][p] = 0.0
                for r in range(4):
                    if r == p or r == q:
                        continue
                    arp, arq = A[r][p], A[r][q]
                    A[r][p] = A[p][r] = c * arp - s * arq
                    A[r][q] = A[q][r] = s * arp + c * arq
                for r in range(4):
                    vrp, vrq = V[r][p], V[r][q]
                    V[r][p] = c * vrp - s * vrq
                    V[r][q] = s * vrp + c * vrq
    best = 0
    for i in range(1, 4):
        if A[i][i] > A[best][best]:
            best = i
    v = [V[r][best] for r in range(4)]
    norm = math.sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3])
    v = [x / norm for x in v]
    flip = v[0] < 0.0
    if v[0] == 0.0:
        for x in v[1:]:
            if x != 0.0:
                flip = x < 0.0
                break
    return [-x for x in v] if flip else v


def centred(sums):
    """A3: M[a][b] = n * Spg[a][b] - Sp[a] * Sg[b], Python ints."""
    return [[sums["n"] * sums["spg"][a][b] - sums["sp"][a] * sums["sg"][b] for b in range(3)] for a in range(3)]


def solve(sums, scale_c=1.0):
    """A3-A4: (dT as 12 floats row-major, shift_m, rotation_rad)."""
    n = sums["n"]
    M = [[float(v) for v in row] for row in centred(sums)]
    mx = 0.0
    for a in range(3):
        for b in range(3):
            if abs(M[a][b]) > mx:
                mx = abs(M[a][b])
    if mx != 0.0:
        w, x, y, z = _jacobi_quaternion([[M[a][b] / mx for b in range(3)] for a in range(3)])
    else:
        w, x, y, z = 1.0, 0.0, 0.0, 0.0
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    R = [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
         [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
         [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]
    pm = [float(sums["sp"][a]) / float(n) for a in range(3)]
    gm = [float(sums["sg"][a]) / float(n) for a in range(3)]
    dT, sh = [], []
    for a in range(3):
        dT += [R[a][0], R[a][1], R[a][2], (gm[a] - ((R[a][0] * pm[0] + R[a][1] * pm[1]) + R[a][2] * pm[2])) / scale_c]
        sh.append((gm[a] - pm[a]) / scale_c)
    return dT, math.sqrt((sh[0] * sh[0] + sh[1] * sh[1]) + sh[2] * sh[2]), 2.0 * math.sqrt((xx + yy) + zz)


def compose(D, T):
    """A5: D o T, 12 floats each."""
    out = []
    for a in range(3):
        for c in range(4):
            v = (D[4 * a] * T[c] + D[4 * a + 1] * T[4 + c]) + D[4 * a + 2] * T[8 + c]
            out.append(v + D[4 * a + 3] if c == 3 else v)
    return out


def align(store, raw, voxel, T0=None, max_distance=1.0, max_iterations=30, min_pairs=3, stop_translation=1e-4, stop_rotation=1e-5):
    """A1-A8 as DenseCloudCreator.align_reference returns it (transform as 12 floats)."""
    store, raw = np.asarray(store, f32)[:, :3], np.asarray(raw, f32)[:, :3]
    T = [float(v) for v in (IDENTITY if T0 is None else np.asarray(T0, np.float64)[:3, :4].reshape(-1))]
    sc = scale_c_of(voxel)
    d4_scale, _ = dm.scale_of(max_distance)
    history, stop, sums = [], "MAX_ITERATIONS", None
    for _ in range(max_iterations):
        ref = dm.transform(raw, np.array(T).reshape(3, 4))
        valid = dm.valid_rows(ref, voxel)
        sums, d2, _ = pair_sums(store, ref, valid, max_distance, voxel)
        d4 = dm.direction(d2, valid, max_distance, max_distance)
        it = dict(matched=d4["matched"], unmatched=d4["unmatched"], s2=d4["s2"], rms_m=d4["rms_m"], shift_m=0.0, rotation_rad=0.0)
        history.append(it)
        assert d4["matched"] == sums["n"] and d4_scale > 0
        if sums["n"] < min_pairs:
            stop = "TOO_FEW_PAIRS"
            break
        dT, it["shift_m"], it["rotation_rad"] = solve(sums, sc)
        T = compose(dT, T)
        if it["shift_m"] <= stop_translation and it["rotation_rad"] <= stop_rotation:
            stop = "CONVERGED"
            break
    return dict(transform=T, iterations=len(history), stop=stop, scale_c=sc, history=history, sums=sums)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------------
def rigid(deg, axis, t):
    """A 3x4 float64 rigid motion: a rotation by `deg` degrees about `axis`, then the translation t (Rodrigues, numpy)."""
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = math.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    return np.concatenate([R, np.asarray(t, np.float64).reshape(3, 1)], axis=1)


def inverse(T):
    T = np.asarray(T, np.float64).reshape(3, 4)
    return np.concatenate([T[:, :3].T, -(T[:, :3].T @ T[:, 3:])], axis=1)


def room(rng, voxel=0.1, size=(8.0, 6.0, 3.0), step=None, corner=(-4.0, -3.0, -1.0)):
    """The surface of a box with two inner faces, one point per lattice node `step` apart with a jitter well inside a voxel: an (n,3) float32
    cloud in which no two points share a voxel."""
    step = 2 * voxel if step is None else step
    sx, sy, sz = size
    xs, ys, zs = (np.arange(step / 2, s, step) for s in size)
    faces = []
    for x in (0.0, sx):
        yy, zz = np.meshgrid(ys, zs, indexing="ij")
        faces.append(np.stack([np.full(yy.size, x), yy.ravel(), zz.ravel()], axis=1))
    for y in (0.0, sy):
        xx, zz = np.meshgrid(xs, zs, indexing="ij")
        faces.append(np.stack([xx.ravel(), np.full(xx.size, y), zz.ravel()], axis=1))
    for z in (0.0, sz):
        xx, yy = np.meshgrid(xs, ys, indexing="ij")
        faces.append(np.stack([xx.ravel(), yy.ravel(), np.full(xx.size, z)], axis=1))
    # two inner faces: a wall across x at 3/8 of the length over half the width, and a wall across y at 2/3 of the width over a third of the length
    yy, zz = np.meshgrid(ys[ys < sy / 2], zs, indexing="ij")
    faces.append(np.stack([np.full(yy.size, 0.375 * sx), yy.ravel(), zz.ravel()], axis=1))
    xx, zz = np.meshgrid(xs[xs > 2 * sx / 3], zs, indexing="ij")
    faces.append(np.stack([xx.ravel(), np.full(xx.size, 2 * sy / 3), zz.ravel()], axis=1))
    pts = np.concatenate(faces) + np.asarray(corner)
    return (pts + rng.uniform(-0.2 * voxel, 0.2 * voxel, pts.shape)).astype(f32)


def sample_reference(rng, store, m, noise, motion):
    """m rows of the store with Gaussian noise, moved by the INVERSE of `motion`: aligning them back should find `motion`."""
    pick = rng.choice(store.shape[0], m, replace=False)
    p = store[pick, :3].astype(np.float64) + rng.normal(0.0, noise, (m, 3))
    inv = inverse(motion)
    return (p @ inv[:, :3].T + inv[:, 3]).astype(f32)
