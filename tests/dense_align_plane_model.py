"""The independent model of include/dmsa_dense_align_plane.h, P0-P9: the yardstick of tests/test_gpu_dense_align_plane.py.

The pairs come from dense_compare_model.nearest; the store's normals are an argument ((rows, >= 3) float32, NaN where a row has none);
quantisation, the per-pair integers and all sums are Python ints of any size; the re-centring is Python ints written as sums over
explicit 3 x 3 matrices, not as the library's formulas; P4 is pure-Python floats, operation for operation as the header states (a Python
float operation is one IEEE double operation, rounded on its own; float(int) rounds to nearest even).  Composition is A5
(dense_align_model.compose).  Nothing here knows of cells, waves or limbs."""
import math

import numpy as np

import dense_align_model as am
import dense_compare_model as dm

f32 = np.float32
STOPS = ("CONVERGED", "MAX_ITERATIONS", "TOO_FEW_PAIRS", "DEGENERATE")
SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # xx xy xz yy yz zz
LEAST_PIVOT = 2.0**-40


def quantise_normals(normals):
    """P1: per row the integer normal, or None where the row has no normal."""
    out = []
    for row in np.asarray(normals, f32)[:, :3]:
        if not all(abs(float(v)) <= 2.0 for v in row):  # (NaN, infinity, or a component whose square alone is past 2^29)
            out.append(None)
            continue
        N = [int(np.rint(f32(v) * f32(16384.0))) for v in row]  # (the product is exact; to nearest even)
        out.append(N if 2**27 <= N[0] * N[0] + N[1] * N[1] + N[2] * N[2] <= 2**29 else None)
    return out


def cross(p, n):
    return [p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0]]


def sums_of_pairs(P, G, N, no_normal=0, pivot=(0, 0, 0)):
    """P2 over the quantised used pairs (lists of int triples), Python ints; with `pivot` the c are taken about it directly: (P - pivot) x N."""
    out = dict(n=len(P), no_normal=no_normal, sp=[0, 0, 0], nn=[0] * 6, cn=[[0, 0, 0] for _ in range(3)], cc=[0] * 6, ne=[0, 0, 0], ce=[0, 0, 0], ee=0)
    for p, g, n in zip(P, G, N):
        c = cross([p[a] - pivot[a] for a in range(3)], n)
        e = sum((g[a] - p[a]) * n[a] for a in range(3))
        for a in range(3):
            out["sp"][a] += p[a]
            out["ne"][a] += n[a] * e
            out["ce"][a] += c[a] * e
            for b in range(3):
                out["cn"][a][b] += c[a] * n[b]
        for k, (a, b) in enumerate(SYM):
            out["nn"][k] += n[a] * n[b]
            out["cc"][k] += c[a] * c[b]
        out["ee"] += e * e
    return out


def plane_sums(store, normals, ref, ref_valid, max_distance, voxel):
    """P1-P2 of the reference as it stands: (sums, d2 of the completeness direction, index)."""
    store, ref = np.asarray(store, f32)[:, :3], np.asarray(ref, f32)[:, :3]
    d2, idx = dm.nearest(ref, store, max_distance, q_valid=ref_valid)
    got = np.flatnonzero(idx >= 0)
    sc = am.scale_c_of(voxel)
    Nq = quantise_normals(normals)
    P, G = am.quantise(ref[got], sc), am.quantise(store[idx[got]], sc)
    use = [k for k, j in enumerate(idx[got]) if Nq[j] is not None]
    return sums_of_pairs([P[k] for k in use], [G[k] for k in use], [Nq[idx[got][k]] for k in use], no_normal=len(got) - len(use)), d2, idx


def _sym(v):
    return [[v[SYM.index((min(a, b), max(a, b)))] for b in range(3)] for a in range(3)]


def _mat(A, B):
    return [[sum(A[a][k] * B[k][b] for k in range(3)) for b in range(3)] for a in range(3)]


def _tr(A):
    return [[A[b][a] for b in range(3)] for a in range(3)]


def pivot_of(sums):
    """P3: C_a = floor((2 Sp_a + n) / (2 n))."""
    return [(2 * v + sums["n"]) // (2 * sums["n"]) for v in sums["sp"]]


def recentred(sums):
    """P3 in Python ints: (C, the 6 x 6 matrix A, b).  c' = c - K N, so  c'N^T = cN^T - K NN,  c'c'^T = cc^T - cN^T K^T - K Nc^T + K NN K^T,
    c'e = ce - K Ne, as matrix products."""
    C = pivot_of(sums)
    K = [[0, -C[2], C[1]], [C[2], 0, -C[0]], [-C[1], C[0], 0]]
    NN, cc, cN = _sym(sums["nn"]), _sym(sums["cc"]), sums["cn"]
    KNN = _mat(K, NN)
    cNp = [[cN[a][b] - KNN[a][b] for b in range(3)] for a in range(3)]
    t1, t2, t3 = _mat(cN, _tr(K)), _mat(K, _tr(cN)), _mat(KNN, _tr(K))
    ccp = [[cc[a][b] - t1[a][b] - t2[a][b] + t3[a][b] for b in range(3)] for a in range(3)]
    cep = [sums["ce"][a] - sum(K[a][k] * sums["ne"][k] for k in range(3)) for a in range(3)]
    A = [[0] * 6 for _ in range(6)]
    for a in range(3):
        for b in range(3):
            A[a][b], A[a][3 + b], A[3 + b][a], A[3 + a][3 + b] = ccp[a][b], cNp[a][b], cNp[a][b], NN[a][b]
    return C, A, cep + list(sums["ne"])


def solve(sums, scale_c=1.0):
    """P3-P5: (dT as 12 floats row-major, shift_m, rotation_rad, min_pivot, degenerate)."""
    identity = list(am.IDENTITY)
    C, Ai, bi = recentred(sums)
    A = [[float(v) for v in row] for row in Ai]
    b = [float(v) for v in bi]
    for i in range(6):
        if not A[i][i] > 0.0:
            return identity, 0.0, 0.0, 0.0, True
    s = [1.0 / math.sqrt(A[i][i]) for i in range(6)]
    M = [[(A[i][j] * s[i]) * s[j] if j <= i else None for j in range(6)] for i in range(6)]
    r = [b[i] * s[i] for i in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        v = M[j][j]
        for k in range(j):
            v = v - (L[j][k] * D[k]) * L[j][k]
        D[j] = v
        if not v > LEAST_PIVOT:
            return identity, 0.0, 0.0, v, True
        for i in range(j + 1, 6):
            u = M[i][j]
            for k in range(j):
                u = u - (L[i][k] * D[k]) * L[j][k]
            L[i][j] = u / v
    x = [0.0] * 6
    for i in range(6):
        y = r[i]
        for k in range(i):
            y = y - L[i][k] * x[k]
        x[i] = y
    x = [x[i] / D[i] for i in range(6)]
    for i in range(5, -1, -1):
        y = x[i]
        for k in range(i + 1, 6):
            y = y - L[k][i] * x[k]
        x[i] = y
    x = [x[i] * s[i] for i in range(6)]
    hx, hy, hz = x[0] * 0.5, x[1] * 0.5, x[2] * 0.5
    nr = math.sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz)
    w, qx, qy, qz = 1.0 / nr, hx / nr, hy / nr, hz / nr
    xx, yy, zz, xy, xz, yz, wx, wy, wz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, w * qx, w * qy, w * qz
    R = [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
         [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
         [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]
    Cd = [float(v) for v in C]
    dT = []
    for a in range(3):
        dT += [R[a][0], R[a][1], R[a][2], ((Cd[a] + x[3 + a]) - ((R[a][0] * Cd[0] + R[a][1] * Cd[1]) + R[a][2] * Cd[2])) / scale_c]
    shift = math.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]) / scale_c
    return dT, shift, 2.0 * math.sqrt((xx + yy) + zz), min(D), False


def align(store, normals, raw, voxel, T0=None, max_distance=1.0, max_iterations=30, min_pairs=6, stop_translation=1e-4, stop_rotation=1e-5):
    """P1-P9 as DenseCloudCreator.align_reference(metric="plane") returns it (transform as 12 floats)."""
    store, raw = np.asarray(store, f32)[:, :3], np.asarray(raw, f32)[:, :3]
    T = [float(v) for v in (am.IDENTITY if T0 is None else np.asarray(T0, np.float64)[:3, :4].reshape(-1))]
    sc = am.scale_c_of(voxel)
    history, stop, sums = [], "MAX_ITERATIONS", None
    for _ in range(max_iterations):
        ref = dm.transform(raw, np.array(T).reshape(3, 4))
        valid = dm.valid_rows(ref, voxel)
        sums, d2, _ = plane_sums(store, normals, ref, valid, max_distance, voxel)
        d4 = dm.direction(d2, valid, max_distance, max_distance)
        it = dict(matched=d4["matched"], unmatched=d4["unmatched"], s2=d4["s2"], used=sums["n"], no_normal=sums["no_normal"], rms_m=d4["rms_m"], plane_rms_m=0.0,
                  shift_m=0.0, rotation_rad=0.0, min_pivot=0.0)
        history.append(it)
        assert d4["matched"] == sums["n"] + sums["no_normal"]
        if sums["n"] > 0:
            it["plane_rms_m"] = math.sqrt(float(sums["ee"]) / float(sums["n"])) / (sc * 16384.0)
        if sums["n"] < min_pairs:
            stop = "TOO_FEW_PAIRS"
            break
        dT, it["shift_m"], it["rotation_rad"], it["min_pivot"], degenerate = solve(sums, sc)
        if degenerate:
            stop = "DEGENERATE"
            break
        T = am.compose(dT, T)
        if it["shift_m"] <= stop_translation and it["rotation_rad"] <= stop_rotation:
            stop = "CONVERGED"
            break
    return dict(transform=T, iterations=len(history), stop=stop, scale_c=sc, history=history, sums=sums)
