"""CPU-side checks of include/dmsa_dense_align_plane.h: the symbol list, the structs and defaults, P3-P5 of the library against the model
(tests/dense_align_plane_model.py, the yardstick of the GPU tests) bit for bit with the words in the device's uncarried limb form, the exact
re-centring against sums taken about the pivot directly, the invariance under flipped normals, the step against numpy's least squares, the
model's own convergence on the synthetic room, degenerate geometry, and the refusals that need no context.  P0's refusals with their
reasons need an object, which needs a device: they are in tests/test_gpu_dense_align_plane.py."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

from dmsa_lidar_slam_amd import _capi as capi
from dmsa_lidar_slam_amd import dense_cloud as dcl
from dmsa_lidar_slam_amd.api import DmsaError

import dense_align_model as am
import dense_align_plane_model as pm
import dense_normals_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
LIM = 2**30 - 1
REACH = 2**16 + 1  # a coordinate of G - P at the reach of 64 voxels, the quantisations included


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def _bits(values):
    return [struct.unpack("<Q", struct.pack("<d", float(v)))[0] for v in np.asarray(values, np.float64).reshape(-1)]


def _ints(a):
    return [[int(v) for v in row] for row in np.asarray(a).reshape(-1, 3)]


def _limbs(x, count):
    return [(x >> (32 * k)) & 0xFFFFFFFF for k in range(count - 1)] + [x >> (32 * (count - 1))]


def _pair_words(P, G, N, c=1, no_normal=0):
    """P2's 64 words as a device adds them: every limb summed pair by pair, no carry from a limb into the next; every pair taken c times."""
    w = [0] * 64
    w[1] = no_normal

    def add(at, x, count):
        for k, v in enumerate(_limbs(x, count)):
            w[at + k] += c * v

    for p, g, n in zip(_ints(P), _ints(G), _ints(N)):
        cr = pm.cross(p, n)
        e = sum((g[a] - p[a]) * n[a] for a in range(3))
        w[0] += c
        for a in range(3):
            w[2 + a] += c * p[a]
            add(47 + 2 * a, n[a] * e, 2)
            add(53 + 3 * a, cr[a] * e, 3)
            for b in range(3):
                add(11 + 2 * (3 * a + b), cr[a] * n[b], 2)
        for k, (a, b) in enumerate(pm.SYM):
            w[5 + k] += c * n[a] * n[b]
            add(29 + 3 * k, cr[a] * cr[b], 3)
        add(62, e * e, 2)
    return w


def _times(sums, c):
    """The sums of the same pairs taken c times each."""
    mul = lambda v: [mul(x) for x in v] if isinstance(v, list) else v * c
    return {k: (v if k == "no_normal" else mul(v)) for k, v in sums.items()}


def _unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    return np.rint(v / np.linalg.norm(v, axis=1, keepdims=True) * 16384.0).astype(np.int64)


def _noisy_pairs(rng, n, deg, spread=2**20, noise=30.0, offset=(0, 0, 0)):
    """n pairs of a small motion: G is where a rotation by `deg` and a shift of up to 1000 units take P, with noise; normals of any direction."""
    P = rng.integers(-spread, spread, (n, 3))
    T = am.rigid(deg, rng.normal(size=3), rng.uniform(-1000, 1000, 3))
    G = np.rint(P @ T[:, :3].T + T[:, 3] + rng.normal(0, noise, (n, 3))).astype(np.int64)
    off = np.asarray(offset, np.int64)
    return P + off, G + off, _unit_normals(rng, n)


def _solve_cases():
    rng = np.random.default_rng(31)
    cases = {}
    for k in range(12):
        P, G, N = _noisy_pairs(rng, int(rng.integers(6, 300)), float(rng.uniform(0, 1.5)))
        cases[f"random{k}"] = (pm.sums_of_pairs(_ints(P), _ints(G), _ints(N), no_normal=k), _pair_words(P, G, N, no_normal=k))
    P, G, N = _noisy_pairs(rng, 200, 0.5, offset=(2**29, -(2**29), 2**29 - 2**21))
    cases["far_from_the_origin"] = (pm.sums_of_pairs(_ints(P), _ints(G), _ints(N)), _pair_words(P, G, N))
    # the bounds: coordinates at +-(2^30 - 1) with mixed signs (c near 2^45 in both signs, the top limbs negative), N at both length bounds
    # (N^2 = 2^29 and 2^27), G - P at the reach in the direction of N (e near 2^30.5 in both signs), every pair 2^22 times: 2^25 pairs
    corners = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1], [1, 1, -1], [-1, 1, 1], [1, -1, 1], [-1, -1, -1]]) * LIM
    N = np.array([[16384, 16384, 0], [0, 16384, -16384], [23170, 0, 0], [0, -23170, 0], [0, 8192, 8192], [8192, 0, -8192], [0, 0, 11586], [-16384, 0, 16384]])
    assert all(2**27 <= int(n @ n) <= 2**29 for n in N) and int(N[0] @ N[0]) == 2**29 and int(N[4] @ N[4]) == 2**27
    G = corners - np.sign(corners) * (np.abs(N) > 0) * np.array([[REACH, 0, 0], [0, REACH, 0], [REACH, 0, 0], [0, REACH, 0], [0, REACH, 0], [REACH, 0, 0], [0, 0, REACH], [0, 0, REACH]])
    assert np.abs(G - corners).max() == REACH and np.abs(G).max() <= LIM
    cases["extreme"] = (_times(pm.sums_of_pairs(_ints(corners), _ints(G), _ints(N)), 2**22), _pair_words(corners, G, N, 2**22))
    P, G, N = _noisy_pairs(rng, 5, 0.5)
    cases["five_pairs"] = (pm.sums_of_pairs(_ints(P), _ints(G), _ints(N)), _pair_words(P, G, N))
    P, G, N = _noisy_pairs(rng, 80, 0.5)
    N[:] = (0, 0, 16384)
    cases["parallel_normals"] = (pm.sums_of_pairs(_ints(P), _ints(G), _ints(N)), _pair_words(P, G, N))
    N[::2] = (16384, 0, 0)
    cases["two_directions"] = (pm.sums_of_pairs(_ints(P), _ints(G), _ints(N)), _pair_words(P, G, N))
    P, G, N = _noisy_pairs(rng, 60, 0.0, noise=0.0)
    cases["identical"] = (pm.sums_of_pairs(_ints(P), _ints(P), _ints(N)), _pair_words(P, P, N))
    return cases


SOLVE_CASES = _solve_cases()
DEGENERATE = {"five_pairs", "parallel_normals", "two_directions"}


def test_symbol_tuple_equals_the_header_and_the_library_exports_it(lib):
    header = open(os.path.join(ROOT, "include", "dmsa_dense_align_plane.h")).read()
    declared = set(re.findall(r"\b(dmsa_[a-z_0-9]+)\s*\(", header.split("#ifndef DMSA_DENSE_ALIGN_PLANE_H")[1]))
    assert declared == set(capi.DENSE_ALIGN_PLANE_SYMBOLS) and len(capi.DENSE_ALIGN_PLANE_SYMBOLS) == len(declared) == 4
    others = (set(capi.EXPORTED_SYMBOLS) | set(capi.DENSE_CLOUD_SYMBOLS) | set(capi.DENSE_NORMALS_SYMBOLS) | set(capi.DENSE_OUTLIERS_SYMBOLS) | set(capi.DENSE_CARVE_SYMBOLS) |
              set(capi.DENSE_INTENSITY_SYMBOLS) | set(capi.DENSE_CLUSTERS_SYMBOLS) | set(capi.DENSE_COMPARE_SYMBOLS) | set(capi.DENSE_ALIGN_SYMBOLS))
    assert not declared & others
    for name in declared:
        assert hasattr(lib, name), name
    for rule in ("P0", "P1", "P2", "P3", "P4", "P5", "P6", "P7", "P8", "P9"):
        assert re.search(rf"\b{rule}\b", header)
    assert "DECIDED HERE" in header and "placeholders" in header and "does not detect" in header and "belongs to D0" in header


def test_structs_and_defaults(lib):
    assert C.sizeof(capi.DenseAlignPlaneConfig) == 32 and C.sizeof(capi.DenseAlignPlaneIteration) == 80
    assert C.sizeof(capi.DenseAlignPlaneReport) == 16 + 64 * 80 + 64 * 8 + 12 * 8
    cfg = capi.DenseAlignPlaneConfig(9.0, 9, 9, 9, 9.0, 9.0)
    lib.dmsa_default_dense_align_plane_config(C.byref(cfg))
    assert (cfg.max_distance, cfg.max_iterations, cfg.min_pairs, cfg.pad, cfg.stop_translation, cfg.stop_rotation) == (1.0, 30, 6, 0, 1e-4, 1e-5)
    lib.dmsa_default_dense_align_plane_config(None)
    assert capi.ALIGN_PLANE_STOP == ("CONVERGED", "MAX_ITERATIONS", "TOO_FEW_PAIRS", "DEGENERATE") == pm.STOPS and capi.ALIGN_PLANE_STOP[:3] == capi.ALIGN_STOP
    assert capi.ALIGN_PLANE_SUMS == 64 and capi.ALIGN_PLANE_DEGENERATE == 1
    # the header's constants are these
    header = open(os.path.join(ROOT, "include", "dmsa_dense_align_plane.h")).read()
    assert "#define DMSA_ALIGN_PLANE_SUMS 64" in header and "#define DMSA_ALIGN_STOP_DEGENERATE 3" in header and "#define DMSA_ALIGN_PLANE_DEGENERATE 1" in header


@pytest.mark.parametrize("name", sorted(SOLVE_CASES))
@pytest.mark.parametrize("scale_c", [1.0, 2.0**13])
def test_the_solve_equals_the_model_bit_for_bit(name, scale_c):
    sums, words = SOLVE_CASES[name]
    assert dcl._align_plane_sums(words) == sums  # the device's form recombines to the Python ints
    want = pm.solve(sums, scale_c)
    for given in (words, sums):
        dT, shift, rot, pivot, degenerate = dcl.align_plane_solve(given, scale_c)
        assert degenerate == want[4] == (name in DEGENERATE), (name, pivot, want[3])
        assert _bits(dT) == _bits(want[0]), (dT, want[0])
        assert _bits([shift, rot, pivot]) == _bits(want[1:4]), ((shift, rot, pivot), want[1:4])
    R = dT[:, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14
    if degenerate:
        assert np.array_equal(dT, np.eye(3, 4)) and shift == 0.0 and rot == 0.0 and pivot <= 2.0**-40
    else:
        assert 2.0**-40 < pivot <= 1.0
    if name == "identical":
        assert shift == 0.0 and rot == 0.0 and np.array_equal(dT, np.eye(3, 4))
    if name == "extreme":  # the words in the device's form: lower limbs far past 2^32, never carried; top limbs of both signs
        canonical = dcl.align_plane_sum_words(sums)
        assert words != canonical and max(words[29:47:3]) > 2**54 and min(words[11:29]) < -(2**49) and max(words[11:29]) > 2**49
        assert sums["n"] == 2**25 and max(sums["cc"]) > 2**113 and max(abs(v) for v in sums["ce"]) > 2**98 and sums["ee"] > 2**85
        assert max(abs(v) for v in pm.pivot_of(sums)) <= 1


def test_the_words_and_the_dict_are_one_thing():
    sums, words = SOLVE_CASES["extreme"]
    canonical = dcl.align_plane_sum_words(sums)
    assert len(canonical) == 64 and dcl._align_plane_sums(canonical) == sums and dcl.align_plane_sum_words(canonical) == canonical
    lower = [k for a, count, limbs in ((11, 9, 2), (29, 6, 3), (47, 3, 2), (53, 3, 3), (62, 1, 2)) for i in range(count) for k in range(a + limbs * i, a + limbs * i + limbs - 1)]
    assert len(lower) == 9 + 12 + 3 + 6 + 1 and all(0 <= canonical[k] < 2**32 for k in lower)
    with pytest.raises(ValueError):
        dcl.align_plane_sum_words(list(range(25)))


def test_the_recentring_is_exact_against_sums_taken_about_the_pivot_directly():
    """P3 moves the pivot in integers.  The yardstick takes c' = (P - C) x N pair by pair; on coordinates near 2^29 a float path would lose
    every low bit of it."""
    rng = np.random.default_rng(7)
    for offset in ((0, 0, 0), (2**29, -(2**29), 2**29 - 2**21), (-(2**30) + 2**21, 2**30 - 2**21, 12345)):
        P, G, N = _noisy_pairs(rng, 150, 1.0, offset=offset)
        sums = pm.sums_of_pairs(_ints(P), _ints(G), _ints(N))
        C_, A, b = pm.recentred(sums)
        assert all((2 * s + 150) // 300 == c and abs(c - m) <= 0.5 for s, c, m in zip(sums["sp"], C_, P.mean(axis=0)))
        direct = pm.sums_of_pairs(_ints(P), _ints(G), _ints(N), pivot=C_)
        for k, (i, j) in enumerate(pm.SYM):
            assert A[i][j] == A[j][i] == direct["cc"][k] and A[3 + i][3 + j] == A[3 + j][3 + i] == direct["nn"][k] == sums["nn"][k]
        for i in range(3):
            assert b[i] == direct["ce"][i] and b[3 + i] == direct["ne"][i] == sums["ne"][i]
            for j in range(3):
                assert A[i][3 + j] == A[3 + j][i] == direct["cn"][i][j]
        if offset != (0, 0, 0):
            assert max(sums["cc"]) > 2**18 * max(direct["cc"])  # what the origin's sums would cost a double solve


def test_the_sums_do_not_depend_on_the_orientation_of_the_normals():
    rng = np.random.default_rng(8)
    P, G, N = _noisy_pairs(rng, 120, 1.0)
    want, want_words = pm.sums_of_pairs(_ints(P), _ints(G), _ints(N)), dcl.align_plane_sum_words(dcl._align_plane_sums(_pair_words(P, G, N)))
    for _ in range(5):
        flip = np.where(rng.random(120) < 0.5, -1, 1)[:, None]
        assert pm.sums_of_pairs(_ints(P), _ints(G), _ints(N * flip)) == want
        assert dcl.align_plane_sum_words(dcl._align_plane_sums(_pair_words(P, G, N * flip))) == want_words
    assert pm.sums_of_pairs(_ints(P), _ints(G), _ints(-N)) == want


def test_the_step_against_numpys_least_squares():
    """The yardstick is numpy.linalg.lstsq on the same linearised problem in float64: rows [(P - C) x N, N], right-hand side e.  From its
    (omega, t) the rotation by P4's formula and the translation about the pivot, in numpy doubles.  Measured on this file's 40 cases (noisy
    pairs of 12 to 300 points within +-2^20 units, motions up to 1.5 degrees and 1000 units, 30 units of noise): the largest entry difference
    of R was 2.00e-17 and the largest difference of a translation entry, relative to the largest entry, 6.43e-14; the bounds are ten times
    these.  (Without the equilibration numpy's own answer is the worse one: the differences are then 3.7e-13 and 6.0e-11.)"""
    rng = np.random.default_rng(23)
    worst_r, worst_t = 0.0, 0.0
    for _ in range(40):
        P, G, N = _noisy_pairs(rng, int(rng.integers(12, 300)), float(rng.uniform(0, 1.5)))
        sums = pm.sums_of_pairs(_ints(P), _ints(G), _ints(N))
        dT, _, _, pivot, degenerate = dcl.align_plane_solve(sums)
        assert not degenerate and pivot > 1e-6
        Cp = np.array(pm.pivot_of(sums), np.float64)
        J = np.concatenate([np.cross(P - Cp, N), N.astype(np.float64)], axis=1)
        e = np.einsum("ij,ij->i", (G - P).astype(np.float64), N.astype(np.float64))
        col = np.linalg.norm(J, axis=0)  # (the columns of c' are 2^20 times those of N: the yardstick solves the equilibrated problem)
        x = np.linalg.lstsq(J / col, e, rcond=None)[0] / col
        h = x[:3] / 2
        w, (qx, qy, qz) = 1 / math.sqrt(1 + h @ h), h / math.sqrt(1 + h @ h)
        R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - w * qz), 2 * (qx * qz + w * qy)],
                      [2 * (qx * qy + w * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - w * qx)],
                      [2 * (qx * qz - w * qy), 2 * (qy * qz + w * qx), 1 - 2 * (qx * qx + qy * qy)]])
        t = Cp + x[3:] - R @ Cp
        worst_r = max(worst_r, float(np.abs(R - dT[:, :3]).max()))
        worst_t = max(worst_t, float(np.abs(t - dT[:, 3]).max() / max(1.0, np.abs(t).max())))
    print(f"largest entry difference to numpy's least squares: R {worst_r:.3e}, translation (relative) {worst_t:.3e}")
    assert worst_r < 2.00e-16 and worst_t < 6.43e-13


@pytest.fixture(scope="module")
def room_with_normals():
    """dense_align_model.room with N4's normals at 0.3 m: the moments of dense_normals_model, the library's dmsa_dense_normal_from_moments."""
    rng = np.random.default_rng(5)
    store = am.room(rng)
    normals = dcl.normal_from_moments(nm.moments(store, 0.3), -store[:, :3], 5)
    return rng, store, normals


def test_the_model_recovers_known_displacements_of_the_room(room_with_normals):
    """The room of tests/test_dense_align_cpu.py (4 920 store rows at 0.1 m voxels, 2 000 reference rows with 1 cm noise), displaced by 2
    degrees and 0.146 m, then by 5 degrees and 0.367 m, the normals N4's at 0.3 m.  Measured: CONVERGED after 3 and after 4 iterations,
    the entries of T within 2.31e-4 and 6.77e-4 of the applied motion, the smallest pivots 0.972 and 0.946.  Point to point on the same scenes (tests/test_dense_align_cpu.py):
    8 and 12 iterations, 2.96e-4 and 3.16e-4.  The bound is twice the larger error; the iteration counts are bounded by what was measured
    on these two scenes and claim nothing beyond them."""
    rng, store, normals = room_with_normals
    assert store.shape[0] == 4920 and np.isfinite(normals[:, :3]).all(axis=1).sum() > 4800
    for deg, shift, most in ((2.0, (0.1, -0.08, 0.07), 3), (5.0, (0.25, -0.2, 0.18), 4)):
        motion = am.rigid(deg, (0.2, -0.3, 1.0), shift)
        ref = am.sample_reference(rng, store, 2000, 0.01, motion)
        out = pm.align(store, normals, ref, 0.1)
        err = float(np.abs(np.array(out["transform"]).reshape(3, 4) - motion).max())
        h = out["history"]
        print(f"{deg} degrees: {out['iterations']} iterations, {out['stop']}, largest entry error {err:.3e}, min_pivot {min(x['min_pivot'] for x in h):.3f}")
        assert out["stop"] == "CONVERGED" and out["iterations"] <= most
        assert err < 1.354e-3
        assert h[0]["plane_rms_m"] > 2 * h[-1]["plane_rms_m"] and h[-1]["shift_m"] <= 1e-4 and h[-1]["rotation_rad"] <= 1e-5
        assert all(x["used"] + x["no_normal"] == x["matched"] and x["min_pivot"] > 1e-3 for x in h) and h[-1]["matched"] == 2000


def test_parallel_normals_are_degenerate_and_five_pairs_are_too_few():
    # a flat lattice with normals exactly +-e_z: the model's loop stops DEGENERATE at iteration 0 and applies nothing
    rng = np.random.default_rng(9)
    xs = np.arange(0.05, 3.0, 0.2)
    store = np.stack([*(v.ravel() for v in np.meshgrid(xs, xs, indexing="ij")), np.zeros(xs.size**2)], axis=1).astype(f32)
    normals = np.tile(np.array([0.0, 0.0, 1.0, 0.0], f32), (store.shape[0], 1))
    normals[::3, 2] = -1.0
    ref = (store + np.array([0.01, 0.0, 0.02])).astype(f32)
    T0 = am.rigid(0.2, (0, 0, 1), (0.0, 0.01, 0.0))
    out = pm.align(store, normals, ref, 0.1, T0=T0)
    assert out["stop"] == "DEGENERATE" and out["iterations"] == 1 and out["transform"] == list(T0.reshape(-1))
    h = out["history"][0]
    assert h["used"] == store.shape[0] and h["shift_m"] == 0.0 and h["rotation_rad"] == 0.0 and h["min_pivot"] <= 2.0**-40 and h["plane_rms_m"] > 0.01
    dT, shift, rot, pivot, degenerate = dcl.align_plane_solve(out["sums"], out["scale_c"])
    assert degenerate and _bits([pivot]) == _bits([h["min_pivot"]]) and np.array_equal(dT, np.eye(3, 4))
    # five used pairs: TOO_FEW_PAIRS before any solve, whatever the geometry
    normals5 = normals.copy()
    normals5[5:] = np.nan
    out = pm.align(store, normals5, ref, 0.1, max_distance=0.1)
    h = out["history"][0]
    assert out["stop"] == "TOO_FEW_PAIRS" and out["iterations"] == 1 and h["used"] == 5 and h["no_normal"] == store.shape[0] - 5 and h["min_pivot"] == 0.0
    assert out["transform"] == am.IDENTITY
    # and the solve alone calls five pairs of any geometry rank deficient
    assert dcl.align_plane_solve(SOLVE_CASES["five_pairs"][0])[4]


def test_normals_that_are_no_normals_are_not_used():
    rows = np.array([[0, 0, 1], [np.nan, 0, 1], [0, np.inf, 0], [0, 0, 0], [0.5, 0.5, 0], [0.5, 0.5, 0.01], [1, 1, 0], [1, 1, 0.01], [3e38, 0, 0], [0, 0, -1], [2.5, 0, 0]], f32)
    got = pm.quantise_normals(rows)
    assert [g is not None for g in got] == [True, False, False, False, True, True, True, False, False, True, False]
    assert got[0] == [0, 0, 16384] and got[4] == [8192, 8192, 0] and got[6] == [16384, 16384, 0] and got[9] == [0, 0, -16384]


def test_refusals_without_a_context(lib):
    cfg = capi.DenseAlignPlaneConfig()
    lib.dmsa_default_dense_align_plane_config(C.byref(cfg))
    words = (C.c_int64 * 64)()
    assert lib.dmsa_dense_cloud_align_plane_sums(None, C.byref(cfg), words, None) == -1
    assert lib.dmsa_dense_cloud_align_reference_plane(None, None, 0, 3, None, C.byref(cfg), None, None) == -1
    ok = dcl.align_plane_sum_words(SOLVE_CASES["random0"][0])
    dT = (C.c_double * 12)()
    assert lib.dmsa_dense_align_plane_solve((C.c_int64 * 64)(*ok), 1.0, dT, None, None, None) == 0
    assert lib.dmsa_dense_align_plane_solve(None, 1.0, dT, None, None, None) == -1
    assert lib.dmsa_dense_align_plane_solve((C.c_int64 * 64)(*ok), 1.0, None, None, None, None) == -1
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.dmsa_dense_align_plane_solve((C.c_int64 * 64)(*ok), scale, dT, None, None, None) == -1
    n = ok[0]
    for at, value in ((0, 0), (0, -3), (0, 2**26 + 1), (1, -1), (1, 2**26 - n + 1), (2, n * 2**30 + 1), (4, -(n * 2**30) - 1), (5, -1), (6, n * 2**29 + 1), (8, -1),
                      (11, -1), (11, n * 2**32), (12, n * 2**28 + 1), (28, -(n * 2**28) - 1), (29, -1), (30, n * 2**32), (31, n * 2**27 + 1), (46, -(n * 2**27) - 1),
                      (47, -1), (48, n * 2**14 + 1), (53, n * 2**32), (54, -1), (55, -(n * 2**13) - 1), (62, -1), (63, -1), (63, n * 2**30 + 1)):
        bad = list(ok)
        bad[at] = value
        with pytest.raises(DmsaError) as e:
            dcl.align_plane_solve(bad)
        assert e.value.status == -1, (at, value)
    # the limits themselves are legal
    edge = list(ok)
    edge[1], edge[12] = 2**26 - n, n * 2**28
    dcl.align_plane_solve(edge)
