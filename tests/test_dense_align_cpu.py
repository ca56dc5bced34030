"""CPU-side checks of include/dmsa_dense_align.h: the symbol list, the structs and defaults, A3-A5 of the library against the model
(tests/dense_align_model.py, the yardstick of the GPU tests) bit for bit, A3's rotation against numpy's SVD, the model's own convergence
on the synthetic room, the transform file, and the refusals that need no context.  A0's refusals with their reasons need an object, which
needs a device: they are in tests/test_gpu_dense_align.py."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
LIM = 2**30 - 1


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def _bits(values):
    return [struct.unpack("<Q", struct.pack("<d", float(v)))[0] for v in np.asarray(values, np.float64).reshape(-1)]


def _ints(a):
    return [[int(v) for v in row] for row in np.asarray(a).reshape(-1, 3)]


def _times(sums, c):
    """The sums of the same pairs taken c times each."""
    return dict(n=sums["n"] * c, sp=[v * c for v in sums["sp"]], sg=[v * c for v in sums["sg"]], spg=[[v * c for v in row] for row in sums["spg"]])


def _pair_words(P, G, c=1):
    """A2's 25 words as a device adds them: lo and hi summed pair by pair, no carry from lo into hi; every pair taken c times."""
    w = [0] * 25
    for p, g in zip(_ints(P), _ints(G)):
        w[0] += c
        for a in range(3):
            w[1 + a] += c * p[a]
            w[4 + a] += c * g[a]
            for b in range(3):
                w[7 + 2 * (3 * a + b)] += c * ((p[a] * g[b]) & 0xFFFFFFFF)
                w[8 + 2 * (3 * a + b)] += c * ((p[a] * g[b]) >> 32)
    return w


def _noisy_pairs(rng, n, deg, spread=2**20, noise=30.0):
    P = rng.integers(-spread, spread, (n, 3))
    T = am.rigid(deg, rng.normal(size=3), rng.uniform(-1000, 1000, 3))
    G = np.rint(P @ T[:, :3].T + T[:, 3] + rng.normal(0, noise, (n, 3))).astype(np.int64)
    return P, G


def _solve_cases():
    rng = np.random.default_rng(11)
    cases = {}
    for k in range(12):
        P, G = _noisy_pairs(rng, int(rng.integers(4, 300)), float(rng.uniform(0, 40)))
        cases[f"random{k}"] = am.sums_of_pairs(_ints(P), _ints(G))
    # coordinates at +-(2^30 - 1), 2^26 pairs, a half turn about x: M = n^2 LIM^2 diag(1, -1, -1) is near 2^112 in both signs, every product is
    # near 2^60; and the same magnitudes all of one sign: n * Spg and Sp * Sg are both near 2^112 and M is their small exact difference
    corners = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1], [1, 1, -1], [-1, 1, 1], [1, -1, 1], [-1, -1, -1]]) * LIM
    turned = corners * np.array([1, -1, -1])
    cases["extreme"] = _times(am.sums_of_pairs(_ints(corners), _ints(turned)), 2**23)
    EXTREME_WORDS["extreme"] = _pair_words(corners, turned, 2**23)
    one_p, one_g = np.abs(corners) - np.arange(8)[:, None], -np.abs(turned) + np.arange(8)[:, None] * 3
    cases["extreme_one_sign"] = _times(am.sums_of_pairs(_ints(one_p), _ints(one_g)), 2**23)
    EXTREME_WORDS["extreme_one_sign"] = _pair_words(one_p, one_g, 2**23)
    P, G = _noisy_pairs(rng, 3, 10.0)
    cases["three"] = am.sums_of_pairs(_ints(P), _ints(G))
    line = np.outer(np.arange(-20, 21), [3, -2, 5]) * 1000
    cases["collinear"] = am.sums_of_pairs(_ints(line), _ints(line[:, [1, 0, 2]] + 17))
    cases["collinear_same"] = am.sums_of_pairs(_ints(line), _ints(line))
    P, _ = _noisy_pairs(rng, 50, 0.0)
    cases["identical"] = am.sums_of_pairs(_ints(P), _ints(P))
    cases["zero_m"] = am.sums_of_pairs([[5, -7, 11]] * 9, [[100, 200, -300]] * 9)
    cases["half_turn"] = am.sums_of_pairs(_ints(P), _ints(P * np.array([-1, -1, 1])))
    return cases


EXTREME_WORDS = {}
SOLVE_CASES = _solve_cases()


def test_symbol_tuple_equals_the_header_and_the_library_exports_it(lib):
    header = open(os.path.join(ROOT, "include", "dmsa_dense_align.h")).read()
    declared = set(re.findall(r"\b(dmsa_[a-z_0-9]+)\s*\(", header.split("#ifndef DMSA_DENSE_ALIGN_H")[1]))
    assert declared == set(capi.DENSE_ALIGN_SYMBOLS) and len(capi.DENSE_ALIGN_SYMBOLS) == len(declared) == 6
    others = (set(capi.EXPORTED_SYMBOLS) | set(capi.DENSE_CLOUD_SYMBOLS) | set(capi.DENSE_NORMALS_SYMBOLS) | set(capi.DENSE_OUTLIERS_SYMBOLS) |
              set(capi.DENSE_CARVE_SYMBOLS) | set(capi.DENSE_INTENSITY_SYMBOLS) | set(capi.DENSE_CLUSTERS_SYMBOLS) | set(capi.DENSE_COMPARE_SYMBOLS))
    assert not declared & others
    for name in declared:
        assert hasattr(lib, name), name
    for rule in ("A0", "A1", "A2", "A3", "A4", "A5", "A6", "A7", "A8"):
        assert re.search(rf"\b{rule}\b", header)
    assert "DECIDED HERE" in header and "placeholders" in header and "90 km" in header


def test_structs_and_defaults(lib):
    assert C.sizeof(capi.DenseAlignConfig) == 32 and C.sizeof(capi.DenseAlignIteration) == 48
    assert C.sizeof(capi.DenseAlignReport) == 16 + 64 * 48 + 25 * 8 + 12 * 8
    cfg = capi.DenseAlignConfig(9.0, 9, 9, 9, 9.0, 9.0)
    lib.dmsa_default_dense_align_config(C.byref(cfg))
    assert (cfg.max_distance, cfg.max_iterations, cfg.min_pairs, cfg.pad, cfg.stop_translation, cfg.stop_rotation) == (1.0, 30, 3, 0, 1e-4, 1e-5)
    lib.dmsa_default_dense_align_config(None)
    assert capi.ALIGN_STOP == ("CONVERGED", "MAX_ITERATIONS", "TOO_FEW_PAIRS") == am.STOPS
    for voxel in (0.1, 0.05, 0.5, 1.0, 0.25, 3.0):
        assert lib.dmsa_dense_align_scale(voxel) == am.scale_c_of(voxel)
    assert lib.dmsa_dense_align_scale(0.0) == 0.0 and lib.dmsa_dense_align_scale(-1.0) == 0.0 and lib.dmsa_dense_align_scale(float("nan")) == 0.0
    assert am.scale_c_of(0.1) == 2.0**13  # 0.1 = 0.8 * 2^-3


@pytest.mark.parametrize("name", sorted(SOLVE_CASES))
@pytest.mark.parametrize("scale_c", [1.0, 2.0**13])
def test_the_solve_equals_the_model_bit_for_bit(name, scale_c):
    sums = SOLVE_CASES[name]
    dT, shift, rot = dcl.align_solve(sums, scale_c)
    want_T, want_shift, want_rot = am.solve(sums, scale_c)
    assert _bits(dT) == _bits(want_T), (dT, want_T)
    assert _bits([shift, rot]) == _bits([want_shift, want_rot])
    R = dT[:, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14
    if name == "identical":
        assert shift == 0.0 and np.abs(dT - np.eye(3, 4)).max() < 1e-14
    if name == "collinear_same":  # every rotation about the line is a best fit (Horn's largest eigenvalue is double): the line stays where it is
        u = np.array([3.0, -2.0, 5.0]) / math.sqrt(38.0)
        assert shift == 0.0 and np.abs(R @ u - u).max() < 1e-14 and np.abs(dT[:, 3]).max() < 1e-9
    if name == "zero_m":
        assert all(v == 0 for row in am.centred(sums) for v in row) and np.array_equal(R, np.eye(3)) and rot == 0.0
        assert np.array_equal(dT[:, 3], np.array([95.0, 207.0, -311.0]) / scale_c)
    if name.startswith("extreme"):
        M = am.centred(sums)
        words = EXTREME_WORDS[name]  # the same sums in the device's form: lo far past 2^32, never carried into hi
        assert dcl._align_sums(words) == sums and words != dcl.align_sum_words(sums) and max(words[7::2]) > 2**55
        again = dcl.align_solve(words, scale_c)
        assert _bits(again[0]) == _bits(want_T) and again[1:] == (want_shift, want_rot)
        if name == "extreme":
            assert M[0][0] > 2**111 and M[1][1] < -(2**111) and min(words[8::2]) < -(2**52) and max(words[8::2]) > 2**52  # hi of both signs
            assert abs(rot - 2.0) < 1e-12 and np.abs(R - np.diag([1.0, -1.0, -1.0])).max() < 1e-12
        else:
            assert -sums["n"] * sums["spg"][0][0] > 2**111 and 0 < max(abs(v) for row in M for v in row) < 2**70
    if name == "half_turn":
        assert abs(rot - 2.0) < 1e-12 and np.abs(R - np.diag([-1.0, -1.0, 1.0])).max() < 1e-12


def test_the_words_and_the_dict_are_one_thing():
    sums = SOLVE_CASES["extreme"]
    words = dcl.align_sum_words(sums)
    assert len(words) == 25 and dcl._align_sums(words) == sums and dcl.align_sum_words(words) == words
    assert all(0 <= w for w in words[7::2])
    a, b = dcl.align_solve(sums), dcl.align_solve(words)
    assert _bits(a[0]) == _bits(b[0]) and a[1:] == b[1:]


def test_the_rotation_against_numpys_svd():
    """The yardstick is numpy.linalg.svd's Kabsch rotation from the same integer pairs in float64.  Measured on this file's 40 cases (noisy
    pairs of 4 to 300 points, rotations up to 40 degrees): the largest entry difference was 1.36e-15; the bound is ten times that."""
    rng = np.random.default_rng(23)
    worst = 0.0
    for _ in range(40):
        P, G = _noisy_pairs(rng, int(rng.integers(4, 300)), float(rng.uniform(0, 40)))
        dT, _, _ = dcl.align_solve(am.sums_of_pairs(_ints(P), _ints(G)))
        Pc, Gc = P - P.mean(axis=0), G - G.mean(axis=0)
        U, _, Vt = np.linalg.svd(Pc.T.astype(np.float64) @ Gc.astype(np.float64))
        d = np.sign(np.linalg.det(Vt.T @ U.T))
        R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
        worst = max(worst, float(np.abs(R - dT[:, :3]).max()))
        t = G.mean(axis=0) - R @ P.mean(axis=0)
        assert np.abs(t - dT[:, 3]).max() < 1e-6 * max(1.0, np.abs(t).max())
    print(f"largest entry difference to numpy's Kabsch rotation: {worst:.3e}")
    assert worst < 1.36e-14


def test_the_composition_equals_the_model_bit_for_bit():
    rng = np.random.default_rng(4)
    for _ in range(10):
        D = am.rigid(float(rng.uniform(-5, 5)), rng.normal(size=3), rng.uniform(-1, 1, 3))
        T = am.rigid(float(rng.uniform(-180, 180)), rng.normal(size=3), rng.uniform(-100, 100, 3))
        got = dcl.align_compose(D, T)
        assert _bits(got) == _bits(am.compose(list(D.reshape(-1)), list(T.reshape(-1))))
        full = np.vstack([D, [0, 0, 0, 1]]) @ np.vstack([T, [0, 0, 0, 1]])
        assert np.abs(got - full[:3]).max() < 1e-12


@pytest.mark.parametrize("deg,shift,most", [(2.0, (0.1, -0.08, 0.07), 10), (5.0, (0.25, -0.2, 0.18), 20)])
def test_the_model_recovers_a_known_displacement_of_the_room(deg, shift, most):
    """An 8 x 6 x 3 m box with two inner faces at 0.1 m voxels: 4 920 store rows, 2 000 reference rows with 1 cm noise, displaced by 2 degrees
    and 0.146 m, and by 5 degrees and 0.367 m.  Measured: CONVERGED after 8 and after 12 iterations, the entries of T within 2.96e-4 and
    3.16e-4 of the applied motion; the bound is twice the larger."""
    rng = np.random.default_rng(5)
    store = am.room(rng)
    motion = am.rigid(deg, (0.2, -0.3, 1.0), shift)
    ref = am.sample_reference(rng, store, 2000, 0.01, motion)
    out = am.align(store, ref, 0.1)
    T = np.array(out["transform"]).reshape(3, 4)
    err = float(np.abs(T - motion).max())
    print(f"{deg} degrees: {out['iterations']} iterations, {out['stop']}, largest entry error {err:.3e}")
    assert store.shape[0] == 4920 and out["stop"] == "CONVERGED" and out["iterations"] <= most <= 20
    assert err < 6.4e-4
    h = out["history"]
    assert h[0]["rms_m"] > 2 * h[-1]["rms_m"] and h[-1]["shift_m"] <= 1e-4 and h[-1]["rotation_rad"] <= 1e-5 and h[-1]["matched"] == 2000


def test_the_transform_file_round_trips_twelve_doubles(tmp_path):
    rng = np.random.default_rng(9)
    T = am.rigid(33.3, rng.normal(size=3), rng.uniform(-1e5, 1e5, 3))
    T[0, 1], T[2, 3] = 1e-300, -math.pi * 1e8
    path = tmp_path / "T.txt"
    dcl.write_transform(path, T)
    lines = open(path).read().splitlines()
    assert len(lines) == 3 and all(len(line.split()) == 4 for line in lines)
    assert _bits(dcl.read_transform(path)) == _bits(T)
    dcl.write_transform(path, np.vstack([T, [0, 0, 0, 1]]))  # a 4x4: its upper rows
    assert _bits(dcl.read_transform(path)) == _bits(T)
    open(path, "w").write("1 2 3\n")
    with pytest.raises(ValueError):
        dcl.read_transform(path)


def test_refusals_without_a_context(lib):
    cfg = capi.DenseAlignConfig()
    lib.dmsa_default_dense_align_config(C.byref(cfg))
    words = (C.c_int64 * 25)()
    assert lib.dmsa_dense_cloud_align_sums(None, C.byref(cfg), words, None) == -1
    assert lib.dmsa_dense_cloud_align_reference(None, None, 0, 3, None, C.byref(cfg), None, None) == -1
    ok = dcl.align_sum_words(SOLVE_CASES["three"])
    dT = (C.c_double * 12)()
    assert lib.dmsa_dense_align_solve((C.c_int64 * 25)(*ok), 1.0, dT, None, None) == 0
    assert lib.dmsa_dense_align_solve(None, 1.0, dT, None, None) == -1 and lib.dmsa_dense_align_solve((C.c_int64 * 25)(*ok), 1.0, None, None, None) == -1
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.dmsa_dense_align_solve((C.c_int64 * 25)(*ok), scale, dT, None, None) == -1
    for at, value in ((0, 0), (0, -3), (0, 2**26 + 1), (1, 3 * 2**30 + 1), (5, -(3 * 2**30) - 1), (7, -1), (7, 3 * 2**32), (8, 3 * 2**28 + 1), (24, -(3 * 2**28) - 1)):
        bad = list(ok)
        bad[at] = value
        with pytest.raises(DmsaError) as e:
            dcl.align_solve(bad)
        assert e.value.status == -1
    assert lib.dmsa_dense_align_compose(None, dT, dT) == -1
