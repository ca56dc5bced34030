"""k_leaf_finalize (csrc/dmsa_kernels.hip), the chained scan of (accepted sets, members) over the leaves, at the sizes where its tile frame
and its look-back (csrc/chained_scan.h) can go wrong: one tile of 4096 leaves +- 1, and 64, 65 and 129 tiles -- one full round of the
look-back, a second round that consumes one lane, a third.

The kernel has no hook of its own: it is reached through upload -> pose tables -> updateGlobalPoints -> buildGaussians, as in
tests/test_gpu_lattice_hint.py.  The cloud has L occupied voxels of the finer level with two points each; every third voxel carries one
ring id twice and is rejected (max(id) != min(id)), so the accepted flags vary along the scan.  The first point is the origin: the voxel
lattice of both levels is pinned to it (pcl_octree_model.PclOctree._adopt), every box bound is a small integer multiple of the resolution,
and every other point lies at 0.2 or 0.3 of its fine voxel -- at least 0.06 m from every face of both levels.

small_voxel = 0 (its default) is stated in every context: the one-launch path of small windows never runs k_leaf_finalize.
"""
import dataclasses

import numpy as np
import pytest

import lattice_cases as lc
from dmsa_lidar_slam_amd.problems import ContinuousTrajectory, DmsaOptimSettings

pytestmark = pytest.mark.gpu

F32 = np.float32
S = dataclasses.replace(DmsaOptimSettings.sliding_window(), min_num_points_per_set=2)
TILE = 4096  # kFinTile: leaves per tile of k_leaf_finalize
SIZES = [1, TILE - 1, TILE, TILE + 1, 64 * TILE, 64 * TILE + 1, 2 * 64 * TILE + 1]


def _cloud(L):
    """(problem, expected (M, Mm) of level 0 and level 1) -- voxel v = (i, j, k) of a cube, points 2 v and 2 v + 1"""
    res = lc.resolutions()
    assert res[0] < res[1]
    side = int(np.ceil(L ** (1.0 / 3.0) - 1e-9))
    while side ** 3 < L:
        side += 1
    v = np.arange(L)
    ijk = np.stack([v % side, (v // side) % side, v // (side * side)], axis=1).astype(np.float64)
    xyz = np.empty((2 * L, 3), F32)
    xyz[0::2] = ((ijk + 0.2) * res[0]).astype(F32)
    xyz[1::2] = ((ijk + 0.3) * res[0]).astype(F32)
    xyz[0] = 0.0
    ring = np.zeros(2 * L, np.int64)
    ring[1::2] = (v % 3 != 0)
    # the model: a leaf is accepted iff it has >= 2 points and two different ring ids
    mixed = v % 3 != 0
    cell = np.floor(xyz[0::2].astype(np.float64) / res[1]).astype(np.int64)
    assert np.array_equal(cell, np.floor(xyz[1::2].astype(np.float64) / res[1]).astype(np.int64))
    _, of_cell = np.unique(cell, axis=0, return_inverse=True)
    of_cell = of_cell.reshape(-1)
    acc1 = np.bincount(of_cell, weights=mixed) > 0
    size1 = 2 * np.bincount(of_cell)
    expect = ((int(mixed.sum()), 2 * int(mixed.sum())), (int(acc1.sum()), int(size1[acc1].sum())))
    rows = np.arange(2 * L) % 2
    prob = ContinuousTrajectory(relOrientations=np.zeros((3, 3)), relTranslations=np.zeros((3, 3)), stamps=np.array([0.0, 0.05, 0.1]),
                                trajTime=np.linspace(0.0, 0.1, lc.TABLE_ROWS), localPoints=xyz, tformIdPerPoint=rows, ringIds=ring,
                                minGridSize=lc.MIN_GRID)
    return prob, expect


def _build(opt, prob, L):
    opt.upload(prob)
    opt.setPoseTables(lc.pose_tables())
    glob = opt.updateGlobalPoints(0)
    assert np.array_equal(glob[:, :3].view(np.uint32), np.asarray(prob.localPoints, F32)[:, :3].view(np.uint32))
    counts = opt.buildGaussians(S)
    info = opt.voxelLevel(0)[0]
    assert info.num_leaves == L, (L, info.num_leaves)  # otherwise the case is vacuous
    return glob, counts, opt.gaussians()


def _same(got, want, what):
    assert got[1] == want[1], (what, got[1], want[1])
    for a, b, name in zip(got[2], want[2], ("seg", "members", "info", "weights")):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name)


@pytest.mark.parametrize("L", SIZES)
def test_leaf_finalize_against_the_single_workgroup_scan_the_model_and_the_oracle(hip, orc, L):
    prob, expect = _cloud(L)
    want_counts = (expect[0][0] + expect[1][0], expect[0][1] + expect[1][1])
    runs = {}
    for name, debug in (("default", {"small_voxel": 0}), ("one workgroup", {"small_voxel": 0, "fused_leaf_scan": 0})):
        opt = hip.DmsaOptimizer(debug=debug)
        first = _build(opt, prob, L)
        second = _build(opt, prob, L)  # a non-zero ticket base and a new epoch over the first call's words
        _same(second, first, (L, name, "second build"))
        if name == "default":
            classes = opt.levelSizeClasses()
        opt.close()
        runs[name] = first
    print(f"L={L}: (M, Mm) = {runs['default'][1]}, model {want_counts}")
    _same(runs["default"], runs["one workgroup"], (L, "k_leaf_scan"))
    assert runs["default"][1] == want_counts, (L, runs["default"][1], want_counts)
    seg = runs["default"][2][0]
    assert np.array_equal(np.diff(seg[: expect[0][0] + 1]), np.full(expect[0][0], 2)), L  # level 0: every accepted leaf has its two points
    if L <= TILE + 1:
        glob = runs["default"][0]
        ref = orc.Gaussians(glob, prob.ringIds, prob.minGridSize, S)
        _same((glob, (ref.M, ref.Mm), (ref.seg_offset, ref.members, ref.info, ref.weights)), runs["default"], (L, "oracle"))
    if L == 64 * TILE + 1:  # the finalisation's gauss_size output: the fit by level, whatever the size
        opt = hip.DmsaOptimizer(debug={"small_voxel": 0, "fit_by_level": 2})
        forced = _build(opt, prob, L)
        _same(_build(opt, prob, L), forced, (L, "fit_by_level", "second build"))
        forced_classes = opt.levelSizeClasses()
        opt.close()
        assert forced_classes[1]
        assert np.array_equal(forced_classes[0], classes[0]), (forced_classes, classes)
        _same(forced, runs["default"], (L, "fit_by_level"))
