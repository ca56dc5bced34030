"""The constructed clouds of tests/size_edge_cloud.py really have the member counts they promise (CPU oracle): every count read from the
kernels' constants is a Gaussian at both resolutions, 9 members at none, nothing merged or cut by a cell edge -- the condition under which
tests/test_gpu_size_edges.py pins the size-class boundaries of the kernels."""
import numpy as np
import pytest

import size_edge_cloud as sec
from dmsa_lidar_slam_amd.problems import DmsaOptimSettings


def test_count_list_holds_every_boundary_of_the_sources(orc):
    c = sec.constants()
    assert sec.eigen_kc(orc) == (680, 1016)  # include/dmsa_debug.h: eigen_l1_bytes 32768 -> 680, 49152 -> 1016
    counts = sec.count_list(orc)
    for name, straddle in sec.boundaries(orc).items():
        assert len(straddle) >= 2 and set(straddle) <= set(counts), name
    # the list the issue tried on the oracle is a subset
    tried = [10, 11, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 680, 681, 767, 768, 769, 1016, 1017, 1023, 1024, 1025, 1360, 1361,
             2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 8191, 8192, 8193]
    assert set(tried) <= set(counts)
    for v in (2 * 680, 2 * 680 + 1, 2 * 1016, 2 * 1016 + 1, c["long_chunk"], c["long_chunk"] + 1, (1 << c["long_log2"]) - 1, 1 << c["long_log2"]):
        assert v in counts


@pytest.mark.parametrize("seed", [0, 1])
def test_every_requested_count_is_a_gaussian_at_both_resolutions(orc, seed):
    counts = sec.count_list(orc)
    prob, s, off = sec.window(counts, seed)
    assert s.min_num_points_per_set == sec.MIN_POINTS
    glob, ids = sec.global_points(orc, prob)
    G = orc.Gaussians(glob, ids, prob.minGridSize, s)
    found = sec.check_clusters(G, prob.localPoints.shape[0], off, counts)
    sizes = np.diff(G.seg_offset)
    for i, n in enumerate(counts):
        assert [int(sizes[g]) for g in found[i]] == ([n, n] if n >= sec.MIN_POINTS else [])
    assert G.M >= 2 * (len(counts) - 1)
    # both sides of limitCovariance's 1e-4 clamp occur among the clusters' covariances, in every shape
    _, cov, _ = G.fit_sums()
    ev = np.array([np.linalg.eigvalsh(cov[found[i][0]].reshape(3, 3).astype(np.float64)) for i in range(1, len(counts))])
    above = (ev > 1e-4).sum(axis=1)
    assert {0, 1, 2, 3} <= set(above.tolist()), sorted(set(above.tolist()))


@pytest.mark.parametrize("case", ["noisy", "duplicates", "flipped_tail"])
def test_split_leaves_come_out_as_their_prescribed_halves(orc, case):
    prob, s, off, leaves = sec.keyframes(case)
    _, g, n4 = sec.keyframe_global(orc, prob)
    a, b = sec.KEY_FIRST, sec.KEY_FIRST + off[-1]
    assert np.array_equal(g[a:b, :3], prob.localPoints[a:b, :3])  # frame 0 is the identity
    G = orc.Gaussians(g, prob.ringIds, prob.minGridSize, s, normals4=n4)
    G0 = orc.Gaussians(g, prob.ringIds, prob.minGridSize, DmsaOptimSettings(min_num_points_per_set=sec.MIN_POINTS), normals4=n4)
    sec.check_split(G, G0, off, leaves)
    assert (G.M, G.Mm) != (G0.M, G0.Mm)
