"""GPU tests of what the three stages over the dense cloud share (csrc/dense_cloud_obj.h): the retained store, the search grid over it and one row
mask per classifying stage, against the numpy models of the stages (dense_normals_model, dense_outliers_model, dense_carve_model), bit for bit.

The stage tests classify and remove in one breath.  Here the calls of different stages are interleaved on one object: a classification has to
outlive the other stage's call (both scans run through one scratch buffer), the grid has to be rebuilt when another edge is asked for or the
store has grown and reused otherwise, and a call refused for its config has to leave the earlier classification alone.

Stores of 65 and 257 rows from four origins: the totals cross a wave and a workgroup and are no multiple of 64, the smallest at which a misplaced
n + 1 word or a stale scan shows."""
import numpy as np
import pytest

import dense_carve_model as cm
import dense_normals_model as nm
import dense_outliers_model as om
import test_gpu_dense_carve as cg
import test_gpu_dense_cloud as base
import test_gpu_dense_normals as ng

pytestmark = pytest.mark.gpu

f32 = np.float32
VOXEL = cg.VOXEL
RADIUS, K, MUL = 0.3, 4, 1.0
CARVE = dict(cell_size=0.2, min_passes=1, **cg.LIVELY)
TOTALS = (65, 257)
_bits = ng._bits
_store = cg._store


@pytest.fixture(scope="module")
def opt():
    from dmsa_lidar_slam_amd.api import DmsaOptimizer

    o = DmsaOptimizer(device=0)
    yield o
    o.close()


def _cube(opt, total):
    """`total` rows, one per voxel of a cube two metres in front of four origins: the rays of one scan run through the rows of the others."""
    rng = np.random.default_rng(1000 + total)
    xyz = ng._one_per_voxel(rng, total, VOXEL, 8, corner=(2.0, -0.4, -0.3))
    dc, g, o = _store(opt, cg._split(rng, xyz, 4))
    assert g.shape[0] == total
    return dc, g, o


def _refused(call, text):
    from dmsa_lidar_slam_amd.api import DmsaError

    with pytest.raises(DmsaError) as e:
        call()
    assert e.value.status == -1 and text in e.value.args[0], e.value.args[0]


def _same_store(dc, g, o):
    g2, o2 = dc.retained()
    assert np.array_equal(_bits(g2), _bits(g)) and np.array_equal(_bits(o2), _bits(o)) and dc.retained_count() == g.shape[0]


# ---- 1. two masks side by side ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", TOTALS)
def test_the_outlier_mask_outlives_a_count_and_the_normals(opt, total):
    dc, g, o = _cube(opt, total)
    py, model = cg._cfg(**CARVE)
    flags, o_stats, _ = om.classify(g, RADIUS, K, MUL)
    passes, c_stats = cm.count_passes(g, o, model)
    got, got_flags = dc.classify_outliers(RADIUS, K, MUL, download=True)
    assert got == o_stats and np.array_equal(got_flags, flags)
    got, got_passes = dc.count_passes(py, download=True)  # its scan runs through the scratch the classification's ran through
    assert got == c_stats and np.array_equal(got_passes, passes)
    assert total < 257 or (0 < o_stats["inliers"] < total and 0 < c_stats["kept"] < total and o_stats["inliers"] != c_stats["kept"])
    dc.compute_normals(RADIUS, 5)
    keep = flags.astype(bool)
    assert dc.remove_outliers() == o_stats["inliers"] == int(keep.sum())
    _same_store(dc, g[keep], o[keep])
    _refused(dc.remove_transients, "no pass counts of the store as it stands")
    dc.close()


@pytest.mark.parametrize("total", TOTALS)
def test_the_carve_mask_outlives_a_classification(opt, total):
    dc, g, o = _cube(opt, total)
    py, model = cg._cfg(**CARVE)
    flags, o_stats, _ = om.classify(g, RADIUS, K, MUL)
    passes, c_stats = cm.count_passes(g, o, model)
    got, got_passes = dc.count_passes(py, download=True)
    assert got == c_stats and np.array_equal(got_passes, passes)
    got, got_flags = dc.classify_outliers(RADIUS, K, MUL, download=True)
    assert got == o_stats and np.array_equal(got_flags, flags)
    keep = passes < 1
    assert dc.remove_transients() == c_stats["kept"] == int(keep.sum())
    _same_store(dc, g[keep], o[keep])
    _refused(dc.remove_outliers, "no classification of the store as it stands")
    dc.close()


# ---- 2. the grid cache ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", TOTALS)
def test_the_grid_follows_the_edge_asked_for_and_the_store(opt, total):
    dc, g, o = _cube(opt, total)
    py, model = cg._cfg(**CARVE)
    want_m = nm.moments(g, RADIUS)
    first = dc.neighbour_moments(RADIUS)
    assert first.dtype == np.int64 and np.array_equal(first, want_m)
    assert np.array_equal(_bits(dc.knn_mean_distance(RADIUS, K)), _bits(om.knn_mean_distance(g, RADIUS, K)))  # the same edge: the grid as it is
    passes, c_stats = cm.count_passes(g, o, model)
    got, got_passes = dc.count_passes(py, download=True)  # another edge
    assert got == c_stats and np.array_equal(got_passes, passes)
    again = dc.neighbour_moments(RADIUS)  # ... and back
    assert again.tobytes() == first.tobytes()
    far = np.c_[np.full(40, 2.4), np.linspace(-0.35, 0.35, 40), np.linspace(-0.25, 0.45, 40)] + 0.013
    dc.add_scan((far - cg.ORIGINS[2]).astype(f32), np.linspace(base.S[4] + 0.01, base.S[5] - 0.01, 40))
    g2, o2 = dc.retained()
    assert g2.shape[0] > total and np.array_equal(_bits(g2[:total]), _bits(g))
    assert np.array_equal(_bits(dc.knn_mean_distance(RADIUS, K)), _bits(om.knn_mean_distance(g2, RADIUS, K)))  # the same edge, a grown store
    dc.close()


# ---- 3. a refused count leaves the earlier one --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", TOTALS)
def test_a_count_refused_for_its_config_leaves_the_earlier_counts_valid(opt, total):
    """T1 is checked before a count begins: the refused call has classified nothing and has not touched the classification there was."""
    from dmsa_lidar_slam_amd.dense_cloud import DenseCarveConfig

    dc, g, o = _cube(opt, total)
    py, model = cg._cfg(**CARVE)
    passes, c_stats = cm.count_passes(g, o, model)
    assert dc.count_passes(py) == c_stats
    _refused(lambda: dc.count_passes(DenseCarveConfig(cell_size=np.inf)), "cell_size is not finite")
    keep = passes < 1
    assert dc.remove_transients() == c_stats["kept"] == int(keep.sum())
    _same_store(dc, g[keep], o[keep])
    dc.close()
