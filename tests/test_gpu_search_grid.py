"""The keyframe search grid (sp_build_grid_device and its kernels in csrc/static_kernels.hip) on the cases of tests/search_grid_cases.py:
64-bit keys, both query kernels and their dispatch boundary, the 64-lane walk at every chunk edge, each of the 26 neighbour cells, the
grid margin, k = 1 .. 8 with ties, the exhaustive fallback, degenerate bounds.  tests/test_search_grid_cases.py proves that every case
takes the path it names and that the numpy model equals the oracle.  Everything here is flag and index work: exact equality only."""
import numpy as np
import pytest

import search_grid_cases as sg
from dmsa_lidar_slam_amd.api import DmsaError
from dmsa_lidar_slam_amd.keyframe_cloud import KeyframeCloudBuilder
from dmsa_lidar_slam_amd.static_points import StaticPointSelector

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def sel():
    s = StaticPointSelector(device=0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def kb():
    b = KeyframeCloudBuilder(device=0)
    yield b
    b.close()


def _same(got, ref):
    assert np.array_equal(got, ref, equal_nan=True), int(np.sum(np.any((got != ref) & ~(np.isnan(got) & np.isnan(ref)), axis=1)))


# ---- radius flags ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sg.RADIUS)
def test_radius_flags_equal_the_model(sel, name):
    c = sg.case(name)
    got = sel.radiusExists(c.cloud, c.query, c.r)
    ref = sg.model_flags(name)
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:10]


@pytest.mark.parametrize("name", sg.WIDE)
def test_wide_overlap_and_self_query(sel, orc, name):
    c = sg.case(name)
    got = sel.getOverlap(c.cloud, c.query, c.r)
    assert got == orc.get_overlap(c.cloud, c.query, c.r) and got[1] == int(sg.model_flags(name).sum())
    assert np.array_equal(sel.radiusExists(c.cloud, c.cloud, c.r), sg.finite_rows(c.cloud))  # every finite row finds itself


@pytest.mark.parametrize("name", ["wide64", "wide64_slab", "wide32_edge", "runs_64_last_end", "runs_65_first_marker", "runs_129_last_marker", "degenerate_identical"])
def test_both_query_kernels_at_the_dispatch_boundary(sel, name):
    """131072 queries go a wave per query, 131073 a thread per query (the cloud has fewer than four times as many rows)."""
    c = sg.case(name)
    n_wave = sg.WAVE_QUERY_LIMIT
    assert c.cloud.shape[0] < 4 * n_wave
    flags = sg.model_flags(name)
    by_wave = sel.radiusExists(c.cloud, sg.tiled(c.query, n_wave), c.r)
    by_thread = sel.radiusExists(c.cloud, sg.tiled(c.query, n_wave + 1), c.r)
    assert np.array_equal(by_wave, by_thread[:n_wave])
    assert np.array_equal(by_wave, sg.tiled(flags, n_wave)) and np.array_equal(by_thread, sg.tiled(flags, n_wave + 1))


@pytest.mark.parametrize("group", ["RUNS", "NEIGHBOUR", "REST"])
def test_thread_per_query_kernel_on_the_small_cases(sel, group):
    """The thread-per-query kernel has its own 27-cell loop and its own walk of a run: the same cases, one query past the boundary."""
    names = {"RUNS": sg.RUNS, "NEIGHBOUR": sg.NEIGHBOUR, "REST": ("margin", "deepest", "lattice_ties", "degenerate_planar_negzero", "few_finite_3", "wide64_band")}[group]
    count = sg.WAVE_QUERY_LIMIT + 1
    for name in names:
        c = sg.case(name)
        got = sel.radiusExists(c.cloud, sg.tiled(c.query, count), c.r)
        assert np.array_equal(got, sg.tiled(sg.model_flags(name), count)), name


# ---- normals and neighbour lists ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sg.K_VALUES)
@pytest.mark.parametrize("name", sg.KNN)
def test_neighbour_lists_and_normals(kb, orc, name, k):
    name = sg.knn_case_for(name, k)
    c = sg.case(name)
    if name == "wide64":  # the normals build their own grid from the cell hint: it, too, has more than 2^32 cells
        assert sg.grid_rule(c.cloud, c.r).cells > 2**32
    nrm, nn = kb.updateNormals(c.cloud, c.r, k=k, neighbours=True)
    assert nn.shape == (c.cloud.shape[0], k)
    model = sg.model_knn(name)[:, :k]
    assert np.array_equal(nn, model), np.flatnonzero((nn != model).any(axis=1))[:10]
    ref, ref_nn = orc.update_normals(c.cloud, k=k, neighbours=True)
    assert np.array_equal(nn, ref_nn)
    _same(nrm, ref)
    assert np.isnan(nrm[(nn >= 0).sum(axis=1) < 3]).all()  # fewer than three neighbours: no plane
    if k < 3:
        assert np.isnan(nrm).all()
    _same(kb.updateNormals(c.cloud, c.r, k=k), ref)  # without the lists


@pytest.mark.parametrize("k", [6, 8])
def test_cell_hint_does_not_matter(kb, k):
    c = sg.case("isolated_in_crowd")
    model = sg.model_knn(c.name)[:, :k]
    first = None
    for scale in (0.5, 1.0, 8.0):
        nrm, nn = kb.updateNormals(c.cloud, f32(scale) * c.r, k=k, neighbours=True)
        assert np.array_equal(nn, model), scale
        first = nrm if first is None else first
        _same(nrm, first)


# ---- errors and state ----------------------------------------------------------------------------------------------------------------------
def test_too_deep_is_refused_and_the_context_goes_on(sel, kb):
    deep, small, ok = sg.case("too_deep"), sg.case("runs_65_last_marker"), sg.case("deepest")
    with pytest.raises(DmsaError):
        sel.radiusExists(deep.cloud, deep.query, deep.r)
    with pytest.raises(DmsaError):
        sel.getOverlap(deep.cloud, deep.query, deep.r)
    assert np.array_equal(sel.radiusExists(small.cloud, small.query, small.r), sg.model_flags(small.name))
    with pytest.raises(DmsaError):
        kb.updateNormals(deep.cloud, deep.r, neighbours=True)
    few = sg.case("few_finite_5")
    assert np.array_equal(kb.updateNormals(few.cloud, few.r, k=8, neighbours=True)[1], sg.model_knn(few.name))
    # one cell less along the axis is the deepest grid the build accepts; its two rows are 2 M cells apart (exhaustive pass)
    assert np.array_equal(kb.updateNormals(ok.cloud, ok.r, k=8, neighbours=True)[1], sg.knn(ok.cloud, 8))


def test_key_width_is_state_of_the_build_not_of_the_buffers():
    """64-bit keys, then a 32-bit grid with fewer rows in the same buffers, then 64-bit keys again."""
    wide, small, edge = sg.case("wide64"), sg.case("runs_129_last_marker"), sg.case("wide32_edge")
    assert wide.rule.key64 and not small.rule.key64 and not edge.rule.key64 and small.cloud.shape[0] < wide.cloud.shape[0]
    s, b = StaticPointSelector(device=0), KeyframeCloudBuilder(device=0)
    try:
        flags = [s.radiusExists(c.cloud, c.query, c.r) for c in (wide, small, wide, edge, wide)]
        for got, c in zip(flags, (wide, small, wide, edge, wide)):
            assert np.array_equal(got, sg.model_flags(c.name)), c.name
        few = sg.case("few_finite_5")
        out = [b.updateNormals(c.cloud, c.r, k=6, neighbours=True) for c in (wide, few, wide)]
        for (nrm, nn), c in zip(out, (wide, few, wide)):
            assert np.array_equal(nn, sg.model_knn(c.name)[:, :6]), c.name
        _same(out[0][0], out[2][0])
    finally:
        s.close(), b.close()
