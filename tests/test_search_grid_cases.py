"""CPU checks of tests/search_grid_cases.py: what makes the GPU cases of tests/test_gpu_search_grid.py non-vacuous.

Every fact a constructor claims is re-derived here -- key width, aliasing pair, run length and position, neighbour cell, margin band, tie
share, ring distance -- and the numpy model equals the oracle's exhaustive searches bit for bit on every case, so that from here on the
model and the oracle are two references that agree."""
import numpy as np
import pytest

import search_grid_cases as sg

F32 = np.float32


def _d(q, p):
    return sg.sq_dist(np.asarray(q, F32).reshape(1, -1), np.asarray(p, F32).reshape(-1, 4))[0]


# ---- the model against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["WIDE", "RUNS", "NEIGHBOUR", "REST"])
def test_radius_model_equals_the_oracles_exhaustive_search(orc, group):
    names = {"WIDE": sg.WIDE, "RUNS": sg.RUNS, "NEIGHBOUR": sg.NEIGHBOUR}.get(group) or [n for n in sg.RADIUS if n not in sg.WIDE + sg.RUNS + sg.NEIGHBOUR]
    for name in names:
        c = sg.case(name)
        assert np.array_equal(sg.model_flags(name), orc.radius_exists(c.cloud, c.query, c.r, brute=True)), name
        own = sg.radius_exists(c.cloud, c.cloud, c.r)
        assert np.array_equal(own, sg.finite_rows(c.cloud)), name  # every finite row finds itself, no other row finds anything


@pytest.mark.parametrize("name", sg.KNN)
def test_knn_model_equals_the_oracles_exhaustive_search(orc, name):
    c = sg.case(name)
    model = sg.model_knn(name)
    fin = sg.finite_rows(c.cloud)
    want = min(sg.K_MAX, int(fin.sum()))
    assert np.all(model[~fin] == -1) and np.all(model[fin][:, :want] >= 0) and np.all(model[fin][:, want:] == -1)
    for k in sg.K_VALUES:
        assert np.array_equal(orc.update_normals(c.cloud, k=k, neighbours=True)[1], model[:, :k]), k
        assert np.array_equal(sg.knn(c.cloud[:300], k), sg.knn(c.cloud[:300], sg.K_MAX)[:, :k])  # a shorter list is a prefix


# ---- wide grids: key width ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sg.WIDE)
def test_wide_cases_take_the_key_width_they_claim(name):
    c = sg.case(name)
    rule = c.rule
    assert rule.dims == c.facts["dims"] and not rule.too_deep
    if name == "wide32_edge":
        assert not rule.key64 and rule.cells > 0.999 * 2**31 and (rule.dims[0] + 1) ** 3 > 2**31  # one more cell per axis would not fit
    elif name == "wide64_band":
        assert rule.key64 and 2**31 < rule.cells < 2**32
    else:
        assert rule.key64 and rule.cells > 2**32
    fin = sg.finite_rows(c.cloud)
    codes = rule.code(c.cloud[fin])
    n = c.cloud.shape[0]
    assert c.cloud.shape[0] <= 6000 and not fin[:2].any() and not fin[-2:].any() and not fin[n // 2 - 4:n // 2 + 4].all()
    assert np.isnan(c.cloud[~fin][:, :3]).any() and np.isinf(c.cloud[~fin][:, :3]).any()
    if name in ("wide64", "wide64_slab"):
        assert (codes >= np.uint64(2**32)).sum() > 100 and (codes < np.uint64(2**32)).sum() > 100
    pair = sg.occupied_alias_pair(c)
    if name == "wide64":
        assert pair is not None and pair[0] != pair[1] and (pair[1] - pair[0]) % 2**32 == 0
        both = [c.cloud[fin][codes == np.uint64(p)] for p in pair]
        assert _d(both[0][0], both[1]).min() > 1e4 * c.r * c.r  # a 32-bit key would merge two cells that are far apart
        near = [(sg.sq_dist(c.query[sg.finite_rows(c.query)], b) <= c.r * c.r).any() for b in both]
        assert all(near), "queries hit rows of both aliased cells"
    if name == "wide64_slab":
        assert rule.dims[0] > 2**20 and (rule.cell_of(c.cloud[fin])[:, 0] > 2**20).sum() > 1000
    flags = sg.model_flags(name)
    assert 0.2 < flags.mean() < 0.8
    # tight clusters: most rows have their 8 nearest within two rings, the two pin rows are isolated
    nn = sg.knn(c.cloud, sg.K_MAX)
    rows = np.flatnonzero(fin)
    kth = sg.sq_dist(c.cloud[rows], c.cloud[rows])[np.arange(rows.shape[0]), np.searchsorted(rows, nn[rows, -1])]
    assert (kth < (0.999 * 2 * rule.cell) ** 2).mean() > 0.95
    assert (kth > (20 * rule.cell) ** 2).sum() >= 2


def test_too_deep_is_one_cell_past_the_deepest_grid(orc):
    deep, ok = sg.case("too_deep"), sg.case("deepest")
    assert deep.rule.too_deep and deep.rule.ext.max() >= 2097150.0
    assert not ok.rule.too_deep and ok.rule.dims == (1, 2097150, 1) and not ok.rule.key64
    with pytest.raises(RuntimeError):
        orc.radius_exists(deep.cloud, deep.query, deep.r)  # the oracle's grid refuses the same cloud
    assert np.array_equal(orc.radius_exists(ok.cloud, ok.query, ok.r), sg.model_flags("deepest"))
    assert sg.model_flags("deepest").tolist() == [True, True, False, False]


# ---- runs: the 64-lane walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sg.RUNS)
def test_runs_have_the_length_position_and_tail_they_claim(name):
    c = sg.case(name)
    m, near, tail, hit = c.facts["m"], c.facts["near"], c.facts["tail"], c.facts["hit"]
    rule = c.rule
    assert rule.dims == (3, 2, 3 if tail == "cell" else 2) and not rule.key64
    order, codes = sg.sorted_layout(c.cloud, rule)
    target = rule.code(hit[None])[0]
    run = np.flatnonzero(codes == target)
    assert run.shape[0] == m and np.array_equal(run, np.arange(run[0], run[0] + m))
    assert rule.cell_of(hit[None])[0].tolist() == [2, 1, 1]
    # the one near row is the last (first) of the run after the stable sort: lane (m - 1) % 64 of chunk (m - 1) // 64, or lane 0 of chunk 0
    at = m - 1 if near == "last" else 0
    assert np.array_equal(c.cloud[order[run[at]]], hit)
    n, nf = c.cloud.shape[0], int(sg.finite_rows(c.cloud).sum())
    end = run[-1] + 1
    if tail == "cell":
        assert end < nf == n and codes[end] != target
    elif tail == "end":
        assert end == n == nf
    else:
        assert end == nf < n and codes[end] == np.uint64(0xFFFFFFFFFFFFFFFF)
    # the query pair sits in the neighbouring cell; d(q_in) <= r^2 < d(q_out), one float apart; every other row of the run is beyond r
    q_in, q_out = c.query[0], c.query[1]
    r2 = c.r * c.r
    assert np.floor(rule.coord(c.query[:2])).tolist() == [[1, 1, 1], [1, 1, 1]]
    assert _d(q_in, hit[None])[0] <= r2 < _d(q_out, hit[None])[0] and q_out[0] == np.nextafter(q_in[0], F32(-np.inf))
    others = c.cloud[order[run]][np.arange(m) != at]
    assert _d(q_in, others).min() > r2 and _d(q_out, others).min() > r2
    assert _d(q_in, c.cloud[sg.finite_rows(c.cloud)]).argmin() == np.flatnonzero((c.cloud[sg.finite_rows(c.cloud)] == hit).all(axis=1))[0]
    assert sg.model_flags(name).tolist() == c.facts["expect"]


def test_run_lengths_straddle_the_chunks():
    assert sg.RUN_LENGTHS == (63, 64, 65, 127, 128, 129) and len(sg.RUNS) == 36


# ---- the 27 cells and the margin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", sg.OFFSETS)
def test_neighbour_cases_hit_through_one_cell_only(o):
    name = f"{o[0]}_{o[1]}_{o[2]}"
    inside, outside = sg.case("neighbour_in_" + name), sg.case("neighbour_out_" + name)
    for c in (inside, outside):
        rule = c.rule
        assert rule.dims == (3, 3, 3)
        cells = rule.cell_of(c.cloud)
        row = c.facts["row"]
        assert cells[row].tolist() == [1 + o[0], 1 + o[1], 1 + o[2]]
        assert np.floor(rule.coord(c.query)).tolist() == [[1, 1, 1]]
        d = _d(c.query[0], c.cloud)
        anchors = np.arange(9) != row
        assert (d[anchors] > c.r * c.r).all() and set(map(tuple, cells[anchors])) == {(x, y, z) for x in (0, 2) for y in (0, 2) for z in (0, 2)}
        assert (d[row] <= c.r * c.r) == c.facts["inside"]
        assert sg.model_flags(c.name).tolist() == [c.facts["inside"]]
    assert len(sg.OFFSETS) == 26 and np.array_equal(np.delete(inside.cloud, 4, 0), np.delete(outside.cloud, 4, 0))


def test_margin_queries_lie_in_their_bands():
    c = sg.case("margin")
    rule = c.rule
    n = c.facts["n_axis"]
    assert rule.dims == (n, n, n)
    band, facing = c.facts["band"], c.facts["facing"]
    v = rule.coord(c.query)
    out = np.maximum(-v, v - n).max(axis=1)  # cells outside the grid along the worst axis (below: -v; above: v - n)
    for b, (least, most) in enumerate(((0, 1), (1, 2), (2, np.inf))):
        rows = band == b
        assert rows.sum() >= 12 and ((out[rows] > least) & (out[rows] < most)).all()
    for a in range(3):  # every face has all three bands
        for below in (True, False):
            face = (-v[:, a] == out) if below else (v[:, a] - n == out)
            assert set(band[face]) == {0, 1, 2}, (a, below)
    # the gate of cell_of is -2 < v < n + 2: band 1 passes it and finds no cell, band 2 does not pass it
    assert (((v > -2) & (v < n + 2)).all(axis=1) == (band < 2)).all()
    assert (np.abs(c.query[:, :3]) >= F32(1e30)).any(axis=1).sum() == 8
    flags = sg.model_flags("margin")
    assert np.array_equal(flags, (band == 0) & facing) and flags.sum() == 6 + 8
    for b in (1, 2):  # necessarily false: the nearest row is more than a cell away whichever way the query faces
        rows = np.flatnonzero(band == b)
        assert sg.sq_dist(c.query[rows], c.cloud).min() > c.r * c.r


# ---- neighbour lists ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sg.K_VALUES)
def test_lattice_ties_are_decided_by_index(k):
    name = sg.knn_case_for("lattice_ties", k)
    c = sg.case(name)
    assert c.facts["k"] == (1 if k == 1 else 6)
    assert sg.kth_tie(c.cloud, k).mean() > 0.5
    fin = sg.finite_rows(c.cloud)
    pts = c.cloud[fin][:, :3]
    assert np.array_equal(pts * 4, np.round(pts * 4))  # exact quarter units: equal distances are equal floats
    order, _ = sg.sorted_layout(c.cloud, c.rule)
    spatial = np.lexsort((pts[:, 0], pts[:, 1], pts[:, 2]))
    assert not np.array_equal(order[: fin.sum()], np.flatnonzero(fin)) and not np.array_equal(spatial, np.arange(pts.shape[0]))
    flags = sg.model_flags(name)
    edge = np.abs(c.query[:, :3]).max(axis=1) == 1.0
    on_face = edge & ((np.abs(c.query[:, :3]) == 1.0).sum(axis=1) == 1)
    assert flags[~edge].all() and flags[on_face].all() and not flags[edge & ~on_face].any()  # d == r^2 exactly on the faces


def test_isolated_rows_pass_ring_six_and_the_crowd_does_not():
    c = sg.case("isolated_in_crowd")
    kind = c.facts["kind"]
    assert (kind == 0).sum() == 4000 and (kind == 1).sum() == 40 and (kind == 2).sum() == 12 and c.cloud.shape[0] <= 6000
    assert np.array_equal(kind == 2, ~sg.finite_rows(c.cloud))
    lone_at = np.flatnonzero(kind == 1)
    assert lone_at.min() < 500 and lone_at.max() > 3500 and np.flatnonzero(kind == 2).min() < 1500  # scattered through the index order
    fin = np.flatnonzero(kind < 2)
    for scale in (0.5, 1.0):
        rule = sg.grid_rule(c.cloud, F32(scale) * c.r)
        cells = rule.cell_of(c.cloud[fin])
        for i in np.flatnonzero(kind[fin] == 1):
            ring = np.abs(cells - cells[i]).max(axis=1)
            ring[i] = 1 << 30
            assert ring.min() > sg.K_MAX_RINGS + 1  # nothing within 7 rings: the walk reaches ring 7 and starts over exhaustively
    rule = c.rule
    nn = sg.model_knn("isolated_in_crowd")
    crowd = np.flatnonzero(kind == 0)
    kth = np.array([_d(c.cloud[i], c.cloud[nn[i, -1]][None])[0] for i in crowd[::7]])
    assert (kth < (0.999 * 2 * rule.cell) ** 2).all()  # k = 8 is complete within two rings
    flags = sg.model_flags("isolated_in_crowd")
    assert flags[:40].all() and not flags[40:80].any() and 0 < flags[80:].sum()


@pytest.mark.parametrize("f", sg.FEW)
def test_few_finite_rows(f):
    c = sg.case(f"few_finite_{f}")
    fin = sg.finite_rows(c.cloud)
    assert fin.sum() == f and (~fin).sum() == 20 and np.flatnonzero(fin).tolist() == c.facts["at"]
    nn = sg.model_knn(c.name)
    assert np.all(np.sort(nn[fin][:, :f], axis=1) == np.flatnonzero(fin)) and np.all(nn[fin][:, f:] == -1) and np.all(nn[fin][:, 0] == np.flatnonzero(fin))


@pytest.mark.parametrize("kind", sg.DEGENERATE)
def test_degenerate_bounds(kind):
    c = sg.case(f"degenerate_{kind}")
    rule = c.rule
    fin = sg.finite_rows(c.cloud)
    if kind == "identical":
        assert rule.dims == (1, 1, 1) and (rule.ext == 0).all() and c.cloud.shape[0] == 1000
        assert sg.model_flags(c.name).tolist() == c.facts["expect"]
        assert np.array_equal(sg.model_knn(c.name), np.tile(np.arange(8, dtype=np.int32), (1000, 1)))  # all ties: the first eight rows
        v = rule.coord(c.query)
        assert 1 < v[3, 2] < 2 and v[4, 0] < -2
        return
    assert rule.dims[2] == 1 and rule.dims[0] > 5 and rule.dims[1] > 5 and (c.cloud[fin][:, 2] == 0).all()
    neg = np.signbit(c.cloud[fin][:, 2])
    assert neg.sum() == (0 if kind == "planar" else neg.shape[0] // 2)
    plain = sg.case("degenerate_planar")
    assert np.array_equal(c.cloud[fin], plain.cloud[fin]) and np.array_equal(sg.model_flags(c.name), sg.model_flags(plain.name))
    flags = sg.model_flags(c.name).reshape(-1)
    assert flags[:400].all() and not flags[400:1200].any() and flags[1200:].all()


def test_tiled_queries_repeat_in_order():
    c = sg.case("runs_65_last_end")
    q = sg.tiled(c.query, 12)
    assert q.shape == (12, 4) and np.array_equal(q[5:10], c.query) and np.array_equal(sg.tiled(sg.model_flags(c.name), 12)[10:], sg.model_flags(c.name)[:2])


def test_constants_are_read_from_the_sources():
    assert sg.constants() == {"kMaxNeighbours": 8, "kMaxRings": 6, "wave_query_shift": 17}
    assert (sg.K_MAX, sg.K_MAX_RINGS, sg.WAVE_QUERY_LIMIT) == (8, 6, 131072) and max(sg.K_VALUES) == sg.K_MAX
