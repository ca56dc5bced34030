"""CPU checks of tests/lattice_cases.py: what makes the GPU cases of tests/test_gpu_lattice_hint.py non-vacuous.

The model of the sequential box agrees with the pointer tree (tests/pcl_octree_model.py) and with the oracle; every base cloud has the events
it was built for, at both resolutions; every hold case leaves both histories alone; every reject case changes the history it aims at; and
every constructed float lies where its case says."""
import numpy as np
import pytest

import lattice_cases as lc
from pcl_octree_model import PclOctree

C = lc.constants()
BLOCK = C["kAabbBlock"]
VARIANTS = ["plain", "near_origin", "leading_nan", "many_blocks_12", "many_blocks_13"]


_base = lc.base_by_variant


def _xyz4(xyz):
    return np.concatenate([xyz, np.ones((xyz.shape[0], 1), np.float32)], axis=1)


def test_constants_are_read_from_the_sources():
    assert C == {"kAabbBlock": 1024, "kHintBlocks": 12, "kLatticeLdsBlocks": 2048, "kMaxLatticeEvents": 64}, C


@pytest.mark.parametrize("variant", VARIANTS)
def test_box_history_agrees_with_the_pointer_tree(variant):
    base = _base(variant)
    for level in (0, 1):
        h = base.hist(level)
        tree, trig = PclOctree(base.res[level]), []
        first = -1
        for i, p in enumerate(base.xyz):
            if not np.isfinite(p).all():
                continue
            before = tree.events
            tree._adopt(p)
            trig += [i] * (tree.events - before)
            first = i if first < 0 else first
        assert (first, trig) == (h.first, h.triggers.tolist())
        assert tree.mn == h.mn[-1].tolist() and tree.mx == h.mx[-1].tolist() and tree.depth == h.depth[-1]
        assert tree.events == h.num_events


@pytest.mark.parametrize("variant", VARIANTS + ["big"])
def test_box_history_agrees_with_the_oracle(orc, variant):
    base = lc.big_cloud() if variant == "big" else _base(variant)
    for level in (0, 1):
        h = base.hist(level)
        info, code, key, order = orc.voxelize(_xyz4(base.xyz), base.res[level])
        assert (info.depth, info.num_events, list(info.min_xyz)) == (h.depth[-1], h.num_events, h.mn[-1].tolist())
        ok = h.epoch >= 0
        assert info.num_valid == ok.sum()
        assert np.array_equal(key[ok], h.keys(base.xyz)[ok])


@pytest.mark.parametrize("variant", ["plain", "near_origin", "leading_nan"])
@pytest.mark.parametrize("level", [0, 1])
def test_base_clouds_hold_the_events_they_were_built_for(variant, level):
    base = _base(variant)
    h = base.hist(level)
    assert base.xyz.shape[0] == 14 * BLOCK + 37
    trig = h.triggers
    blocks = trig // BLOCK
    fb = h.first // BLOCK
    assert set(trig.tolist()) == set(base.outliers)                                    # every outlier is a trigger at this level, nothing else is
    assert len(set(trig[blocks == fb].tolist())) >= 2                                  # two events in the first point's block
    assert any(len(set(trig[blocks == b].tolist())) >= 2 for b in set(blocks.tolist()) - {fb})  # two different triggers in one later block
    assert max(np.bincount(trig)) >= 3                                                 # the same trigger three times or more
    assert any(t % BLOCK == BLOCK - 1 and t + 1 in trig for t in trig.tolist())        # triggers at k * 1024 - 1 and k * 1024
    grew_down = h.shift != 0
    up_and_down = [e for e in range(h.num_events) if not grew_down[e, 0] and base.xyz[trig[e], 1] < h.mn[e][1]]
    assert up_and_down, "no event that is above the box on x while below it on y"
    assert len(h.special_blocks(BLOCK)) <= C["kHintBlocks"] and h.num_events <= C["kMaxLatticeEvents"]
    assert len(base.free_blocks(BLOCK)) >= 3
    if variant == "leading_nan":
        assert h.first == BLOCK + 5 and not np.isfinite(base.xyz[:h.first]).any()
    if variant == "near_origin":
        assert np.abs(h.mn[0]).max() < 1.0 and np.abs(h.mx[0]).max() < 1.0
        assert grew_down[0, 0] and trig[0] // BLOCK == 0                               # an early event grows downward on x ...
        x_up = [int(trig[e]) for e in range(h.num_events) if not grew_down[e, 0]]
        assert min(x_up) // BLOCK > base.free_blocks(BLOCK)[0]                          # ... and none upward before the block R3 uses


@pytest.mark.parametrize("k", [12, 13])
def test_many_blocks_have_k_special_blocks(k):
    base = _base(f"many_blocks_{k}")
    for level in (0, 1):
        assert len(base.hist(level).special_blocks(BLOCK)) == k
    same, held = zip(*lc.expectation(base, base))
    assert same == (True, True) and held == ((True, True) if k <= C["kHintBlocks"] else (False, False))


@pytest.mark.parametrize("case,level", [(c, l) for c, l in lc.case_ids() if c in lc.HOLD_CASES])
def test_hold_cases_leave_the_histories_alone(case, level):
    base = lc.base_of(case)
    t, notes = lc.tamper(base, case, level)
    h = base.hist(level)
    assert h.same_as(t.hist(level)), (case, level)
    if (case.startswith("H3") or case == "H8_on_min") and level == 1:  # level 0's boxes lie inside level 1's: the faces of level 1 are outside them, level 0 must replay
        assert all((base.hist(0).mn[-1] >= base.hist(1).mn[-1]).tolist()) and not base.hist(0).same_as(t.hist(0))
    else:
        assert base.hist(1 - level).same_as(t.hist(1 - level)), (case, level)
    if case != "H1" and case != "H6":
        assert t.xyz.tobytes() != base.xyz.tobytes()
    if case.startswith("H3"):  # every face, in a block without triggers and around the triggers of a special block; the next float is outside
        for where in ("free", "before", "between", "behind"):
            assert len(notes[where]) >= 3, (where, notes[where])
            for i, a, s, e in notes[where]:
                assert e == h.epoch[i] and i not in base.outliers
                q = t.xyz[i].copy()
                assert lc._inside(h, e, q)
                q[a] = np.nextafter(q[a], np.float32(np.inf if s == "hi" else -np.inf))
                assert not lc._inside(h, e, q)
        for where in ("free", "before", "between", "behind"):  # every face in the block without triggers AND at each place of the special block
            assert [(a, s) for _, a, s, _ in notes[where]] == lc._FACES, where
        assert notes["free"][0][0] // BLOCK in base.free_blocks(BLOCK) and notes["before"][0][0] // BLOCK in h.special_blocks(BLOCK)
        e_before, e_between, e_behind = (notes[w][0][3] for w in ("before", "between", "behind"))
        assert e_before < e_between < e_behind
    if case == "H2":
        moved = (t.xyz != base.xyz).any(axis=1)
        assert moved.sum() > 14000 and not moved[list(base.outliers)].any() and np.abs(t.xyz.astype(np.float64) - base.xyz).max() < 1e-3
    if case == "H4":
        b = notes["block"]
        assert not np.isfinite(t.xyz[b * BLOCK:(b + 1) * BLOCK]).any() and np.isfinite(t.xyz[list(base.outliers)]).all()
        assert (~np.isfinite(t.xyz).all(axis=1)).sum() == BLOCK + 4
        lone = lc._lone_inf(t.xyz)[0]  # an infinity beside two finite coordinates, in a block without triggers and in a special block
        assert np.flatnonzero(lone).tolist() == sorted(notes["lone_inf"])
        prob, tab = lc.problem(t), lc.pose_tables()
        for i in notes["lone_inf"]:  # what the transform computes for them, in its order of operations: the prescribed floats
            r, p = tab[prob.tformIdPerPoint[i]].reshape(3, 4), prob.localPoints[i]
            with np.errstate(over="ignore"):
                g = np.array([((r[k, 0] * p[0] + r[k, 1] * p[1]) + r[k, 2] * p[2]) + r[k, 3] for k in range(3)], np.float32)
            assert np.isfinite(p[:3]).all() and g.tobytes() == t.xyz[i].tobytes()
    if case == "H5":
        assert notes["trigger"] in base.outliers and t.xyz[notes["trigger"]].tobytes() != base.xyz[notes["trigger"]].tobytes()
    if case == "H8_on_min":
        i = notes["moved"]
        assert h.epoch[i] == 0 and float(t.xyz[i, 0]) == h.mn[0][0] and i // BLOCK == h.first // BLOCK
    if case.startswith("H7_"):
        i, tr = notes["copy"], notes["trigger"]
        assert i == tr + 1 and t.xyz[i].tobytes() == base.xyz[tr].tobytes()
        assert h.events_of(tr).size >= (3 if case == "H7_behind_repeated" else 1)


@pytest.mark.parametrize("case,level", [(c, l) for c, l in lc.case_ids() if c in lc.REJECT_CASES])
def test_reject_cases_change_the_history_they_aim_at(case, level):
    base = lc.base_of(case)
    t, notes = lc.tamper(base, case, level)
    h, ht = base.hist(level), t.hist(level)
    if case == "R11":  # the identical cloud: the history holds, the table is beyond what the verification takes
        assert h.same_as(ht) and lc.expectation(base, t) == [(True, False), (True, False)]
        return
    assert not h.same_as(ht), (case, level)
    assert lc.expectation(base, t)[level] == (False, False)
    if case not in ("R10_shorter", "R10_longer", "R12"):  # one change each
        assert (t.xyz.view(np.uint32) != base.xyz.view(np.uint32)).any(axis=1).sum() == 1
    if case == "R0_on_max":
        i = notes["moved"]
        assert h.epoch[i] == 0 and float(t.xyz[i, 0]) == h.mx[0][0] and i in ht.triggers
    if case.startswith("R1_"):  # one float step outside the box of its epoch, in a block without triggers
        (i, a, s, e), = notes["moved"]
        assert (i // BLOCK) in base.free_blocks(BLOCK) and e == h.epoch[i] and ("xyz"[a], s) == (case[3], case[5:])
        q = t.xyz[i].copy()
        assert not lc._inside(h, e, q)
        q[a] = np.nextafter(q[a], np.float32(-np.inf if s == "hi" else np.inf))
        assert lc._inside(h, e, q)
        assert i in ht.triggers
    if case.startswith("R2_"):  # inside the box behind the trigger's events, outside the one in front of them, and in front of the trigger
        i, tr = notes["copy"], notes["trigger"]
        ev = h.events_of(tr)
        assert i < tr and h.epoch[i] == ev[0] and not lc._inside(h, ev[0], t.xyz[i]) and lc._inside(h, ev[-1] + 1, t.xyz[i])
        if case == "R2_free_block":
            sp = h.special_blocks(BLOCK)
            assert i // BLOCK not in sp and i // BLOCK - 1 in sp and i // BLOCK + 1 in sp and tr // BLOCK == i // BLOCK + 1
        else:
            assert i == tr - 1 and i // BLOCK == tr // BLOCK
            assert ev.size >= (3 if case == "R2_own_block_repeated" else 1)
        assert i in ht.triggers and tr not in ht.triggers
    if case.startswith("R3_"):  # fitted the first box, does not fit the box grown downward: a float in [mx_e, mx_0)
        i = notes["moved"]
        e = int(h.epoch[i])
        x = float(t.xyz[i, 0])
        assert e >= 1 and (h.shift[:e, 0] != 0).all()  # every event so far grew downward on x
        assert h.mx[e][0] <= x < h.mx[0][0] and lc._inside(h, 0, t.xyz[i]) and not lc._inside(h, e, t.xyz[i])
        assert (i // BLOCK in h.special_blocks(BLOCK)) == (case != "R3_later_block") and i not in base.outliers
        rd0 = lc.below(h.mx[0][0]) if float(np.float32(h.mx[0][0])) != h.mx[0][0] else np.float32(h.mx[0][0])  # box 0's maximum rounded inward
        if case == "R3_special_block":
            assert t.xyz[i, 0] == rd0
        if case == "R3_special_block_second":  # passes a float test against the first box alone, and still fails every later box of its block
            last = int(h.epoch[(i // BLOCK + 1) * BLOCK - 1])
            assert t.xyz[i, 0] < rd0 and last > e and all(x >= h.mx[k][0] for k in range(1, last + 1))
    if case == "R4":
        assert h.events_of(notes["trigger"]).size > 0 and ht.events_of(notes["trigger"]).size == 0 and np.isfinite(t.xyz[notes["trigger"]]).all()
    if case == "R5":
        tr = notes["trigger"]
        e0, e1 = h.events_of(tr)[0], ht.events_of(tr)[0]
        assert h.shift[e0, 0] == 0 and ht.shift[e1, 0] != 0  # x: at or above the maximum before, below the minimum now
    if case in ("R6_more", "R6_fewer"):
        tr = notes["trigger"]
        assert h.events_of(tr).size >= 3 and ht.events_of(tr).size == h.events_of(tr).size + (1 if case == "R6_more" else -1)
    if case == "R7":
        assert not np.isfinite(t.xyz[notes["trigger"]]).any() and ht.events_of(notes["trigger"]).size == 0
    if case.startswith("R8_"):
        i = notes["moved"]
        assert i < h.first and ht.first == i and not np.isfinite(base.xyz[i]).any()
        assert (i // BLOCK == h.first // BLOCK) == (case == "R8_own_block")
    if case == "R9":
        assert ht.first == h.first and ht.mn[0].tobytes() != h.mn[0].tobytes()
    if case == "R10_shorter":
        assert t.xyz.shape[0] <= h.triggers[-1] and np.array_equal(t.xyz, base.xyz[:t.xyz.shape[0]])
    if case == "R10_longer":
        n0 = base.xyz.shape[0]
        assert t.xyz.shape[0] == n0 + BLOCK and np.array_equal(t.xyz[:n0], base.xyz) and notes["moved"] // BLOCK > (n0 - 1) // BLOCK
        assert ht.triggers[-1] == notes["moved"] and np.array_equal(ht.triggers[:h.num_events], h.triggers)
    if case == "R12":
        assert t.xyz.tobytes() == base.xyz.tobytes() and t.res != base.res


def test_the_cloud_beyond_the_lds_table():
    base = lc.big_cloud()
    n = base.xyz.shape[0]
    assert n == (C["kLatticeLdsBlocks"] + 1) * BLOCK + 5
    t, notes = lc.tamper_big(base, 0)
    i = notes["moved"]
    assert i // BLOCK == C["kLatticeLdsBlocks"]
    for level in (0, 1):
        h = base.hist(level)
        late = h.triggers[h.triggers >= BLOCK]
        assert set(late.tolist()) == set(base.outliers) and len(h.special_blocks(BLOCK)) <= C["kHintBlocks"]
    h = base.hist(0)
    e = int(h.epoch[i])
    assert e == h.num_events and i // BLOCK not in h.special_blocks(BLOCK)
    q = t.xyz[i].copy()
    assert not lc._inside(h, e, q)
    q[1] = np.nextafter(q[1], np.float32(-np.inf))
    assert lc._inside(h, e, q)
    assert lc.expectation(base, base) == [(True, True), (True, True)]
    assert lc.expectation(base, t)[0] == (False, False)
