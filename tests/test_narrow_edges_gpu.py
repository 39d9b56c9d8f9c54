"""The narrow phase's three kernel variants at the edges of their LDS working sets (tests/narrow_edges_cases.py has the generator, the case
table and the two references; tests/test_narrow_edges_cpu.py holds the table and the exact reference's bound to the oracle).  Every world is a
lattice of comb-against-bar pairs, each case in both floe orders.  An item AT a capacity must be answered by the variant it starts in, an item
one step PAST it must be flagged, emit nothing, add nothing to the totals and be redone by the last variant (stats()["n_retry"] counts exactly
those), and an item past the LAST variant must end the call in an error.  An item that was wrongly kept shows as rows that differ from both
references (a dropped closing point, a missing region), one that was wrongly handed on as a retry count that is off.
Needs a real MI355X: run with -m gpu."""
import os
import re

import numpy as np
import pytest

import narrow_edges_cases as nec
import parity
from test_hip_parity import _ab_worlds, _assert_worlds_bit_equal, mk, omk

pytestmark = pytest.mark.gpu

FIRST = [n for n in nec.TABLE if n.startswith("first")]
LARGER = [n for n in nec.TABLE if n.startswith("larger")]
LAST_OK = ["last-R-at", "last-K-at"]
TOTALS = ["coll_fx", "coll_fy", "coll_trq", "overarea"]


@pytest.fixture(scope="module")
def caps():
    return nec.capacities()


def _process(w):
    n = w.M
    w.add_ghosts(); w.timestep_collisions(n, 10)
    return w


def _oracle_steps(ow, n):
    for k in range(n):
        ow.timestep_sim(k, 10, coupling_dt=10, coupling_on=False)
    return ow


def _env_world(env, build):
    for k, v in env.items():
        os.environ[k] = v
    try:
        return build(mk())
    finally:
        for k in env:
            del os.environ[k]


def test_first_variant_is_the_parsed_one(caps):
    """the capacities the table is held to are the ones of the kernel that runs"""
    assert nec.first_variant_of(mk().narrow_kernel_name()) == caps["first"]


def test_process_mode_at_and_past_every_capacity(caps):
    """a. add_ghosts + timestep_collisions on a fresh context, all three variants' at / past rows that the last variant can answer (40 floes):
    pairs bit-exact, rows and totals to the oracle at 1e-10, overlap and contact point to the exact reference, n_retry from the table, every
    floe's totals the sums of its own rows"""
    names = FIRST + LARGER + LAST_OK
    place = nec.placements(names)
    hw = _process(nec.build_world(mk(), place)); ow = _process(nec.build_world(omk(), place))
    assert hw.M == ow.M == 2 * len(place)
    assert parity.compare_pairs(hw, ow) == len(place)
    parity.compare_interactions(hw, ow, rtol=1e-10)
    parity.compare_worlds(hw, ow, rtol=1e-10, fields=TOTALS, check_inter=False)
    print("worst error / exact bound:", nec.assert_world_rows_exact(hw, place, "hip"))
    nec.assert_totals_are_row_sums(hw, "hip")
    off, _ = hw.interactions()
    k = [n for n, _, _, _ in place].index("last-R-at")
    assert off[2 * k + 1] - off[2 * k] == caps["ROWS_PER_ITEM"]                 # 16 regions, 16 rows: the row stride is full
    assert hw.stats()["n_retry"] == nec.expected_n_retry(names, caps) == 8, hw.stats()["n_retry"]


@pytest.mark.parametrize("group", ["first", "larger"])
def test_process_mode_retries_only_what_is_past(caps, group):
    """a, by variant: a world of the at-capacity and inside rows alone is not retried at all, the world of the past rows once per item"""
    rows = FIRST if group == "first" else LARGER
    for names in ([n for n in rows if not nec.TABLE[n]["over"]], [n for n in rows if nec.TABLE[n]["over"]]):
        place = nec.placements(names)
        hw = _process(nec.build_world(mk(), place)); ow = _process(nec.build_world(omk(), place))
        parity.compare_pairs(hw, ow)
        parity.compare_interactions(hw, ow, rtol=1e-10)
        nec.assert_world_rows_exact(hw, place, "hip")
        nec.assert_totals_are_row_sums(hw, "hip")
        assert hw.stats()["n_retry"] == nec.expected_n_retry(names, caps) == (4 if nec.TABLE[names[0]]["over"] else 0), (names, hw.stats()["n_retry"])


@pytest.mark.parametrize("comb_is_element", [True, False], ids=["comb-element", "bar-element"])
def test_element_items_at_and_past_every_capacity(caps, comb_is_element):
    """b. open boundaries, the comb as a topography element against a bar floe and a bar-shaped element against a comb floe: the first and
    the larger variant's rows, one context per row (an element table holds one kind of ring)"""
    for name in FIRST + LARGER:
        hw = _process(nec.build_element_world(mk(), name, comb_is_element)); ow = _process(nec.build_element_world(omk(), name, comb_is_element))
        parity.compare_interactions(hw, ow, rtol=1e-10)
        parity.compare_worlds(hw, ow, rtol=1e-10, fields=TOTALS, check_pairs=False, check_inter=False)
        nec.assert_rows_exact(hw.inter(0), name, nec.ORIGIN[0], nec.ORIGIN[1], "hip element item")
        nec.assert_totals_are_row_sums(hw, "hip")
        assert hw.stats()["n_retry"] == nec.expected_n_retry([name], caps, orders=1), (name, hw.stats()["n_retry"])


def test_resident_three_launch_steps(caps):
    """c. five resident steps of the three-launch kind with the contacts held (no coupling, a soft E): the state to the oracle at 1e-9, the
    guards' counts equal, and SZ_LEAN_NARROW=1 (the last variant enters after a pause and a restart of the step) bit-equal to =0"""
    names = FIRST + LARGER + LAST_OK
    place = nec.placements(names)
    build = lambda w: nec.build_world(w, place, E=1e3)
    ow = _oracle_steps(build(omk()), 5)
    runs = []
    for lean in ("1", "0"):
        hw = _env_world({"SZ_PIPELINE": "0", "SZ_LEAN_NARROW": lean}, build)
        assert hw.run(5, 0, 10, coupling_dt=10, coupling_on=False, stop_on_tags=False) == 5 and not hw.pipelined()
        assert hw.stats()["n_retry"] >= nec.expected_n_retry(names, caps)          # (every step retries them again)
        runs.append(hw)
    parity.compare_worlds(runs[0], ow, rtol=1e-9, check_pairs=False)
    assert np.array_equal(runs[0].warn_counts(), ow.warn_counts())
    for f in parity.SCALARS:
        assert np.array_equal(runs[0].get(f), runs[1].get(f)), f
    assert np.array_equal(runs[0].rings()[1], runs[1].rings()[1])
    a, b = runs[0].interactions(), runs[1].interactions()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("names", [["first-all-at", "first-inside"], FIRST], ids=["at-capacity", "past-from-step-0"])
def test_pipelined_steps(caps, names):
    """d. rings of at most 18 points, two batches of pipelined steps against the three-launch steps bit for bit and against the oracle at
    1e-9; the second world holds its over-capacity pairs from step 0 on: the pause comes in the first step of a pipelined batch"""
    place = nec.placements(names)
    build = lambda w: nec.stir(nec.build_world(w, place, E=1e3))
    a, b = _ab_worlds(build, {"SZ_PIPELINE": "0"})
    ow = build(omk())
    t = 0
    for n in (4, 5):
        da = a.run(n, t, 10, coupling_dt=10, coupling_on=False, stop_on_tags=False)
        db = b.run(n, t, 10, coupling_dt=10, coupling_on=False, stop_on_tags=False)
        assert da == db == n and a.pipelined() and not b.pipelined()
        _assert_worlds_bit_equal(a, b)
        for k in range(t, t + n):
            ow.timestep_sim(k, 10, coupling_dt=10, coupling_on=False)
        parity.compare_worlds(a, ow, rtol=1e-9, check_pairs=False)
        t += n
    want = nec.expected_n_retry(names, caps)
    assert (a.stats()["n_retry"] >= want) and (a.stats()["n_retry"] > 0) == (want > 0), a.stats()["n_retry"]


def _ring_world(w, points, periodic, E=None):
    """both floe orders of `tttt` padded to `points`; periodic: the pairs lie across the west wall, so both floes of a pair get ghosts"""
    place = [(points, order, (-3000 if periodic else nec.ORIGIN[0]), 20457 + 40000 * k) for k, order in enumerate(("comb-first", "bar-first"))]
    w = nec.build_world(w, place, kinds=(1, 1, 1, 1) if periodic else (0, 0, 0, 0), E=E, ext=(0.0, 1.0e5, 0.0, 1.0e5))
    return (nec.stir(w) if E is not None else w), place


@pytest.mark.parametrize("periodic", [False, True], ids=["open", "periodic-wall"])
@pytest.mark.parametrize("points", nec.RING_CLASSES)
def test_ring_classes(caps, points, periodic):
    """e. one world per ring size (which launches a context uses is decided by its LARGEST ring: 18 / 19 the first variant, 20 / 21 the
    one-launch integrator and the inline ghosts, 32 / 33 the larger variant, 64 / 65 and 128 / 129 the ghost passes' one and two points per
    lane, 255 / 256 the byte a ring size travels in), process mode and a 5-step resident batch, away from the walls and across a periodic one.
    Up to 255 points (128 where a ghost has to be made: the refusal is pinned here) the oracle's answer; beyond, an error that names the limit."""
    limit = caps["last"]["CAP"] if not periodic or points > caps["last"]["CAP"] else caps["GHOST_FILL_WIDE"]
    if points > limit:
        hw, _ = _ring_world(mk(), points, periodic)
        with pytest.raises(Exception) as e:
            hw.add_ghosts()
        assert type(e.value).__name__ == "SzError" and f"{points} points" in str(e.value) and str(limit) in str(e.value), str(e.value)
        assert ("periodic" in str(e.value)) == (points <= caps["last"]["CAP"])
        return
    (hw, place), (ow, _) = _ring_world(mk(), points, periodic), _ring_world(omk(), points, periodic)
    _process(hw); _process(ow)
    assert hw.M == ow.M == (8 if periodic else 4) and hw.ghosts() == ow.ghosts()
    assert parity.compare_pairs(hw, ow) >= 2
    parity.compare_interactions(hw, ow, rtol=1e-10)
    parity.compare_worlds(hw, ow, rtol=1e-10, fields=TOTALS, check_inter=False)
    if not periodic:
        nec.assert_world_rows_exact(hw, place, "hip")
    assert hw.stats()["n_retry"] == 0
    (hw, _), (ow, _) = _ring_world(mk(), points, periodic, E=1e3), _ring_world(omk(), points, periodic, E=1e3)
    assert hw.run(5, 0, 10, coupling_dt=10, coupling_on=False, stop_on_tags=False) == 5
    _oracle_steps(ow, 5)
    parity.compare_worlds(hw, ow, rtol=1e-9, check_pairs=False)
    assert np.array_equal(hw.warn_counts(), ow.warn_counts())
    assert len(hw.interactions()[1]) >= 16                      # the contacts are still there


@pytest.mark.parametrize("name,bit", [("last-R-past", 4), ("last-K-past", 2)])
def test_past_the_last_variant_is_an_error(caps, name, bit):
    """f. 17 regions / 66 crossings: the call raises a capacity error whose message carries exactly the bit of what was outgrown, beside the
    legend that names it (regions = 4, crossings = 2: the crossing test comes first, so 66 crossings never reach the region count), and the
    rows of every OTHER pair of the world -- a retried one among them -- are the oracle's all the same"""
    names = ["first-all-at", name, "larger-R-at", "first-K-past"]
    place = nec.placements(names)
    hw = nec.build_world(mk(), place); ow = _process(nec.build_world(omk(), place))
    hw.add_ghosts()
    with pytest.raises(Exception) as e:
        hw.timestep_collisions(hw.M, 10)
    msg = str(e.value)
    assert type(e.value).__name__ == "SzError" and "capacity" in msg and ("regions=4" if bit == 4 else "crossings=2") in msg, msg
    assert int(re.search(r"bits 0x([0-9a-f]+)", msg).group(1), 16) == bit, msg
    hoff, hrows = hw.interactions(); ooff, orows = ow.interactions()
    fl = parity.force_floors(orows, np.max(ow.get("rmax")))
    for k, (nm, _, _, _) in enumerate(place):
        if nm == name:
            continue
        for i in (2 * k, 2 * k + 1):
            h, o = hrows[hoff[i]:hoff[i + 1]], orows[ooff[i]:ooff[i + 1]]
            assert h.shape == o.shape and np.array_equal(h[:, 0], o[:, 0]), (nm, i)
            for c, floor in ((1, fl["force"]), (2, fl["force"]), (3, 1e-10 * fl["Lc"]), (4, 1e-10 * fl["Lc"]), (5, fl["torque"]), (6, fl["area"])):
                parity.assert_elementwise(f"{nm} floe {i} column {c}", h[:, c], o[:, c], 1e-10, floor)
