"""The narrow-phase edge cases (tests/narrow_edges_cases.py) on the CPU: the table's claims against the capacities parsed from the sources and
against the oracle's own clip, the exact reference's bound on the oracle's rows, and the retry count each GPU world has to show."""
import numpy as np
import pytest

import narrow_edges_cases as nec

ALL = list(nec.TABLE) + list(nec.RING_CLASSES)


@pytest.fixture(scope="module")
def caps():
    return nec.capacities()


def test_capacities_parse(caps):
    """the three instantiations and the two constants are found, ordered, and the first variant is the one the static_assert holds to 2 KB"""
    for v in nec.VARIANTS:
        assert set(caps[v]) == {"G", "CAP", "KC", "RC", "RM"} and all(isinstance(x, int) and x > 0 for x in caps[v].values()), (v, caps[v])
    for k in ("CAP", "KC", "RC", "RM", "G"):
        assert caps["first"][k] < caps["larger"][k] < caps["last"][k], k
    assert caps["last"]["CAP"] == 255 and caps["last"]["KC"] <= 64          # ring sizes and edge indices travel as bytes, crossing ranks in 6 bits
    assert caps["first"]["CAP"] <= caps["MV_RING"] <= caps["larger"]["CAP"] and caps["ROWS_PER_ITEM"] >= caps["last"]["RM"]
    assert caps["GHOST_FILL"] == 64 and caps["GHOST_FILL_WIDE"] == 128
    assert nec.first_variant_of("sz_k_narrow<8,18,8,16,4,64,0,0,3,0,0>") == dict(G=8, CAP=18, KC=8, RC=16, RM=4)


@pytest.mark.parametrize("name", list(nec.TABLE))
def test_table_rows_sit_on_their_edges(caps, name):
    """every at / past / in word of the table is an equality against the parsed capacities"""
    assert nec.edge_claims_hold(name, caps) == []


@pytest.mark.parametrize("name", ALL, ids=str)
def test_oracle_counts_are_the_tables(name):
    """ring points, K, R, P as the oracle's intersection_points and clip find them equal the construction's, with either polygon as ring a"""
    want = nec.counts(name)
    assert nec.oracle_counts(name) == want and nec.oracle_counts(name, swap=True) == want, (nec.oracle_counts(name), want)


def test_ring_classes_fall_where_the_table_says(caps):
    cls = {n: nec.ring_class(n, caps) for n in nec.RING_CLASSES}
    assert cls == {18: "first", 19: "larger", 20: "larger", 21: "larger", 32: "larger", 33: "last", 64: "last", 65: "last", 128: "last", 129: "last",
                   255: "last", 256: None}
    assert caps["MV_RING"] == 20                                             # 20 / 21 straddle the one-launch integrator's ring
    assert (caps["GHOST_FILL"], caps["GHOST_FILL_WIDE"]) == (64, 128)       # 64 / 65 and 128 / 129 straddle the ghost fill's two widths


@pytest.fixture(scope="module")
def oracle_world():
    """every case whose rows the oracle can form, on the lattice, both floe orders: one add_ghosts + timestep_collisions"""
    from oracle import orc
    names = [n for n in ALL if n != 256]
    place = nec.placements(names)
    w = nec.build_world(orc.World(), place)
    w.add_ghosts(); w.timestep_collisions(w.M, 10)
    return w, place


def test_oracle_rows_one_per_region(oracle_world):
    """each region of each pair gives one interaction row (so `last-R-at` fills ROWS_PER_ITEM exactly), and no pair but the lattice's"""
    w, place = oracle_world
    assert w.M == 2 * len(place)          # nothing straddles a wall: no ghosts
    i, j = w.pairs()
    assert sorted(zip(i.tolist(), j.tolist())) == [(2 * k, 2 * k + 1) for k in range(len(place))]
    off, rows = w.interactions()
    for k, (name, _, _, _) in enumerate(place):
        assert off[2 * k + 1] - off[2 * k] == off[2 * k + 2] - off[2 * k + 1] == nec.counts(name)[2], name
    assert nec.counts("last-R-at")[2] == nec.capacities()["ROWS_PER_ITEM"]


def test_oracle_is_inside_the_exact_bound(oracle_world):
    """the bound of exact_bound() is right: the oracle's overlap and contact-point columns stay inside it on every case at lattice offsets"""
    w, place = oracle_world
    worst = nec.assert_world_rows_exact(w, place, "oracle")
    assert 0.0 <= worst <= 1.0
    nec.assert_totals_are_row_sums(w, "oracle")


@pytest.mark.parametrize("comb_is_element", [True, False], ids=["comb-element", "bar-element"])
def test_oracle_element_rows(comb_is_element):
    """the element worlds of the GPU test: one row per region on the oracle, inside the exact bound, the floe stays active"""
    from oracle import orc
    for name in [n for n in nec.TABLE if not n.startswith("last")]:
        w = nec.build_element_world(orc.World(), name, comb_is_element)
        w.add_ghosts(); w.timestep_collisions(w.M, 10)
        assert nec.assert_rows_exact(w.inter(0), name, nec.ORIGIN[0], nec.ORIGIN[1], "oracle element item") <= 1.0
        assert w.ids()[2][0] == 1


def test_expected_retry_counts(caps):
    """the retry count of a world from the table: items of the first / larger ring class past a capacity of that class, per floe order"""
    per = {n: nec.expected_n_retry([n], caps, orders=1) for n in ALL}
    assert per == {**{n: 0 for n in ALL}, "first-K-past": 1, "first-P-past": 1, "larger-R-past": 1, "larger-K-past": 1}
    assert nec.outgrows("last-R-past", caps) == ("last", True) and nec.outgrows("last-K-past", caps) == ("last", True)
    assert nec.outgrows("last-K-at", caps) == ("last", False) and nec.outgrows(256, caps) == (None, True)
    assert nec.expected_n_retry(list(nec.TABLE), caps) == 8
