"""The rule of a floe frame's list sections (tests/record_lists_ref.py) held to the CPU oracle's list behind add_ghosts!, the partner
renumbering held to a hand-made case, the Python layout mirror, and the tables of julia/SubzeroHIP.jl that say which FloeOutputWriter outputs a
frame serves.  No GPU."""
import json
import os
import re

import numpy as np

import record_lists_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FLOES = 300


def test_the_rule_is_the_oracles_list_behind_add_ghosts():
    """the periodic 300-floe field of tests/test_record_gpu.py at steps 5 and 10: the oracle's list behind add_ghosts! is the list in front of it
    with an empty span on every ghost row -- and the field still has what the GPU tests need of it"""
    from subzero_jl_amd import fields
    from oracle import orc
    cfg = fields.make_config(n_floes=N_FLOES, seed=31, concentration=0.8)
    ow = fields.build_world(orc.World(), cfg)
    t = 0
    for s in (5, 10):
        for q in range(t, s):
            ow.timestep_sim(q, cfg["dt"], coupling_dt=1)
        t = s
        assert ow.M == N_FLOES
        off0, rows0 = ow.interactions()
        ow.add_ghosts()
        M = ow.M
        off1, rows1 = ow.interactions()
        want_off, want_rows = ref.inter_section(off0, rows0, N_FLOES, M)
        assert M > N_FLOES and np.array_equal(off1, want_off) and np.array_equal(rows1.view(np.uint64), want_rows.view(np.uint64))
        assert np.all(off1[N_FLOES:] == off1[N_FLOES])
        n = np.diff(off0)
        assert np.any(rows0[:, 0] > N_FLOES), "no partner that was a ghost of the step before"
        assert np.any(n == 0) and n.max() >= 2
        ow.remove_ghosts(N_FLOES)


def test_renumbering_and_sub_section_by_hand():
    N = 4
    keys = [(1 << 40) + 4 * 2 + 0, (2 << 40) + 4 * 0 + 1, (1 << 40) + 4 * 0 + 0]          # in allocation order
    rows = np.zeros((5, 7))
    rows[:, 0] = [2.0, float(keys[0] + 1), -3.0, float(keys[1] + 1), float((3 << 40) + 1)]          # the last: a key that is not among them
    rows[:, 1] = np.arange(5) + 0.5
    got = ref.renumbered(rows, keys, N)
    assert list(got[:, 0]) == [2.0, N + 2, -3.0, N + 3, float((3 << 40) + 1)]
    assert np.array_equal(got[:, 1:], rows[:, 1:])
    # two ghosts of parent 0, one of parent 2
    ghost_off = np.array([0, 2, 2, 3, 3, 3, 3, 3], np.int32); ghost_idx = np.array([4, 6, 5], np.int32)
    parent = ref.parents_of(ghost_off, ghost_idx, N, 7)
    assert list(parent) == [0, 1, 2, 3, 0, 2, 0]
    sub_off = np.array([0, 2, 2, 5, 6], np.int32); sx = np.arange(6.0); sy = -np.arange(6.0)
    so, x, y = ref.sub_section(sub_off, sx, sy, parent)
    assert list(so) == [0, 2, 2, 5, 6, 8, 11, 13]
    assert list(x) == [0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 0, 1] and np.array_equal(y, -x)
    io, ir = ref.inter_section(np.array([0, 1, 1, 3, 5, 9], np.int32), np.arange(63.0).reshape(9, 7), N, 7)
    assert list(io) == [0, 1, 1, 3, 5, 5, 5, 5] and ir.shape == (5, 7)


def test_frame_bytes_counts_the_lists():
    from subzero_jl_amd import capi
    from subzero_jl_amd.host import World
    assert capi.FRAME_LISTS == ["interactions", "subpoints"]
    mask = World.frame_mask(None)
    base = World.frame_bytes(mask, 11, 9, 70)
    assert World.frame_bytes(mask, 11, 9, 70, None) == World.frame_bytes(mask, 11, 9, 70, 0, 5, 6) == base
    assert World.frame_bytes(mask, 11, 9, 70, ["interactions"], 5, 6) == base + 48 + 5 * 56
    assert World.frame_bytes(mask, 11, 9, 70, ["subpoints"], 5, 6) == base + 48 + 6 * 16
    assert World.frame_bytes(mask, 11, 9, 70, 3, 5, 6) == base + 96 + 5 * 56 + 6 * 16
    assert World.frame_lists(["subpoints", "interactions"]) == 3 and World.frame_lists(None) == 0
    try:
        World.frame_lists(["fuse_idx"])
    except capi.SzError:
        pass
    else:
        raise AssertionError("an unknown list was taken")


def _symbols(text):
    return re.findall(r":([^\W\d]\w*)", text)


def test_julia_tables_cover_every_field_of_floe():
    from subzero_jl_amd import capi
    src = open(os.path.join(ROOT, "julia", "SubzeroHIP.jl")).read()
    fieldnames = json.load(open(os.path.join(ROOT, "tests", "golden", "floe_fieldnames.json")))["fieldnames"]
    assert len(fieldnames) == len(set(fieldnames)) == 39
    # FRAME_BITS / FRAME_OUTPUTS as they were
    bits = _symbols(re.search(r"^const FRAME_BITS = \((.*?)\)$", src, re.S | re.M).group(1))
    assert bits == capi.FRAME_BITS and len(bits) == 33
    outputs = re.search(r"^const FRAME_OUTPUTS = Dict\{Symbol, Vector\{Symbol\}\}\((.*?)\)$", src, re.S | re.M).group(1)
    plain = re.findall(r":(\w+) => \[", outputs)
    assert len(plain) == 30 and {g for lst in re.findall(r"=> \[(.*?)\]", outputs) for g in _symbols(lst)} <= set(bits)
    # the new tables
    lists = _symbols(re.search(r"^const FRAME_LISTS = \((.*?)\)$", src, re.M).group(1))
    assert lists == capi.FRAME_LISTS
    derived_src = re.search(r"^const FRAME_DERIVED_OUTPUTS = Dict\{Symbol, Tuple\{Vector\{Symbol\}, Vector\{Symbol\}\}\}\((.*?)\)$", src, re.S | re.M).group(1)
    derived = {}
    for name, groups, ls in re.findall(r":(\w+) => \((?:Symbol)?\[(.*?)\], (?:Symbol)?\[(.*?)\]\)", derived_src):
        derived[name] = (_symbols(groups), _symbols(ls))
    assert set(derived) == {"interactions", "num_inters", "status", "poly"}
    for name, (groups, ls) in derived.items():
        assert set(groups) <= set(bits) and set(ls) <= set(lists) and (groups or ls), name
    assert derived["interactions"] == ([], ["interactions"]) and derived["num_inters"] == ([], ["interactions"])
    assert derived["status"] == (["status"], []) and derived["poly"] == (["rings"], [])
    host = _symbols(re.search(r"^const FRAME_HOST_OUTPUTS = \((.*?)\)$", src, re.M).group(1))
    assert set(host) == {"angles", "damage", "parent_ids", "x_subfloe_points", "y_subfloe_points"}
    # device-served names are disjoint from host-served ones, and together they are the fields of Floe
    assert not set(plain) & set(derived) and not (set(plain) | set(derived)) & set(host)
    assert set(plain) | set(derived) | set(host) == set(fieldnames)
    assert re.search(r"^frame_covers\(w\) = all\(o -> haskey\(FRAME_OUTPUTS, o\) \|\| haskey\(FRAME_DERIVED_OUTPUTS, o\) \|\| o in FRAME_HOST_OUTPUTS, w\.outputs\)$", src, re.M)
    assert "sz_set_floe_output_lists" in src and "sz_download_floe_frame_interactions" in src and "sz_floe_frame_lists_info" in src
