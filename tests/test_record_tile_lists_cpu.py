"""The rule of the list sections of tile floe frames (tests/record_tile_lists_ref.py; DESIGN.md §9i, "Tiled contexts", the lists) on the CPU
oracle's data, and the mirror checks of the new entry points.  No GPU.

The source is the oracle's list behind add_ghosts! on the periodic 300-floe field of tests/test_record_gpu.py at the output steps 5 and 10, with
the oracle's interactions from in front of add_ghosts! and its sub-floe points.  The ghost list of the step before -- what the partner numbers
above N count in -- is the oracle's too: add_ghosts! on the state that step began with.  Keys stand for positions as in
tests/test_ridgeraft_tiles_cpu.py.  The list is cut by random ownerships, merged back, and must come back equal in every section to
record_lists_ref.inter_section / sub_section / renumbered of the uncut list -- and to the oracle's own list behind add_ghosts!."""
import os
import re

import numpy as np
import pytest

import record_lists_ref as lref
import record_tile_lists_ref as tl
import record_tiles_ref as rec
import ridgeraft_tiles_ref as rt

pytestmark = pytest.mark.filterwarnings("ignore")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FLOES = 300
DOUBLES = ("cx", "cy", "u", "v", "height", "mass")


@pytest.fixture(scope="module")
def oracle_lists():
    """per output step: the uncut frame with lists (partner column untranslated), its keys and roots, the last step's ghost keys and roots, and
    what the merged frame must be"""
    from subzero_jl_amd import fields
    from oracle import orc
    cfg = fields.make_config(n_floes=N_FLOES, seed=31, concentration=0.8)
    ow = fields.build_world(orc.World(), cfg)
    N, t, out = N_FLOES, 0, []
    for s in (5, 10):
        for q in range(t, s - 1):
            ow.timestep_sim(q, cfg["dt"], coupling_dt=1)
        # the ghost list step s - 1 runs on: add_ghosts! on the state it begins with
        ow.add_ghosts()
        last_key, last_root = rt.keys(ow, N)
        last_key, last_root = last_key[N:].copy(), last_root[N:].copy()
        ow.remove_ghosts(N)
        ow.timestep_sim(s - 1, cfg["dt"], coupling_dt=1)
        t = s
        off0, rows0 = ow.interactions()
        off0, rows0 = off0.copy(), rows0.reshape(-1, 7).copy()
        assert ow.M == N and rows0[:, 0].max() <= N + len(last_key)
        raw = rows0.copy()          # the partner column as a tile holds it: key + 1
        was_ghost = raw[:, 0] > N
        raw[was_ghost, 0] = (last_key[raw[was_ghost, 0].astype(np.int64) - N - 1] + 1).astype(np.float64)
        ow.add_ghosts()
        M = ow.M
        off1, rows1 = ow.interactions()
        key, root = rt.keys(ow, N)
        ids, gids, status = ow.ids()
        voff, x, y = ow.rings()
        frame = dict(tstep=s, M=M, N=N, id=ids, ghost_id=gids, status=status, vert_off=voff.astype(np.int32), vx=x, vy=y)
        for name in DOUBLES:
            frame[name] = ow.get(name)
        gl = ow.ghosts()
        frame["ghost_off"] = np.concatenate([[0], np.cumsum([len(g) for g in gl])]).astype(np.int32)
        frame["ghost_idx"] = np.array([g for l in gl for g in l], np.int32)
        want = dict(frame)
        want["inter_off"], want["inter_rows"] = lref.inter_section(off0, lref.renumbered(raw, last_key, N), N, M)
        want["sub_off"], want["sx"], want["sy"] = lref.sub_section(cfg["sub_off"], cfg["sx"], cfg["sy"], root)
        # ... which is the oracle's own list behind add_ghosts!
        assert np.array_equal(want["inter_off"], off1) and rec.same(want["inter_rows"], rows1.reshape(-1, 7)[:off1[M]])
        frame["inter_off"], frame["inter_rows"] = lref.inter_section(off0, raw, N, M)
        frame["sub_off"], frame["sx"], frame["sy"] = want["sub_off"], want["sx"], want["sy"]
        ow.remove_ghosts(N)
        out.append(dict(frame=frame, want=want, key=key, root=root, last_key=last_key, last_root=last_root, off0=off0, rows0=rows0))
    return out


def test_the_field_exercises_the_paths(oracle_lists):
    for d in oracle_lists:
        off0, rows0, fr = d["off0"], d["rows0"], d["frame"]
        assert np.any(rows0[:, 0] > N_FLOES), "no partner that was a ghost"
        assert np.any(np.diff(off0[:N_FLOES + 1]) == 0), "no parent without rows"
        assert np.any(fr["inter_rows"][:, 0] > tl.LIMIT) and np.any(rows0[:, 0] < 0) == np.any(fr["inter_rows"][:, 0] < 0)
        assert fr["M"] > fr["N"] and np.all(np.diff(fr["sub_off"])[fr["N"]:] > 0), "ghost rows without points"
        # the two steps' ghost keys overlap without meaning the same ghosts: the merge must read the table, not the frame's keys
        assert len(np.intersect1d(d["key"][N_FLOES:], d["last_key"])) > 0


def _cross_owner_ghost_partner(d, owner):
    """a row whose partner was a ghost of a parent that another rank owns than the row's floe"""
    off0, rows0 = d["off0"], d["rows0"]
    floe = np.repeat(np.arange(N_FLOES), np.diff(off0[:N_FLOES + 1]))
    g = rows0[:, 0] > N_FLOES
    parent = d["last_root"][rows0[g, 0].astype(np.int64) - N_FLOES - 1]
    return bool(np.any(owner[parent] != owner[floe[g]]))


@pytest.mark.parametrize("nranks", [1, 2, 4, 7])
def test_cut_and_merge_give_the_list_back(oracle_lists, nranks):
    rng = np.random.default_rng(300 + nranks)
    crossed = False
    for step, d in enumerate(oracle_lists):
        for trial in range(2):
            owner = rng.integers(0, nranks, N_FLOES)
            if nranks > 2:
                owner[owner == nranks - 2] = 0          # an owner that holds no floe, in the middle of the ranks
            tiles = tl.cut(d["frame"], d["last_key"], owner, d["key"], d["root"], d["last_root"], nranks, rng)
            assert sum(t["M"] for t in tiles) == d["frame"]["M"] and (nranks <= 2 or tiles[nranks - 2]["M"] == 0)
            assert sum(len(t["inter_rows"]) for t in tiles) == len(d["frame"]["inter_rows"])
            if nranks > 1:
                assert any(not np.array_equal(t["key"][t["N"]:], np.sort(t["key"][t["N"]:])) for t in tiles)          # ghost rows out of order
                assert any(np.any(t["lkeys"] < tl.GHOST) for t in tiles)          # halo parents' keys in a table
                table = np.concatenate([t["lkeys"] for t in tiles])
                assert len(np.unique(table)) < len(table)          # a ghost key in more than one table
                crossed = crossed or _cross_owner_ghost_partner(d, owner)
            got = tl.merge(tiles)
            rec.assert_frames_equal(got, d["want"], (nranks, step, trial))
            rec.assert_frames_equal(tl.merge(tiles[::-1]), d["want"], (nranks, step, trial, "frames in reverse rank order"))
    assert crossed or nranks == 1, "no ghost partner whose parent has another owner than the row's floe"


def test_a_key_found_nowhere_stays_and_unpadded_tables_do():
    """by hand: two ranks, three parents, the last step's ghosts 0 (of parent 2) and 1 (of parent 0); parent 1's row names a key no table holds"""
    k0, k1, lost = tl.GHOST + 4 * 2, (2 << 40) + 4 * 0 + 1, (3 << 40) + 5
    t0 = dict(tstep=3, M=2, N=2, key=np.array([0, 2], np.int64), cx=np.array([1.0, 3.0]),
              inter_off=np.array([0, 2, 2], np.int32), inter_rows=np.array([[k0 + 1.0] + [0.5] * 6, [-2.0] + [1.5] * 6]),
              sub_off=np.array([0, 1, 3], np.int32), sx=np.array([10.0, 30.0, 31.0]), sy=np.array([-10.0, -30.0, -31.0]), lkeys=np.array([k0, k1], np.int64))
    t1 = dict(tstep=3, M=2, N=1, key=np.array([1, tl.GHOST + 4 * 1], np.int64), cx=np.array([2.0, 2.5]),
              inter_off=np.array([0, 3, 3], np.int32), inter_rows=np.array([[k1 + 1.0] + [2.5] * 6, [lost + 1.0] + [3.5] * 6, [3.0] + [4.5] * 6]),
              sub_off=np.array([0, 2, 4], np.int32), sx=np.array([20.0, 21.0, 20.0, 21.0]), sy=np.zeros(4), lkeys=np.array([1, k0, k0], np.int64))
    got = tl.merge([t0, t1])
    assert got["M"] == 4 and got["N"] == 3 and list(got["cx"]) == [1.0, 2.0, 3.0, 2.5]
    assert list(got["inter_off"]) == [0, 2, 5, 5, 5]
    assert list(got["inter_rows"][:, 0]) == [3 + 1, -2.0, 3 + 2, lost + 1.0, 3.0] and list(got["inter_rows"][:, 1]) == [0.5, 1.5, 2.5, 3.5, 4.5]
    assert list(got["sub_off"]) == [0, 1, 3, 5, 7] and list(got["sx"]) == [10.0, 20.0, 21.0, 30.0, 31.0, 20.0, 21.0]


def test_tile_frame_bytes_counts_the_lists():
    from subzero_jl_amd.host import World
    from subzero_jl_amd.tiles import TiledWorld
    mask = World.frame_mask(None)
    plain = World.frame_bytes(mask, 11, 9, 70) + 8 * 11
    assert TiledWorld.tile_frame_bytes(mask, 11, 9, 70) == TiledWorld.tile_frame_bytes(mask, 11, 9, 70, 0, 5, 6, 4) == plain
    assert TiledWorld.tile_frame_bytes(mask, 11, 9, 70, ["interactions"], 5, 6, 4) == plain + 8 * 4 + 48 + 5 * 56
    assert TiledWorld.tile_frame_bytes(mask, 11, 9, 70, ["subpoints"], 5, 6, 4) == plain + 48 + 6 * 16
    assert TiledWorld.tile_frame_bytes(mask, 11, 9, 70, 3, 5, 6, 4) == plain + 8 * 4 + 96 + 5 * 56 + 6 * 16


def test_tile_list_entry_points_mirror_header_and_capi():
    from subzero_jl_amd import capi, tiles
    hdr = open(os.path.join(ROOT, "include", "subzero_hip.h")).read()
    L = capi.load()
    for fn, nargs, like in (("sz_tile_set_floe_output_lists", 3, "sz_set_floe_output_lists"), ("sz_tile_floe_frame_lists_info", 6, None),
                            ("sz_tile_download_floe_frame_interactions", 5, "sz_download_floe_frame_interactions"), ("sz_tile_floe_frame_list_keys", 5, None)):
        d = re.search(rf"\nint {fn}\(([^;]*?)\);", hdr)
        assert d and d.group(1).count(",") + 1 == nargs, fn
        assert fn in capi.EXPORTS and hasattr(L, fn) and len(getattr(L, fn).argtypes) == nargs, fn
        if like:
            assert list(getattr(L, fn).argtypes) == list(getattr(L, like).argtypes), fn
            same = lambda s: re.sub(r"\s+", " ", re.search(rf"\nint {s}\(([^;]*?)\);", hdr).group(1))
            assert same(fn) == same(like), fn
    for name in ("set_floe_output_lists", "tile_frame_bytes", "frame_list_keys", "floe_frame_lists_info"):
        assert callable(getattr(tiles.TiledWorld, name)), name
