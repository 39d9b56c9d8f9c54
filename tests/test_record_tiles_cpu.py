"""The merge rule of tile floe frames (tests/record_tiles_ref.py; DESIGN.md §9i, "Tiled contexts") on the CPU oracle's list, and the mirror check
of the new entry points.  The oracle's list behind add_ghosts! on the 300-floe periodic field of tests/test_record_gpu.py is cut into tile
frames by random ownerships -- a ghost goes with its root parent, keys stand for positions as in tests/test_ridgeraft_tiles_cpu.py, a rank's
ghost rows are shuffled -- and the merged frames must give the list back, in every section."""
import os
import re

import numpy as np
import pytest

import record_tiles_ref as rec
import ridgeraft_tiles_ref as rt

pytestmark = pytest.mark.filterwarnings("ignore")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLES = ("cx", "cy", "u", "v", "height", "mass", "overarea")


@pytest.fixture(scope="module")
def oracle_list():
    from subzero_jl_amd import fields
    from oracle import orc
    cfg = fields.make_config(n_floes=300, seed=31, concentration=0.8)
    w = fields.build_world(orc.World(), cfg)
    w.add_ghosts()
    n, M = cfg["n_floes"], w.M
    assert M - n == 39, "the field's ghosts at step 0"
    ids, gids, status = w.ids()
    off, x, y = w.rings()
    frame = dict(tstep=0, M=M, N=n, id=ids, ghost_id=gids, status=status, vert_off=off.astype(np.int32), vx=x, vy=y)
    for name in DOUBLES:
        frame[name] = w.get(name)
    frame["strain"] = np.stack([w.get("e" + q) for q in ("11", "12", "21", "22")], 1)
    gl = w.ghosts()
    frame["ghost_off"] = np.concatenate([[0], np.cumsum([len(g) for g in gl])]).astype(np.int32)
    frame["ghost_idx"] = np.array([g for l in gl for g in l], np.int32)
    assert len(frame["ghost_idx"]) == M - n and max(len(g) for g in gl) == 3          # every ghost on one list; a corner floe with three
    key, root = rt.keys(w, n)
    return frame, key, root


@pytest.mark.parametrize("nranks", [1, 2, 4, 7])
def test_split_and_merge_give_the_list_back(oracle_list, nranks):
    frame, key, root = oracle_list
    n = frame["N"]
    rng = np.random.default_rng(100 + nranks)
    for trial in range(3):
        owner = rng.integers(0, nranks, n)
        if nranks > 2:
            owner[owner == nranks - 2] = 0          # an owner that holds no floe, in the middle of the ranks
        tiles = rec.split(frame, key, root, owner, nranks, rng)
        assert sum(t["M"] for t in tiles) == frame["M"] and (nranks <= 2 or tiles[nranks - 2]["M"] == 0)
        if nranks > 1:
            assert sum(1 for t in tiles if t["M"] > t["N"]) >= 2          # ghost rows on more than one rank
            assert any(not np.array_equal(t["key"][t["N"]:], np.sort(t["key"][t["N"]:])) for t in tiles)          # ... and out of order
        rec.assert_frames_equal(rec.merge(tiles), frame, (nranks, trial))


def test_merge_does_not_read_the_order_of_the_frames(oracle_list):
    frame, key, root = oracle_list
    rng = np.random.default_rng(7)
    tiles = rec.split(frame, key, root, rng.integers(0, 3, frame["N"]), 3, rng)
    rec.assert_frames_equal(rec.merge(tiles[::-1]), frame, "frames in reverse rank order")


def test_tiled_recorder_entry_points_mirror_header_and_capi():
    from subzero_jl_amd import capi, tiles
    hdr = open(os.path.join(ROOT, "include", "subzero_hip.h")).read()
    L = capi.load()
    for fn, nargs, like in (("sz_tile_set_floe_output", 5, "sz_set_floe_output"), ("sz_tile_set_grid_output", 10, "sz_set_grid_output"), ("sz_tile_floe_frame_keys", 4, None),
                            ("sz_tile_floe_frame_info", 8, "sz_floe_frame_info"), ("sz_tile_download_floe_frame", 4, "sz_download_floe_frame")):
        d = re.search(rf"\nint {fn}\(([^;]*?)\);", hdr)
        assert d and d.group(1).count(",") + 1 == nargs, fn
        assert fn in capi.EXPORTS and len(getattr(L, fn).argtypes) == nargs, fn
        if like:
            assert list(getattr(L, fn).argtypes) == list(getattr(L, like).argtypes), fn
            same = lambda s: re.sub(r"\s+", " ", re.search(rf"\nint {s}\(([^;]*?)\);", hdr).group(1))
            assert same(fn) == same(like), fn
    assert L.sz_tile_floe_frame_keys.argtypes[3] is capi._lp
    for name in ("set_floe_output", "set_grid_output", "output_frames", "clear_frames", "floe_frame_local", "floe_frame", "grid_frame"):
        assert callable(getattr(tiles.TiledWorld, name)), name
