"""tests/ridgeraft_rows_ref.py pinned on hand-made lists (it is what tests/test_pending_splice_gpu.py holds sz_ridgeraft_rows to), and the six
new entry points in the header, the ctypes binding and the Julia binding.  No device is needed."""
import numpy as np

import ridgeraft_rows_ref as rrr


def _list(n_ghosts):
    """parents 0..n-1 with ids 101.., parent p followed -- behind all parents, in parent order -- by n_ghosts[p] ghosts that carry its id"""
    n = len(n_ghosts)
    ids = [101 + p for p in range(n)]
    lists = []
    for p, k in enumerate(n_ghosts):
        lists.append(list(range(len(ids), len(ids) + k)))
        ids += [101 + p] * k
    m = len(ids)
    off = np.zeros(m + 1, np.int64)
    off[1:n + 1] = np.cumsum(n_ghosts)
    off[n + 1:] = off[n]
    return np.array(ids, np.int64), n, off, np.array([g for l in lists for g in l], np.int64), lists


# parents 0..5: 0 has one ghost (6), 1 none, 2 two (7, 8), 3 three -- a corner floe of a doubly periodic domain -- (9, 10, 11), 4 none, 5 one (12)
IDS, N, OFF, IDX, LISTS = _list([1, 0, 2, 3, 0, 1])


def _closure(table):
    return rrr.closure(IDS, N, OFF, IDX, table).tolist()


def test_the_hand_made_list_is_what_it_says():
    assert LISTS == [[6], [], [7, 8], [9, 10, 11], [], [12]] and len(IDS) == 13
    assert [rrr.root_parent(IDS, N, r) for r in range(13)] == [0, 1, 2, 3, 4, 5, 0, 2, 2, 3, 3, 3, 5]


def test_a_parent_brings_its_one_two_or_three_ghosts():
    assert _closure([(0, 2)]) == [0, 1, 6]                   # j = 2 names row 1, which has no ghost
    assert _closure([(1, 3)]) == [1, 2, 7, 8]
    assert _closure([(1, 4)]) == [1, 3, 9, 10, 11]            # the corner floe: all three


def test_an_entry_whose_i_is_a_ghost_brings_the_parent_and_its_other_ghosts():
    assert _closure([(7, 13)]) == [2, 5, 7, 8, 12]            # i = ghost 7 of parent 2; j = 13 names row 12, the ghost of parent 5
    assert _closure([(10, -1)]) == [3, 9, 10, 11]             # the middle ghost of the corner floe against the north boundary


def test_an_entry_whose_j_is_a_ghost():
    assert _closure([(1, 7)]) == [0, 1, 6]                    # j = 7 names row 6, the ghost of parent 0
    assert _closure([(4, 12)]) == [3, 4, 9, 10, 11]


def test_boundary_and_topography_partners_bring_only_the_family_of_i():
    for j in (-1, -2, -3, -4, -5, -17):
        assert _closure([(4, j)]) == [4]
        assert _closure([(2, j)]) == [2, 7, 8]
        assert _closure([(12, j)]) == [5, 12]


def test_one_floe_in_many_entries_comes_once_and_the_result_ascends():
    table = [(5, 2), (1, 3), (1, 4), (1, 7), (1, -3), (0, 2), (6, 2), (1, 2)]
    got = _closure(table)
    assert got == sorted(set(got)) == [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12]
    assert _closure(table[::-1]) == got


def test_an_empty_table_gives_no_row():
    got = rrr.closure(IDS, N, OFF, IDX, [])
    assert got.dtype == np.int32 and got.shape == (0,)


def test_take_list_selects_rows_of_all_four_csr_lists():
    m = len(IDS)
    cols = {"id": IDS, "cx": np.arange(m) * 1.5, "stress_accum": np.arange(4.0 * m).reshape(m, 4),
            "vert_off": np.arange(m + 1, dtype=np.int32) * 4, "vx": np.arange(4.0 * m), "vy": -np.arange(4.0 * m),
            "sub_off": np.concatenate([np.arange(N + 1) * 2, np.full(m - N, 2 * N)]).astype(np.int32), "sx": np.arange(2.0 * N), "sy": np.arange(2.0 * N) + 0.5,
            "inter_off": np.concatenate([[0], np.cumsum(np.arange(m) % 3)]).astype(np.int32), "ghost_off": OFF.astype(np.int32), "ghost_idx": IDX.astype(np.int32)}
    cols["inter_rows"] = np.arange(7.0 * cols["inter_off"][-1]).reshape(-1, 7)
    got = rrr.take_list(cols, [10, 3, 0])
    assert got["id"].tolist() == [104, 104, 101] and got["stress_accum"].shape == (3, 4) and got["stress_accum"][1, 0] == 12.0
    assert got["vert_off"].tolist() == [0, 4, 8, 12] and got["vx"].tolist() == [40, 41, 42, 43, 12, 13, 14, 15, 0, 1, 2, 3]
    assert got["sub_off"].tolist() == [0, 0, 2, 4] and got["sy"].tolist() == [6.5, 7.5, 0.5, 1.5]          # (a ghost row has no points)
    assert got["ghost_off"].tolist() == [0, 0, 3, 4] and got["ghost_idx"].tolist() == [9, 10, 11, 6]
    assert got["inter_off"].tolist() == [0, 1, 1, 1] and got["inter_rows"].shape == (1, 7)
    assert got["inter_rows"][0, 0] == 7.0 * cols["inter_off"][10]


def test_pending_splice_entry_points_mirror_header_capi_and_julia():
    """every new entry point is declared in the header, exported by the ctypes binding with the header's argument count, and bound in Julia"""
    import os
    import re

    import subzero_jl_amd
    from subzero_jl_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "subzero_hip.h")).read()
    jl = open(os.path.join(root, "julia", "SubzeroHIP.jl")).read()
    L = capi.load()
    for fn, nargs in (("sz_ridgeraft_rows", 4), ("sz_download_list_rows", 7), ("sz_splice_parents", 9), ("sz_ridgeraft_rows_f32", 4),
                      ("sz_download_list_rows_f32", 7), ("sz_splice_parents_f32", 9)):
        d = re.search(rf"\nint {fn}\(([^;]*)\);", hdr)
        assert d and d.group(1).count(",") + 1 == nargs, fn
        assert fn in capi.EXPORTS, fn
        assert len(getattr(L, fn).argtypes) == nargs, fn
        assert re.search(rf"@ccall lib\.{fn}\(", jl), fn
    for name in ("function ridgeraft_rows", "function download_list_rows!", "function splice_parents!"):
        assert name in jl, name
    W = subzero_jl_amd.World
    assert W.ridgeraft_rows and W.download_list_rows and W.splice_parents
