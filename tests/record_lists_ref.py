"""The rule of a floe frame's list sections (csrc/sz_record.hpp, "THE LISTS") in numpy: what the interactions and the sub-floe
points of the list behind add_ghosts! are, made from the list in front of it.  tests/test_record_lists_cpu.py holds the rule to the CPU oracle,
tests/test_record_lists_gpu.py the recorded frames to the rule."""
import numpy as np

GHOST_KEY_LIMIT = float(1 << 40)          # a floeidx above this is 1 + the order key of an inline ghost of the last step


def parents_of(ghost_off, ghost_idx, N, M):
    """the parent row of every row of a list with ghosts, from the parents' ghost links (a parent row: itself)"""
    parent = np.arange(M)
    parent[N:] = -1
    for i in range(N):
        parent[ghost_idx[ghost_off[i]:ghost_off[i + 1]]] = i
    return parent


def renumbered(rows, ghost_keys, N):
    """floe.interactions as the reference stores it: a partner that was a ghost of the last step is N + the rank of its order key among that
    step's ghost keys + 1; a key that is not among them, and every other partner, stays"""
    rows = np.array(rows, np.float64).reshape(-1, 7)
    keys = np.sort(np.asarray(ghost_keys, np.int64))
    for r in np.nonzero(rows[:, 0] > GHOST_KEY_LIMIT)[0]:
        key = int(rows[r, 0]) - 1
        k = int(np.searchsorted(keys, key))
        if k < len(keys) and keys[k] == key:
            rows[r, 0] = float(N + k + 1)
    return rows


def inter_section(off, rows, N, M):
    """(inter_off [M + 1], inter_rows): the parents' rows as the list in front of add_ghosts! holds them, an empty span on every ghost row
    (deepcopy_floe passes no interactions: zeros(0, 7), num_inters = 0)"""
    out = np.empty(M + 1, np.int32)
    out[:N + 1] = off[:N + 1]
    out[N:] = off[N]
    return out, np.array(rows[:off[N]], np.float64).reshape(-1, 7)


def sub_section(sub_off, sx, sy, parent):
    """(sub_off [M + 1], sx, sy) of the list whose rows have the parents `parent`: a parent row's own points, a ghost row its parent's"""
    n = np.diff(np.asarray(sub_off, np.int64))[parent]
    out = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    take = np.concatenate([np.arange(sub_off[p], sub_off[p + 1]) for p in parent]) if len(parent) else np.zeros(0, np.int64)
    take = take.astype(np.int64)
    return out, np.asarray(sx)[take], np.asarray(sy)[take]
