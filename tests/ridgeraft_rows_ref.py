"""The closure rule of sz_ridgeraft_rows, restated with numpy on a full download: which list rows the host's
timestep_ridging_rafting! can touch, given the candidate table.  Nothing here touches the device; tests/test_ridgeraft_rows_cpu.py pins it on
hand-made lists and tests/test_pending_splice_gpu.py holds the device to it.

A list is described by what a full download gives: `ids` (one per list row, parents first, a ghost carries its parent's id), `n` (the number
of parents), the ghost lists as CSR (`ghost_off` with one entry per list row + 1, `ghost_idx` in list numbers; a ghost row's list is empty),
and the table as (i, j) pairs -- i a 0-based list row, j as the interaction rows name the partner: a 1-based list row, -1..-4 for a boundary,
-(4 + k) for topography element k.

Also here: `take_list`, the rows of a full download of the whole list as a list of their own (the layout of World.download_list_rows)."""
import numpy as np

CSR = (("vert_off", ("vx", "vy")), ("sub_off", ("sx", "sy")), ("inter_off", ("inter_rows",)), ("ghost_off", ("ghost_idx",)))
CSR_NAMES = {n for off, vals in CSR for n in (off,) + vals}


def root_parent(ids, n, row):
    """the reference's findfirst(x -> x == floes.id[row], floes.id): the first row with that id, which is a parent"""
    p = int(np.nonzero(np.asarray(ids) == ids[row])[0][0])
    assert p < n, "a ghost without a parent among the first n rows"
    return p


def family(ids, n, ghost_off, ghost_idx, row):
    """the row, its root parent and every ghost on that parent's list"""
    p = root_parent(ids, n, row)
    return {int(row), p} | {int(g) for g in ghost_idx[ghost_off[p]:ghost_off[p + 1]]}


def closure(ids, n, ghost_off, ghost_idx, table):
    """ascending 0-based list rows, each once: for every entry (i, j) the family of row i and, where j > 0, of row j - 1"""
    rows = set()
    for i, j in table:
        rows |= family(ids, n, ghost_off, ghost_idx, int(i))
        if j > 0:
            rows |= family(ids, n, ghost_off, ghost_idx, int(j) - 1)
    return np.array(sorted(rows), np.int32)


def closure_of_world(w, table):
    """closure() on what World w downloads: ids(), N, ghosts()"""
    ids = w.ids()[0]
    gl = w.ghosts()
    off = np.concatenate([[0], np.cumsum([len(g) for g in gl])]).astype(np.int64)
    idx = np.array([g for l in gl for g in l], np.int64)
    return closure(ids, w.N, off, idx, table)


def take_list(cols, idx):
    """the list rows idx of a full download `cols` (every column with one entry per list row, the four CSR lists with one offset per list row
    + 1), in the order asked, as a list of their own with offsets from 0"""
    idx = np.asarray(idx, np.int64)
    out = {k: np.array(v[idx]) for k, v in cols.items() if k not in CSR_NAMES}
    for off, vals in CSR:
        o = np.asarray(cols[off], np.int64)
        cnt = o[idx + 1] - o[idx]
        out[off] = np.concatenate([[0], np.cumsum(cnt)]).astype(cols[off].dtype)
        sel = np.concatenate([np.arange(o[i], o[i + 1]) for i in idx] + [np.zeros(0, np.int64)]).astype(np.int64)
        for v in vals:
            out[v] = np.array(cols[v][sel])
    return out
