"""A rank's share of one global row edit (csrc/sz_splice_tile.hpp; sz_tile_splice_floes) restated in numpy.  The edit -- (delete, replace, append)
as tests/splice_ref.py's `apply` takes it, in GLOBAL numbers -- is the same on every rank; `share` says what one rank does with it: which of its
local rows it deletes and replaces, which of the staged floes (the replacements, then the appended ones) it takes, and the global numbers its rows
carry afterwards.  `verdict` is the agreement in front of the change.  tests/test_splice_tiles_cpu.py holds both to splice_ref.apply over the
undivided list: the ranks' results, put in the order of their new numbers, are that list."""
import numpy as np

import splice_ref as sp

E_ARG, E_CAPACITY, E_STATE = -2, -3, -4


def n_staged(edit):
    delete, replace, append = edit
    n_rep = len(replace[0]) if replace is not None else 0
    n_app = sp.n_rows(append) if append is not None else 0
    return n_rep, n_app


def argument_fault(edit, owner, nranks):
    """what the arguments alone decide, the same on every rank: None or the reason"""
    delete, replace, append = edit
    dele = [int(d) for d in delete]
    rep = [int(r) for r in replace[0]] if replace is not None else []
    n_rep, n_app = n_staged(edit)
    for what, names in (("del", dele), ("rep", rep)):
        if any(g < 0 for g in names):
            return what + " negative"
        if any(b == a for a, b in zip(names, names[1:])):
            return what + " repeats"
        if any(b < a for a, b in zip(names, names[1:])):
            return what + " not ascending"
    if set(dele) & set(rep):
        return "both deleted and replaced"
    if n_app and (owner is None or len(owner) != n_app):
        return "app_owner missing"
    if n_app and any(o < 0 or o >= nranks for o in owner):
        return "app_owner out of range"
    for floes in ([replace[1]] if replace is not None else []) + ([append] if append is not None else []):
        o = floes["vert_off"]
        for j in range(sp.n_rows(floes)):
            nv = o[j + 1] - o[j]
            if nv < 4 or floes["vx"][o[j]] != floes["vx"][o[j + 1] - 1] or floes["vy"][o[j]] != floes["vy"][o[j + 1] - 1]:
                return "open ring"
            if nv > 255:
                return "ring over 255 points"
    return None


def share(gidx_of_rank, edit, owner, rank, n_global):
    """one rank's share: dict(del_rows, rep_rows -- ascending LOCAL rows --, staged -- positions among the n_rep + n_app staged floes, ascending:
    the replacements whose row this rank owns, the appended floes it is the owner of --, found_del, found_rep, taken, gidx -- the new global
    numbers of its rows in their new order: the kept rows, each its old number minus the deleted names below it, then the appended floes it
    takes, floe k as n_global - n_del + k)"""
    delete, replace, append = edit
    g = np.asarray(gidx_of_rank, np.int64)
    assert np.all(np.diff(g) > 0), "the owned numbers ascend by row"
    dele = np.asarray([int(d) for d in delete], np.int64)
    rep = np.asarray([int(r) for r in replace[0]] if replace is not None else [], np.int64)
    n_rep, n_app = n_staged(edit)
    own = np.asarray(owner if n_app else [], np.int64)

    def find(names):
        row = np.searchsorted(g, names)
        ok = (row < len(g)) & (g[np.minimum(row, len(g) - 1)] == names) if len(g) else np.zeros(len(names), bool)
        return row, ok
    drow, dok = find(dele)
    rrow, rok = find(rep)
    taken = np.nonzero(own == rank)[0]
    kept = np.ones(len(g), bool); kept[drow[dok]] = False
    new_kept = g[kept] - np.searchsorted(dele, g[kept], side="left")
    new_app = n_global - len(dele) + taken
    return dict(del_rows=drow[dok], rep_rows=rrow[rok], staged=np.concatenate([np.nonzero(rok)[0], n_rep + taken]).astype(np.int64),
                found_del=int(dok.sum()), found_rep=int(rok.sum()), taken=len(taken), gidx=np.concatenate([new_kept, new_app]).astype(np.int64))


def verdict(gidx_by_rank, edit, owner, state_bits=None):
    """the agreement in front of the change, from the records {bits, rows owned, del found, rep found, appended taken} of all ranks: None (the
    edit goes ahead on every rank) or (code, reason), the same on every rank.  state_bits[r]: "ghosts", "order", "error", "rowcap" or None"""
    nranks = len(gidx_by_rank)
    fault = argument_fault(edit, owner, nranks)
    if fault:
        return E_ARG, fault
    delete, replace, append = edit
    n_rep, n_app = n_staged(edit)
    if len(delete) + n_rep + n_app == 0:
        return None
    n_global = sum(len(g) for g in gidx_by_rank)
    bits = set(b for b in (state_bits or []) if b)
    for b, code in (("error", E_CAPACITY), ("ghosts", E_STATE), ("order", E_STATE), ("rowcap", E_CAPACITY)):
        if b in bits:
            return code, b
    if any(len(g) == 0 for g in gidx_by_rank):
        return E_STATE, "a rank holds no floe"
    sh = [share(g, edit, owner, r, n_global) for r, g in enumerate(gidx_by_rank)]
    if sum(s["found_del"] for s in sh) != len(delete) or sum(s["found_rep"] for s in sh) != n_rep:
        return E_ARG, "a name out of range or owned twice"
    if n_global - len(delete) + n_app <= 0:
        return E_ARG, "the edit leaves no floe"
    for r, s in enumerate(sh):
        if len(gidx_by_rank[r]) - s["found_del"] + s["taken"] <= 0:
            return E_ARG, "the edit leaves rank %d without a floe" % r
    return None


def staged_floes(edit):
    """the replacements, then the appended floes, as one list (None: none)"""
    delete, replace, append = edit
    parts = [p for p in ((replace[1] if replace is not None else None), append) if p is not None and sp.n_rows(p)]
    if not parts:
        return None
    out = parts[0]
    for p in parts[1:]:
        out = sp.apply(out, append=p)
    return out


def apply_share(cols_of_rank, s, edit):
    """the rank's list behind its share: splice_ref.apply with the local rows and the staged floes it takes (its rows then carry s["gidx"])"""
    n_rep, n_app = n_staged(edit)
    st = staged_floes(edit)
    mine = [int(j) for j in s["staged"]]
    rep = [j for j in mine if j < n_rep]
    app = [j for j in mine if j >= n_rep]
    return sp.apply(cols_of_rank, list(s["del_rows"]), (list(s["rep_rows"]), sp.take(st, rep)) if rep else None, sp.take(st, app) if app else None)
