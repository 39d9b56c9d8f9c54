"""tests/splice_ref.py pinned against hand-written lists (it is the oracle of tests/test_splice_gpu.py), and the new entry points in the
built library's export table.  No device is needed."""
import numpy as np

import splice_ref as sp


def _list(ids, npts, nsub, ninter):
    """floe k: id ids[k], cx = 10 id, a ring of npts[k] points with x = id + 0.01 j, nsub[k] sub-floe points, ninter[k] interaction rows whose
    first column is id + 0.5"""
    n = len(ids)
    ids = np.asarray(ids, np.int64)
    c = {"cx": 10.0 * ids, "cy": -1.0 * ids, "id": ids, "ghost_id": np.zeros(n, np.int64), "status": np.ones(n, np.int32),
         "stress_accum": np.stack([ids + 0.25 * q for q in range(4)], 1).astype(np.float64)}
    for off, vals, cnt in (("vert_off", ("vx", "vy"), npts), ("sub_off", ("sx", "sy"), nsub)):
        c[off] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        for s, v in enumerate(vals):
            c[v] = np.concatenate([i + 0.01 * np.arange(k) + 100.0 * s for i, k in zip(ids, cnt)] + [np.zeros(0)])
    c["inter_off"] = np.concatenate([[0], np.cumsum(ninter)]).astype(np.int32)
    c["inter_rows"] = np.concatenate([np.full((k, 7), i + 0.5) for i, k in zip(ids, ninter)] + [np.zeros((0, 7))])
    return c


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


BASE = dict(ids=[1, 2, 3, 4, 5], npts=[4, 5, 4, 6, 4], nsub=[2, 0, 3, 1, 2], ninter=[0, 2, 1, 0, 3])


def test_noop_is_the_list_itself():
    c = _list(**BASE)
    _same(sp.apply(c), c)


def test_delete_keeps_the_order_of_the_rest():
    c = _list(**BASE)
    _same(sp.apply(c, delete=[0, 3]), _list([2, 3, 5], [5, 4, 4], [0, 3, 2], [2, 1, 3]))
    _same(sp.apply(c, delete=[1, 2, 3, 4]), _list([1], [4], [2], [0]))


def test_replace_in_place_shifts_every_later_offset():
    c = _list(**BASE)
    new = _list([7], [9], [5], [4])
    got = sp.apply(c, replace=([1], new))
    _same(got, _list([1, 7, 3, 4, 5], [4, 9, 4, 6, 4], [2, 5, 3, 1, 2], [0, 4, 1, 0, 3]))
    assert got["vert_off"][2] == 13 and got["sub_off"][2] == 7 and got["inter_off"][2] == 4


def test_append_goes_behind_the_last_kept_row_in_the_order_given():
    c = _list(**BASE)
    new = _list([9, 8, 7], [4, 5, 6], [1, 1, 0], [0, 1, 0])
    _same(sp.apply(c, append=new), _list([1, 2, 3, 4, 5, 9, 8, 7], [4, 5, 4, 6, 4, 4, 5, 6], [2, 0, 3, 1, 2, 1, 1, 0], [0, 2, 1, 0, 3, 0, 1, 0]))
    _same(sp.apply(c, delete=[4], append=new), _list([1, 2, 3, 4, 9, 8, 7], [4, 5, 4, 6, 4, 5, 6], [2, 0, 3, 1, 1, 1, 0], [0, 2, 1, 0, 0, 1, 0]))


def test_replace_rows_are_numbers_of_the_list_before_the_deletion():
    """row 3 is replaced and rows 0 and 2 are deleted: the new floe ends up in row 1, next to a deleted neighbour"""
    c = _list(**BASE)
    new = _list([6, 7], [5, 4], [0, 4], [1, 1])
    got = sp.apply(c, delete=[0, 2], replace=([3, 4], new), append=_list([8], [4], [1], [0]))
    _same(got, _list([2, 6, 7, 8], [5, 5, 4, 4], [0, 0, 4, 1], [2, 1, 1, 0]))


def test_take_selects_in_the_order_asked():
    c = _list(**BASE)
    _same(sp.take(c, [4, 0, 2]), _list([5, 1, 3], [4, 4, 4], [2, 2, 3], [3, 0, 1]))


def test_resampled_and_scaled_rings_keep_their_shape():
    ring = np.array([[0.0, 0.0], [0.0, 2.0], [2.0, 2.0], [2.0, 0.0], [0.0, 0.0]])
    r2 = sp.resampled(ring)
    assert len(r2) == 9 and np.array_equal(r2[0], r2[-1]) and sp._area(r2) == 4.0
    s = sp.scaled(ring, 0.5)
    assert np.array_equal(s[0], s[-1]) and abs(sp._area(s) - 1.0) < 1e-12


def test_library_exports_the_entry_points():
    import ctypes

    import subzero_jl_amd
    from subzero_jl_amd import capi
    L = capi.load()
    names = ("sz_download_rows", "sz_splice_floes", "sz_download_rows_f32", "sz_splice_floes_f32")
    for n in names:
        assert n in capi.EXPORTS
        assert isinstance(getattr(L, n), ctypes._CFuncPtr)
        assert getattr(L, n).restype is ctypes.c_int
    raw = ctypes.CDLL(capi.lib_path())
    for n in names:
        assert getattr(raw, n) is not None
    assert subzero_jl_amd.World.splice and subzero_jl_amd.World.download_rows
