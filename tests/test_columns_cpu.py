"""The order of the floe columns, stated once in csrc/sz_columns.hpp, against the hand-written lists of the Python binding: no device."""
from subzero_jl_amd import capi


def _names():
    return capi.load().sz_debug_column_names().decode().split(" ")


def test_the_engine_and_the_binding_name_the_same_columns_in_the_same_order():
    assert _names() == capi.DCOLS + capi.TCOLS


def test_the_structs_of_the_binding_begin_with_these_columns():
    want = _names()
    assert len(want) == 28
    for struct in (capi.SzFloeColumns, capi.SzFloeColumnsF32):
        assert [n for n, _ in struct._fields_[:28]] == want, struct.__name__
