"""The request structs at the engine's boundary without a GPU: skw_full_request and skw_sample_rows_request as a C compiler lays them out (tests/cpp/request_layout.c, which
includes include/skw_engine.h as C) are the ctypes structures streamkit_amd/engine.py fills, field for field; SKW_FULL_REQUEST_MIN is the struct as first published; and
libskw_engine.so exports the two request entries beside every entry point and hook they stand behind."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

NEW_SYMBOLS = ["skw_full_batch_request", "skw_debug_sample_rows_request"]
OLD_SYMBOLS = ["skw_full_batch", "skw_full_batch_rng", "skw_full_batch_mixed", "skw_full_batch_context", "skw_full_batch_rules", "skw_full_batch_aligned", "skw_full_batch_grammar",
               "skw_full_batch_traced", "skw_full_batch_traced_context", "skw_align_batch",
               "skw_debug_sample_rows", "skw_debug_sample_rows_mixed", "skw_debug_sample_rows_rules", "skw_debug_sample_rows_grammar", "skw_debug_sample_rows_ex"]


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """{struct: {"sizeof": n, field: offset}} and the constants, as the C program prints them"""
    exe = tmp_path_factory.mktemp("request") / "request_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "request_layout.c")])
    out = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        w = line.split()
        if len(w) == 2:
            out[w[0]] = int(w[1])
        else:
            out.setdefault(w[0], {})[w[1]] = int(w[2])
    return out


@pytest.mark.parametrize("c_name, py_name", [("skw_full_request", "FullRequest"), ("skw_sample_rows_request", "SampleRowsRequest")])
def test_the_ctypes_structure_is_the_c_struct(layout, eng, c_name, py_name):
    S = getattr(eng, py_name)
    want = layout[c_name]
    assert C.sizeof(S) == want["sizeof"]
    got = {name: getattr(S, name).offset for name, _ in S._fields_}
    assert got == {k: v for k, v in want.items() if k != "sizeof"}      # (the same fields under the same names at the same offsets: none missing on either side)
    assert [n for n, _ in S._fields_] == sorted(got, key=got.get)        # (declared in the C order)
    for name, t in S._fields_:      # every pointer is a pointer and every scalar four bytes wide, as in the header
        assert C.sizeof(t) == (C.sizeof(C.c_void_p) if t is C.c_void_p or issubclass(t, C._Pointer) else 4), name


def test_the_minimum_size_is_the_struct_as_first_published(layout, eng):
    """a field appended later grows sizeof and leaves the constant: today the two are equal, and the binding's constant is the header's"""
    assert layout["SKW_FULL_REQUEST_MIN"] == eng.FULL_REQUEST_MIN == 136
    assert layout["skw_full_request"]["sizeof"] >= layout["SKW_FULL_REQUEST_MIN"]
    assert layout["skw_full_request"]["size"] == 0      # (the size comes first: it is read before anything else is trusted)
    assert C.sizeof(eng.FullRequest) >= eng.FULL_REQUEST_MIN


def test_the_library_exports_the_request_entries_and_every_entry_before_them(built):
    L = C.CDLL(os.path.join(ROOT, "streamkit_amd", "libskw_engine.so"))
    assert len(OLD_SYMBOLS) == 15 and len(set(OLD_SYMBOLS + NEW_SYMBOLS)) == 17
    for n in NEW_SYMBOLS + OLD_SYMBOLS:
        assert hasattr(L, n), "libskw_engine.so lacks %s" % n
