"""CPU: the caller's surface stated once -- every entry point refuses a NULL handle; the binding's Stats is the header's ufm_stats,
field by field; the table that merges the shards' statistics of a batch (csrc/ufm_capi.h) has a row for every field."""
import ctypes
import os
import re
import subprocess

import pytest

import ufm_amd
from ufm_amd_pkg import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UFM_ERR_INVALID = -22
NO_HANDLE = {"ufm_create", "ufm_batch_create", "ufm_batch_create_sharded", "ufm_version", "ufm_tile_edge", "ufm_gaussian_taps"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(ufm_amd.library_path()):
        ufm_amd.build_library()
    return ufm_amd.load_library()


def test_every_entry_point_refuses_a_null_handle(lib):
    """a NULL handle, zero or NULL for everything else (the argument lists come from the bound argtypes): UFM_ERR_INVALID, and NULL from
    the two calls that return a stream.  Nothing here reaches the GPU runtime."""
    names = [s for s in capi.SYMBOLS if s not in NO_HANDLE]
    assert len(names) == len(capi.SYMBOLS) - len(NO_HANDLE) == 92
    for name in names:
        fn = getattr(lib, name)
        assert fn.argtypes and fn.argtypes[0] is ctypes.c_void_p, name
        args = [0 if t is ctypes.c_int else 0.0 if t in (ctypes.c_float, ctypes.c_double) else None for t in fn.argtypes]
        got = fn(*args)
        if name.endswith("_stream"):
            assert got is None, name
        else:
            assert got == UFM_ERR_INVALID, (name, got)


def _header_stats_fields():
    txt = open(os.path.join(ROOT, "include", "ufm.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    body = re.search(r"typedef struct ufm_stats \{(.*?)\} ufm_stats;", txt, flags=re.S).group(1)
    fields = re.findall(r"\b(float|uint32_t|uint64_t)\s+(\w+)\s*;", body)
    assert len(fields) == body.count(";")       # (every member was understood)
    return fields


def test_stats_is_the_headers_struct(tmp_path):
    """a C program against include/ufm.h prints sizeof(ufm_stats) and every field's offset and size; capi.Stats has the same"""
    fields = _header_stats_fields()
    src = tmp_path / "stats.c"
    src.write_text('#include "ufm.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(ufm_stats));\n' +
                   "".join('  printf("%s %%zu %%zu\\n", offsetof(ufm_stats, %s), sizeof(((ufm_stats *)0)->%s));\n' % (n, n, n) for _, n in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "stats"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert int(out[0]) == ctypes.sizeof(capi.Stats)
    ctype = {"float": ctypes.c_float, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    assert [(n, ctype[t]) for t, n in fields] == list(capi.Stats._fields_)
    for line, (_, name) in zip(out[1:], fields):
        n, off, size = line.split()
        f = getattr(capi.Stats, name)
        assert (n, int(off), int(size)) == (name, f.offset, f.size)


def test_stats_merge_table_has_every_field():
    """ufm_batch_step merges the shards' ufm_stats through UFM_STATS_MERGE: one SUM or MAX row per field, in the header's order -- a
    field without a row would be dropped for sharded batches.  The two host-measured phase times are maxima, everything else a sum."""
    txt = open(os.path.join(os.path.dirname(ufm_amd.library_path()), "csrc", "ufm_capi.h")).read()
    body = txt[txt.index("#define UFM_STATS_MERGE(SUM, MAX)"):]
    rows = re.findall(r"\b(SUM|MAX)\((\w+)\)", body[:body.index("\nstatic")])
    assert [n for _, n in rows] == [n for _, n in _header_stats_fields()]
    assert [n for kind, n in rows if kind == "MAX"] == ["u_ms", "p_ms"]
