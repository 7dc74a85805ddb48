"""The entry points of include/pct_hip_holes.h: every one exported by the library and bound from the shim's second table,
_capi.HOLE_SIGNATURES; the first table stays the boundary of pct_hip.h and pct_hip_surface.h (no compute)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(*headers):
    text = "".join(open(os.path.join(ROOT, "include", h)).read() for h in headers)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pct_[a-z0-9_]+)\s*\(", text)))


def test_the_header_declares_the_five_calls():
    assert declared("pct_hip_holes.h") == sorted(("pct_fill_holes", "pct_get_hole_triangles", "pct_get_filled_triangles",
                                                  "pct_get_boundary_loops", "pct_fill_hole_stats"))
    text = open(os.path.join(ROOT, "include", "pct_hip_holes.h")).read()
    assert '#include "pct_hip_surface.h"' in text


def test_every_declared_symbol_is_exported_and_bound(built):
    capi = built["capi"]
    lib = ctypes.CDLL(capi.LIB_PATH)
    syms = declared("pct_hip_holes.h")
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in pct_hip_holes.h but not exported"
    assert sorted(capi.HOLE_SIGNATURES) == syms
    loaded = capi.load()
    for name, (res, args) in capi.HOLE_SIGNATURES.items():
        fn = getattr(loaded, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_first_table_is_unchanged(built):
    capi = built["capi"]
    assert sorted(capi.SIGNATURES) == declared("pct_hip.h", "pct_hip_surface.h")
    assert not set(capi.SIGNATURES) & set(capi.HOLE_SIGNATURES)
    assert capi.HOLE_MAX_VERTICES == 32
    text = open(os.path.join(ROOT, "include", "pct_hip_holes.h")).read()
    assert re.search(r"#define\s+PCT_HOLE_MAX_VERTICES\s+32\b", text)


def test_null_handles_are_refused(built):
    lib = built["capi"].load()
    out = (ctypes.c_int64 * 8)()
    assert lib.pct_fill_holes(None, 32, 1.0, 0) == built["capi"].PCT_ERR_INVALID
    assert lib.pct_get_hole_triangles(None, 0, 0, None) == built["capi"].PCT_ERR_INVALID
    assert lib.pct_get_filled_triangles(None, 0, 0, None) == built["capi"].PCT_ERR_INVALID
    assert lib.pct_get_boundary_loops(None, None, None, None) == built["capi"].PCT_ERR_INVALID
    assert lib.pct_fill_hole_stats(None, out, None) == built["capi"].PCT_ERR_INVALID
