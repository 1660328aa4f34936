"""The C-ABI of the overlap queries as Python sees it: the library exports mi_overlap_batch and mi_overlap_host, the numpy dtypes have
the sizes and the field order of include/mi_physics.h's structs, the flags have its values.  Needs no GPU."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap64 as o64  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "mi_physics.h")) as f:
        return f.read()


def _struct_fields(header, name):
    """[field name] of `typedef struct name { ... } name;` in declaration order (arrays by their name)"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", part).strip() for part in decl.split(None, 1)[1].split(",")]
    return names


def test_library_exports_the_overlap_entries(mi):
    lib = mi.load_library()
    assert "mi_overlap_batch" in mi.EXPORTED_SYMBOLS and "mi_overlap_host" in mi.EXPORTED_SYMBOLS
    assert lib.mi_overlap_batch is not None and lib.mi_overlap_host is not None
    h = _header()
    assert re.search(r"int mi_overlap_batch\(mi_world\* w, uint32_t numQueries, const mi_overlap_query\* dQueries, uint32_t maxHits, uint32_t flags, void\* dOut, float\* dOutWorldShapes\);", h)
    assert re.search(r"int mi_overlap_host\(mi_world\* w, uint32_t numQueries, const mi_overlap_query\* queries, uint32_t maxHits, uint32_t flags, void\* out, float\* outWorldShapes\);", h)


def test_dtypes_match_the_header(mi):
    h = _header()
    assert mi.OVERLAP_QUERY_DTYPE.itemsize == 96 and mi.OVERLAP_SUMMARY_DTYPE.itemsize == 16 and mi.OVERLAP_HIT_DTYPE.itemsize == 8
    assert list(mi.OVERLAP_QUERY_DTYPE.names) == _struct_fields(h, "mi_overlap_query") == ["shape", "type", "enabled", "pos", "mount", "rot", "excludeFirst", "excludeCount", "reserved"]
    assert list(mi.OVERLAP_SUMMARY_DTYPE.names) == _struct_fields(h, "mi_overlap_summary") == ["numOverlaps", "numWritten", "valid", "reserved"]
    assert list(mi.OVERLAP_HIT_DTYPE.names) == _struct_fields(h, "mi_overlap_hit") == ["collider", "body"]
    offsets = {n: mi.OVERLAP_QUERY_DTYPE.fields[n][1] for n in mi.OVERLAP_QUERY_DTYPE.names}
    assert offsets == {"shape": 0, "type": 40, "enabled": 44, "pos": 48, "mount": 60, "rot": 64, "excludeFirst": 80, "excludeCount": 84, "reserved": 88}
    assert mi.OVERLAP_QUERY_DTYPE == o64.QUERY_DTYPE
    assert all(mi.OVERLAP_QUERY_DTYPE[n].base == np.dtype("<f4") for n in ("shape", "pos", "rot"))
    assert all(mi.OVERLAP_QUERY_DTYPE[n].base == np.dtype("<u4") for n in ("type", "enabled", "mount", "excludeFirst", "excludeCount", "reserved"))


def test_flags_have_the_headers_values(mi):
    h = _header()
    assert re.search(r"enum \{ MI_OVERLAP_STATIC = 1, MI_OVERLAP_BRUTE_FORCE = 2 \};", h) and re.search(r"#define MI_OVERLAP_MAX_HITS 1024u", h)
    assert (mi.OVERLAP_STATIC, mi.OVERLAP_BRUTE_FORCE, mi.OVERLAP_MAX_HITS) == (1, 2, 1024)
    for name in ("OVERLAP_QUERY_DTYPE", "OVERLAP_SUMMARY_DTYPE", "OVERLAP_STATIC", "OVERLAP_BRUTE_FORCE"):
        assert hasattr(mi, name)
