"""The C-ABI of the contact queries as Python sees it: the library exports mi_contact_query_batch and mi_contact_query_host, the query
record is mi_overlap_query itself, the numpy dtypes have the sizes and the field order of include/mi_physics.h's structs, the flags and
the cap have its values.  Needs no GPU."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contactquery64 as c64  # noqa: E402
import overlap64 as o64  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "mi_physics.h")) as f:
        return f.read()


def _struct_fields(header, name):
    """[field name] of `typedef struct name { ... } name;` in declaration order (arrays by their name, comments dropped)"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", part).strip() for part in decl.split(None, 1)[1].split(",")]
    return names


def test_library_exports_the_contact_query_entries(mi):
    lib = mi.load_library()
    assert "mi_contact_query_batch" in mi.EXPORTED_SYMBOLS and "mi_contact_query_host" in mi.EXPORTED_SYMBOLS
    assert lib.mi_contact_query_batch is not None and lib.mi_contact_query_host is not None
    h = _header()
    assert re.search(r"int mi_contact_query_batch\(mi_world\* w, uint32_t numQueries, const mi_contact_query\* dQueries, uint32_t maxHits, uint32_t flags, void\* dOut, float\* dOutWorldShapes\);", h)
    assert re.search(r"int mi_contact_query_host\(mi_world\* w, uint32_t numQueries, const mi_contact_query\* queries, uint32_t maxHits, uint32_t flags, void\* out, float\* outWorldShapes\);", h)
    assert hasattr(mi.World, "contact_query")


def test_the_query_record_is_overlaps(mi):
    h = _header()
    assert re.search(r"typedef mi_overlap_query mi_contact_query;", h) and not re.search(r"typedef struct mi_contact_query \{", h)
    assert mi.CONTACT_QUERY_DTYPE == mi.OVERLAP_QUERY_DTYPE == o64.QUERY_DTYPE and mi.CONTACT_QUERY_DTYPE.itemsize == 96


def test_dtypes_match_the_header(mi):
    h = _header()
    assert mi.CONTACT_QUERY_SUMMARY_DTYPE.itemsize == 32 and mi.CONTACT_QUERY_RECORD_DTYPE.itemsize == 96
    assert list(mi.CONTACT_QUERY_SUMMARY_DTYPE.names) == _struct_fields(h, "mi_contact_query_summary") == [
        "numContacts", "numWritten", "valid", "reserved0", "deepestCollider", "deepestBody", "deepestDepth", "reserved1"]
    assert list(mi.CONTACT_QUERY_RECORD_DTYPE.names) == _struct_fields(h, "mi_contact_query_record") == ["collider", "body", "count", "reserved", "normal", "maxDepth", "points"]
    assert {n: mi.CONTACT_QUERY_SUMMARY_DTYPE.fields[n][1] for n in mi.CONTACT_QUERY_SUMMARY_DTYPE.names} == {
        "numContacts": 0, "numWritten": 4, "valid": 8, "reserved0": 12, "deepestCollider": 16, "deepestBody": 20, "deepestDepth": 24, "reserved1": 28}
    assert {n: mi.CONTACT_QUERY_RECORD_DTYPE.fields[n][1] for n in mi.CONTACT_QUERY_RECORD_DTYPE.names} == {
        "collider": 0, "body": 4, "count": 8, "reserved": 12, "normal": 16, "maxDepth": 28, "points": 32}
    assert mi.CONTACT_QUERY_RECORD_DTYPE["points"].shape == (4, 4) and mi.CONTACT_QUERY_RECORD_DTYPE["points"].base == np.dtype("<f4")
    assert mi.CONTACT_QUERY_SUMMARY_DTYPE["deepestDepth"] == np.dtype("<f4") and mi.CONTACT_QUERY_RECORD_DTYPE["maxDepth"] == np.dtype("<f4")
    assert mi.CONTACT_QUERY_SUMMARY_DTYPE == c64.SUMMARY_DTYPE and mi.CONTACT_QUERY_RECORD_DTYPE == c64.RECORD_DTYPE
    assert re.search(r"32 \+ 96 \* maxHits bytes", h)


def test_flags_have_the_headers_values(mi):
    h = _header()
    assert re.search(r"enum \{ MI_CONTACT_QUERY_STATIC = 1, MI_CONTACT_QUERY_BRUTE_FORCE = 2 \};", h) and re.search(r"#define MI_CONTACT_QUERY_MAX_HITS 1024u", h)
    assert (mi.CONTACT_QUERY_STATIC, mi.CONTACT_QUERY_BRUTE_FORCE, mi.CONTACT_QUERY_MAX_HITS) == (1, 2, 1024)
