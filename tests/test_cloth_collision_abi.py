"""The C-ABI of cloth collision as Python sees it: the library exports the four entries, the ctypes mirror and the numpy dtype have the
size, field order and field types of include/mi_physics.h's mi_cloth_collision, the flags have its values.  Needs no GPU."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mi_cloth_set_collision", "mi_cloth_get_collision", "mi_cloth_read_contacts", "mi_debug_set_cloth_collision_brute_force")


def _header():
    with open(os.path.join(ROOT, "include", "mi_physics.h")) as f:
        return f.read()


def test_library_exports_the_entries(mi):
    lib = mi.load_library()
    h = _header()
    for name in ENTRIES:
        assert name in mi.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert re.search(r"int mi_cloth_set_collision\(mi_world\* w, uint32_t cloth, const mi_cloth_collision\* settings\);", h)
    assert re.search(r"int mi_cloth_get_collision\(mi_world\* w, uint32_t cloth, mi_cloth_collision\* out, int\* outEnabled\);", h)
    assert re.search(r"int mi_cloth_read_contacts\(mi_world\* w, uint32_t cloth, uint32_t\* outColliderPerParticle\);", h)
    assert re.search(r"int mi_debug_set_cloth_collision_brute_force\(mi_world\* w, int on\);", h)


def test_struct_matches_the_header(mi):
    h = _header()
    body = re.search(r"typedef struct mi_cloth_collision \{(.*?)\} mi_cloth_collision; /\* 32 bytes \*/", h, re.S).group(1)
    assert [d.strip() for d in body.split(";") if d.strip()] == ["float thickness, friction", "uint32_t flags, excludeFirst, excludeCount, reserved[3]"]
    names = ["thickness", "friction", "flags", "excludeFirst", "excludeCount", "reserved"]
    assert C.sizeof(mi.ClothCollision) == 32 and [n for n, _ in mi.ClothCollision._fields_] == names
    assert [t for _, t in mi.ClothCollision._fields_] == [C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32 * 3]
    assert mi.CLOTH_COLLISION_DTYPE.itemsize == 32 and list(mi.CLOTH_COLLISION_DTYPE.names) == names
    assert {n: mi.CLOTH_COLLISION_DTYPE.fields[n][1] for n in names} == {"thickness": 0, "friction": 4, "flags": 8, "excludeFirst": 12, "excludeCount": 16, "reserved": 20}
    assert all(mi.CLOTH_COLLISION_DTYPE[n].base == np.dtype("<f4") for n in names[:2]) and all(mi.CLOTH_COLLISION_DTYPE[n].base == np.dtype("<u4") for n in names[2:])
    assert {n: getattr(mi.ClothCollision, n).offset for n in names} == {n: mi.CLOTH_COLLISION_DTYPE.fields[n][1] for n in names}


def test_flags_have_the_headers_values(mi):
    assert re.search(r"enum \{ MI_CLOTH_COLLIDE_STATIC = 1, MI_CLOTH_COLLIDE_TERRAIN = 2 \};", _header())
    assert (mi.CLOTH_COLLIDE_STATIC, mi.CLOTH_COLLIDE_TERRAIN, mi.CLOTH_NO_CONTACT) == (1, 2, 0xFFFFFFFF)
    assert mi.CLOTH_COLLIDE_STATIC == mi.PROX_STATIC   # (the header maps one to the other; MI_PROX_TERRAIN is 8)
    for name in ("cloth_set_collision", "cloth_clear_collision", "cloth_collision", "cloth_contacts", "set_cloth_collision_brute_force"):
        assert callable(getattr(mi.World, name))
