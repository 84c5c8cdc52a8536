"""rtg_scene_update and rtg_scene_top_hash without a GPU: host-only scenes and the argument
checks.

Equality: a scene built from descriptor A and updated to B has the top-level hash, the composed matrices of
every entry and the top-level build statistics of a scene freshly built from B; updated back to A it has
A's hash again.  The hash covers the host image of everything the top-level phases upload, so this holds
the update to a fresh build bit for bit.  Refusals: a changed frozen field is RTG_ERR_UNSUPPORTED and leaves
the scene as it was."""
import copy
import ctypes as C

import numpy as np
import pytest

from rtg import _abi as A
from rtg import scenegen
from rtg.scene import Material

import update_cases as U

INVALID, UNSUPPORTED = -1, -5


class Host:
    """A host-only scene (RTG_DEVICE_HOST_ONLY) through the C ABI."""

    def __init__(self, lib, sc, tlas=0):
        self.lib = lib
        desc, self.keep = sc.to_desc()
        self.h = C.c_void_p()
        bo = A.BuildOpts(0, tlas, 0, 0)
        A.check(lib.rtg_scene_create_ex(C.byref(desc), A.RTG_DEVICE_HOST_ONLY, C.byref(bo), C.byref(self.h)), lib)

    def update(self, sc, geometry=False):
        desc, keep = sc.to_desc(geometry=geometry)
        return self.lib.rtg_scene_update(self.h, C.byref(desc))

    def hash(self):
        out = C.c_uint64()
        A.check(self.lib.rtg_scene_top_hash(self.h, C.byref(out)), self.lib)
        return out.value

    def matrices(self, n):
        m = np.zeros((n, 2, 16), np.float32)
        for i in range(n):
            A.check(self.lib.rtg_scene_object_matrices(self.h, i, m[i, 0].ctypes.data_as(A.PF),
                                                       m[i, 1].ctypes.data_as(A.PF)), self.lib)
        return m.view(np.int32)

    def stats(self):
        b = A.BuildStats()
        A.check(self.lib.rtg_scene_build_stats(self.h, C.byref(b)), self.lib)
        return b

    def close(self):
        if self.h:
            assert self.lib.rtg_scene_destroy(self.h) == 0
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _same_as_fresh(lib, s, sc, tlas=0):
    with Host(lib, sc, tlas) as fresh:
        assert s.hash() == fresh.hash()
        n = U.entries(sc)
        assert np.array_equal(s.matrices(n), fresh.matrices(n))
        a, b = s.stats(), fresh.stats()
        assert (a.tlas_nodes, a.flat_group_entries) == (b.tlas_nodes, b.flat_group_entries)
        return b


@pytest.mark.parametrize("tlas", [0, 2])
@pytest.mark.parametrize("name,variant", U.CASES)
def test_update_equals_fresh_build(lib, name, variant, tlas):
    a, b = U.pair(name, variant)
    with Host(lib, a, tlas) as s:
        ha = s.hash()
        before = s.stats()
        assert s.update(b) == A.RTG_OK, lib.rtg_last_error()
        _same_as_fresh(lib, s, b, tlas)
        after = s.stats()
        # the per-object fields stay as built
        assert (after.traversal_nodes, after.traversal_hash, after.num_objects) == \
               (before.traversal_nodes, before.traversal_hash, before.num_objects)
        assert after.upload_bytes == 0 and after.upload_ms == 0.0       # host-only: nothing uploaded
        assert s.update(a) == A.RTG_OK, lib.rtg_last_error()
        assert s.hash() == ha
        _same_as_fresh(lib, s, a, tlas)


def test_every_variant_applies_somewhere():
    assert {v for _, v in U.CASES} == set(U.VARIANTS)
    assert {n for n, _ in U.CASES} == set(U.SCENES)


def test_variants_change_the_hash(lib):
    """The hash tells the descriptors apart: every B differs from its A."""
    for name, variant in U.CASES:
        if (name, variant) == ("ties", "reset_transform"):
            continue        # its base mesh has the identity transform: the flag changes nothing there
        a, b = U.pair(name, variant)
        with Host(lib, a) as sa, Host(lib, b) as sb:
            assert sa.hash() != sb.hash(), (name, variant)


@pytest.mark.parametrize("name", ["cornell", "cornell_pt"])
def test_a_mesh_leaves_the_flat_group_and_returns(lib, name):
    a, b = U.pair(name, "leave_group")
    with Host(lib, a) as s:
        n = s.stats().flat_group_entries
        assert n >= 2
        assert s.update(b) == A.RTG_OK
        assert s.stats().flat_group_entries == n - 1
        assert s.update(a) == A.RTG_OK
        assert s.stats().flat_group_entries == n


def test_updates_compose(lib):
    """A -> B1 -> B2 -> ... each equal to a fresh build, with one scene."""
    with Host(lib, U.scene("cornell")) as s:
        for variant in ("transforms", "blur", "light_added", "singular", "scalars", "leave_group"):
            b = U.pair("cornell", variant)[1]
            assert s.update(b) == A.RTG_OK
            _same_as_fresh(lib, s, b)


def _refusal(field):
    """(scene A, changed scene, text the message must name)."""
    if field == "radius":
        a = U.scene("cornell"); b = copy.deepcopy(a); b.objects[0].radius = 1.25
    elif field == "face":
        a = U.scene("cornell"); b = copy.deepcopy(a); b.objects[1].faces = b.objects[1].faces[:-1]
    elif field == "smooth":
        a = U.scene("cornell"); b = copy.deepcopy(a); b.objects[4].smooth = False
    elif field == "is_light":
        a = U.scene("cornell_pt"); b = copy.deepcopy(a); b.objects[0].is_light = True
    elif field == "base_object":
        a = U.scene("cornell"); b = copy.deepcopy(a); b.instances[0].base_object = 1
    elif field == "intersection_test_eps":
        a = U.scene("cornell"); b = copy.deepcopy(a); b.int_eps = 0.002
    elif field == "decal":
        a = scenegen.textured(8, 6); b = copy.deepcopy(a); b.textures[0].decal = A.DECAL_BLEND_KD
    elif field == "num_objects":
        a = U.scene("multilight"); b = copy.deepcopy(a); b.objects.pop()
    elif field == "num_materials":
        a = U.scene("multilight"); b = copy.deepcopy(a); b.materials.append(Material())
    return a, b, field


@pytest.mark.parametrize("field", ["radius", "face", "smooth", "is_light", "base_object", "intersection_test_eps",
                                   "decal", "num_objects", "num_materials"])
def test_frozen_fields_are_refused(lib, field):
    a, b, text = _refusal(field)
    with Host(lib, a) as s:
        h = s.hash()
        m = s.matrices(U.entries(a))
        assert s.update(b) == UNSUPPORTED
        assert text.encode() in lib.rtg_last_error(), lib.rtg_last_error()
        assert s.hash() == h and np.array_equal(s.matrices(U.entries(a)), m)
        # and the scene still updates
        b2 = U.v_scalars(a)
        assert s.update(b2) == A.RTG_OK
        _same_as_fresh(lib, s, b2)


def test_null_arguments(lib):
    sc = U.scene("cornell")
    desc, keep = sc.to_desc(geometry=False)
    out = C.c_uint64()
    with Host(lib, sc) as s:
        assert lib.rtg_scene_update(None, C.byref(desc)) == INVALID
        assert lib.rtg_scene_update(s.h, None) == INVALID
        assert lib.rtg_scene_top_hash(None, C.byref(out)) == INVALID
        assert lib.rtg_scene_top_hash(s.h, None) == INVALID


def test_invalid_free_field_leaves_the_scene_working(lib):
    a = U.scene("cornell")
    bad = copy.deepcopy(a)
    bad.objects[2].material = 99
    with Host(lib, a) as s:
        h = s.hash()
        assert s.update(bad) == INVALID and b"material" in lib.rtg_last_error()
        bad2 = copy.deepcopy(a)
        bad2.instances[0].xforms = [(A.XF_TRANSLATION, 77)]
        assert s.update(bad2) == INVALID and b"transformation" in lib.rtg_last_error()
        assert s.hash() == h
        b = U.pair("cornell", "transforms")[1]
        assert s.update(b) == A.RTG_OK
        _same_as_fresh(lib, s, b)


def test_geometry_pointers_may_be_null_or_given(lib):
    a, b = U.pair("cornell", "transforms")
    desc, keep = b.to_desc(geometry=False)
    assert not desc.vertices and not desc.faces and not desc.texcoords and desc.num_vertices > 0 and desc.num_faces > 0
    with Host(lib, a) as s:
        assert s.update(b, geometry=False) == A.RTG_OK
        h = s.hash()
        assert s.update(a, geometry=True) == A.RTG_OK
        assert s.update(b, geometry=True) == A.RTG_OK
        assert s.hash() == h
    t = scenegen.textured(8, 6)
    t2 = U.v_scalars(t)
    desc, keep = t2.to_desc(geometry=False)
    assert not desc.textures[0].texels and desc.textures[0].width > 0
    with Host(lib, t) as s:
        assert s.update(t2) == A.RTG_OK
        _same_as_fresh(lib, s, t2)


def test_too_many_lights_is_refused_before_anything_changes(lib):
    a = U.scene("cornell_pt")                 # two object lights
    b = copy.deepcopy(a)
    for _ in range(63):
        b = U.v_light_added(b)
    with Host(lib, a) as s:
        h = s.hash()
        assert s.update(b) == UNSUPPORTED and b"lights" in lib.rtg_last_error()
        assert s.hash() == h
        assert s.update(a) == A.RTG_OK and s.hash() == h
