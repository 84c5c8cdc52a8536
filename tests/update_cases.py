"""Scenes and descriptor changes shared by tests/test_update_abi.py and tests/test_gpu_update.py
(rtg_scene_update).

SCENES: the base descriptors ("A").  VARIANTS: functions that return a changed deep copy ("B") of a scene,
touching only the free part of the descriptor, or None where the scene has nothing for the change to act on
(no instance to flip, no light to remove, ...).  CASES lists the (scene, variant) pairs that apply."""
import copy

import numpy as np

from rtg import _abi as A
from rtg import scenegen
from rtg.scene import Instance, Light, Object


def tie_scene():
    """Coincident entries (as tests/test_gpu_queries.py builds them): the same sphere three times and the same
    mesh as an object and as two instances with identity transforms -- every hit is a tie broken by the loop
    order."""
    sc = scenegen.simple(8, 6)
    sc.objects = []
    c = len(sc.vertices) + 1
    sc.vertices = np.concatenate([np.asarray(sc.vertices, np.float32),
                                  np.float32([[0.0, 0.0, -2.0], [-1, -0.5, -1.5], [1, -0.5, -1.5], [0, 0.7, -3.0]])])
    while len(sc.materials) < 6:
        sc.materials.append(sc.materials[len(sc.materials) % 3])
    for m in (2, 1, 3):
        sc.objects.append(Object(type=0, id=len(sc.objects) + 1, material=m, center=c, radius=0.5))
    sc.objects.append(Object(type=2, id=10, material=4, faces=np.array([[c + 1, c + 2, c + 3]], np.int32)))
    base = len(sc.objects) - 1
    sc.instances.append(Instance(base_object=base, id=11, material=5, reset_transform=False))
    sc.instances.append(Instance(base_object=base, id=12, material=6, reset_transform=True))
    return sc


SCENES = {
    "cornell": lambda: scenegen.cornell(8, 6, spp=1),
    "spheres": lambda: scenegen.spheres(8, 6, spp=1, n=300),
    "cornell_pt": lambda: scenegen.cornell_pt(8, 6, spp=1),
    "multilight": lambda: scenegen.multilight(8, 6),
    "ties": tie_scene,
}

_BASE = {}


def scene(name):
    """A fresh deep copy of base scene `name` (the generators run once)."""
    if name not in _BASE:
        _BASE[name] = SCENES[name]()
    return copy.deepcopy(_BASE[name])


def _last_mesh(sc):
    idx = [i for i, o in enumerate(sc.objects) if o.type == A.OBJ_MESH]
    return idx[-1] if idx else None


def v_transforms(sc):
    """Every entry of every transformation table changed; a scene without tables gets a rotation and a
    translation on its last mesh."""
    sc = copy.deepcopy(sc)
    if not (sc.translations or sc.scalings or sc.rotations or sc.composites):
        m = _last_mesh(sc)
        if m is None:
            return None
        sc.translations.append((0.3, -0.2, 0.4))
        sc.rotations.append((33.0, 0.3, 1.0, -0.2))
        sc.objects[m].xforms = [(A.XF_ROTATION, 1), (A.XF_TRANSLATION, 1)]
        return sc
    sc.translations = [(x + 0.25, y - 0.125, z + 0.5) for x, y, z in sc.translations]
    sc.scalings = [(x * 1.25, y * 0.75, z * 1.125) for x, y, z in sc.scalings]
    sc.rotations = [(a + 17.0, x + 0.25, y, z - 0.5) for a, x, y, z in sc.rotations]
    sc.composites = [tuple(np.asarray(c, np.float32) * np.float32(1.5)) for c in sc.composites]
    return sc


def v_reset_transform(sc):
    if not sc.instances:
        return None
    sc = copy.deepcopy(sc)
    sc.instances[0].reset_transform = not sc.instances[0].reset_transform
    return sc


def v_blur(sc):
    """Blur set where it was zero and cleared where it was set."""
    sc = copy.deepcopy(sc)
    for k, e in enumerate(list(sc.objects) + list(sc.instances)):
        e.blur = (0.0, 0.0, 0.0) if any(float(b) != 0.0 for b in e.blur) else (0.125 * (k % 3), 0.25, -0.0625 * (k % 2))
    return sc


def v_materials_permuted(sc):
    sc = copy.deepcopy(sc)
    ents = list(sc.objects) + list(sc.instances)
    mats = [e.material for e in ents]
    if len(set(mats)) < 2:
        return None
    for e, m in zip(ents, mats[1:] + mats[:1]):
        e.material = m
    return sc


def v_material_dielectric(sc):
    """The first plain material becomes a dielectric that absorbs."""
    sc = copy.deepcopy(sc)
    for m in sc.materials:
        if m.type == A.MAT_NORMAL:
            m.type = A.MAT_DIELECTRIC
            m.refraction_index = 1.5
            m.absorption_coeff = (0.1, 0.2, 0.3)
            return sc
    return None


def v_light_added(sc):
    sc = copy.deepcopy(sc)
    sc.lights.append(Light(type=A.LIGHT_SPOT, position=(-2.0, 6.0, 3.0), direction=(0.3, -1.0, -0.4),
                           intensity=(9000, 7000, 5000), coverage_deg=50, falloff_deg=30))
    return sc


def v_light_removed(sc):
    if not sc.lights:
        return None
    sc = copy.deepcopy(sc)
    sc.lights.pop()
    return sc


def v_point_to_area(sc):
    sc = copy.deepcopy(sc)
    for l in sc.lights:
        if l.type == A.LIGHT_POINT:
            l.type, l.direction, l.size = A.LIGHT_AREA, (0.2, -1.0, 0.1), 1.5
            return sc
    return None


def v_scalars(sc):
    sc = copy.deepcopy(sc)
    sc.background = tuple(float(x) + 7.0 for x in sc.background)
    sc.ambient = tuple(float(x) + 3.0 for x in sc.ambient)
    sc.shadow_eps = float(sc.shadow_eps) * 4.0
    sc.max_depth = int(sc.max_depth) + 1
    return sc


def group_candidates(sc):
    """The untransformed small meshes of a linear-loop scene: where the flat group forms."""
    if len(sc.objects) + len(sc.instances) >= 16:
        return []
    return [i for i, o in enumerate(sc.objects)
            if o.type == A.OBJ_MESH and not o.xforms and len(np.asarray(o.faces).reshape(-1, 3)) <= 8
            and not any(float(b) != 0.0 for b in o.blur)]


def v_leave_group(sc):
    """The second member of the flat group gets a transform of its own: it must leave the group."""
    c = group_candidates(sc)
    if len(c) < 2:
        return None
    sc = copy.deepcopy(sc)
    sc.translations.append((0.0, 0.0, -0.25))
    sc.objects[c[1]].xforms = [(A.XF_TRANSLATION, len(sc.translations))]
    return sc


def v_singular(sc):
    """A scaling of 0 on one axis on the last mesh: a singular matrix."""
    m = _last_mesh(sc)
    if m is None:
        return None
    sc = copy.deepcopy(sc)
    sc.scalings.append((1.0, 0.0, 1.0))
    sc.objects[m].xforms = list(sc.objects[m].xforms) + [(A.XF_SCALING, len(sc.scalings))]
    return sc


VARIANTS = {
    "transforms": v_transforms,
    "reset_transform": v_reset_transform,
    "blur": v_blur,
    "materials_permuted": v_materials_permuted,
    "material_dielectric": v_material_dielectric,
    "light_added": v_light_added,
    "light_removed": v_light_removed,
    "point_to_area": v_point_to_area,
    "scalars": v_scalars,
    "leave_group": v_leave_group,
    "singular": v_singular,
}

_PAIRS = {}


def pair(name, variant):
    """(A, B) of a case: deep copies, B None where the variant does not apply."""
    key = (name, variant)
    if key not in _PAIRS:
        _PAIRS[key] = VARIANTS[variant](scene(name))
    b = _PAIRS[key]
    return scene(name), (None if b is None else copy.deepcopy(b))


CASES = [(n, v) for v in VARIANTS for n in SCENES if pair(n, v)[1] is not None]


def entries(sc):
    return len(sc.objects) + len(sc.instances)


def bits(a):
    """float32 array as its int32 bits (NaN-safe equality)."""
    return np.ascontiguousarray(a, np.float32).view(np.int32)
