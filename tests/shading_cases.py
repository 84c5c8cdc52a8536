"""Scenes of the shading known-answer tests (tests/test_shading_kat.py on the CPU, tests/test_gpu_shading_kat.py
on the GPU), the conditions that keep a case from passing vacuously, and the comparison.  A helper, not a test.

Every frame is 4x3; the camera stands at (0, 0.5, 0) and looks along (0, -0.6, -1) through a near plane of
+-0.4 x +-0.3 at distance 1; the floor is y = -1.  Ambient, diffuse, specular, mirror and light colours differ
per channel so that a channel mix-up shows."""
import dataclasses

import numpy as np

import shading_ref
from rtg import _abi as A
from rtg.scene import Camera, Light, Material, Object, Scene, Texture

SEED = 0x5EED2026
HALF = 200.0                            # half-extent of a plane's two triangles
TOL = 1e-5                              # |got - ref| <= TOL * (largest reference channel of the pixel)

BRDFS = {"none": A.BRDF_NONE, "obp": A.BRDF_OBP, "mbp": A.BRDF_MBP, "mbpn": A.BRDF_MBPN, "op": A.BRDF_OP,
         "mp": A.BRDF_MP, "mpn": A.BRDF_MPN, "ts": A.BRDF_TS, "tsf": A.BRDF_TSF}
EXPONENTS = (1, 8, 50)
LIGHTS = ("point", "directional", "spot", "area", "environment")


# ---------------------------------------------------------------------------------------------- scenes
def camera(spp=1):
    return Camera(position=np.float32([0, 0.5, 0]), gaze=np.float32([0, -0.6, -1]), up=np.float32([0, 1, 0]),
                  near_plane=(-0.4, 0.4, -0.3, 0.3), near_distance=1.0, nx=4, ny=3, num_samples=spp)


def add_rect(sc, y, up, material, x=(-HALF, HALF), z=(-HALF, HALF)):
    """A rectangle y = const as one mesh of two triangles whose winding gives the normal +y (`up`) or -y: the
    reference's flat normal is (c - b) x (a - b) (Shape.cpp:143)."""
    base = len(sc.vertices)
    quad = np.float32([[x[0], y, z[0]], [x[1], y, z[0]], [x[1], y, z[1]], [x[0], y, z[1]]])
    sc.vertices = np.concatenate([np.asarray(sc.vertices, np.float32).reshape(-1, 3), quad])
    faces = np.int32([[1, 3, 2], [1, 4, 3]]) if up else np.int32([[1, 2, 3], [1, 3, 4]])
    sc.objects.append(Object(type=A.OBJ_MESH, id=len(sc.objects) + 1, material=material, faces=faces + base))


def floor_material(brdf=A.BRDF_NONE, exponent=8, **kw):
    m = Material(type=A.MAT_NORMAL, brdf=brdf, phong_exp=exponent, ambient=(0.9, 0.6, 0.3),
                 diffuse=(0.7, 0.5, 0.3), specular=(0.3, 0.6, 0.9), refraction_index=2.2, absorption_index=3.1)
    return dataclasses.replace(m, **kw)


def light(kind):
    if kind == "point":
        return Light(type=A.LIGHT_POINT, position=(0.5, 3.0, -2.0), intensity=(30.0, 45.0, 60.0))
    if kind == "directional":
        return Light(type=A.LIGHT_DIRECTIONAL, direction=(0.3, -1.0, -0.2), intensity=(1.0, 1.5, 2.0))
    if kind == "spot":
        return spot_light()
    if kind == "area":
        return Light(type=A.LIGHT_AREA, position=(0.3, 3.0, -2.5), direction=(0.1, -1.0, 0.2),
                     intensity=(20.0, 30.0, 40.0), size=1.5)
    raise ValueError(kind)


def spot_light():
    """A spot along (0, -1, -0.1) with 60 degrees of coverage and 20 of falloff, placed so that pixels fall in
    all three zones and none within 2 degrees of a zone boundary (spot_zones asserts it)."""
    return Light(type=A.LIGHT_SPOT, position=(0.2, 3.0, -1.0), direction=(0.0, -1.0, -0.1),
                 intensity=(30.0, 45.0, 60.0), coverage_deg=60.0, falloff_deg=20.0)


def base_scene(depth=1):
    sc = Scene(max_depth=depth, shadow_eps=0.002, int_eps=0.001, background=(0.0, 0.0, 0.0),
               ambient=(0.05, 0.1, 0.15))
    sc.cameras = [camera()]
    return sc


def add_environment(sc):
    """A uniform environment map: all texels equal, so the texel lookup cannot matter."""
    texels = np.empty((4, 8, 3), np.float32)
    texels[:] = (0.8, 0.6, 0.4)
    sc.textures.append(Texture(kind=A.TEX_IMAGE, decal=A.DECAL_NONE, interp=A.INTERP_BILINEAR, normalizer=1,
                               texels=texels))
    sc.environment_light = len(sc.lights)
    sc.lights.append(Light(type=A.LIGHT_ENVIRONMENT, texture=len(sc.textures) - 1))


def direct(kind, brdf="none", exponent=8, extra=()):
    """The floor under one light (and `extra` ones)."""
    sc = base_scene()
    sc.materials = [floor_material(BRDFS[brdf], exponent)]
    add_rect(sc, -1.0, True, 1)
    for k in (kind,) + tuple(extra):
        if k == "environment":
            add_environment(sc)
        else:
            sc.lights.append(light(k))
    return sc


def grazing(brdf):
    """Two directional lights, one of them 0.0005 above the horizon: the "original" BRDFs cut it
    (cos theta_i < 0.001, Light.cpp:77-80, 106-109), the others do not."""
    sc = direct("directional", brdf, 8)
    sc.lights.append(Light(type=A.LIGHT_DIRECTIONAL, direction=(1.0, -0.0005, 0.0), intensity=(900.0, 700.0, 500.0)))
    return sc


OCCLUDER = dict(y=1.0, x=(-0.25, 0.25), z=(-2.6, -1.9))
SHADOW_LIGHT = (0.0, 3.0, -2.5)


def shadow():
    """A point light over a small quad that shadows some of the floor's pixels."""
    sc = base_scene()
    sc.materials = [floor_material(), floor_material()]
    add_rect(sc, -1.0, True, 1)
    add_rect(sc, OCCLUDER["y"], True, 2, OCCLUDER["x"], OCCLUDER["z"])
    sc.lights.append(Light(type=A.LIGHT_POINT, position=SHADOW_LIGHT, intensity=(30.0, 45.0, 60.0)))
    return sc


def reflector(kind, depth):
    """A mirror or conductor floor under a diffuse ceiling at y = 4, a point light between them."""
    sc = base_scene(depth)
    mtype = {"mirror": A.MAT_MIRROR, "conductor": A.MAT_CONDUCTOR}[kind]
    sc.materials = [floor_material(type=mtype, mirror=(0.9, 0.7, 0.5)),
                    Material(type=A.MAT_NORMAL, phong_exp=3, ambient=(0.4, 0.6, 0.8), diffuse=(0.3, 0.5, 0.7),
                             specular=(0.2, 0.1, 0.3))]
    add_rect(sc, -1.0, True, 1)
    add_rect(sc, 4.0, False, 2)
    sc.lights.append(Light(type=A.LIGHT_POINT, position=(0.5, 2.0, -2.0), intensity=(30.0, 45.0, 60.0)))
    return sc


def slab(absorption, depth):
    """A glass slab, faces y = -1 (normal +y) and y = -1.5 (normal -y), index 1.5, over a diffuse floor at
    y = -3 and under a diffuse ceiling at y = 1.5, one point light between slab and floor and one above the slab.
    The ceiling is there because the reference takes the Beer distance of a transmitted ray that misses from an
    uninitialised hit record.  The glass has no diffuse or specular part: the shadow ray of a point on the top
    face towards the light below starts 0.002 above the face it then has to cross."""
    sc = base_scene(depth)
    sc.materials = [Material(type=A.MAT_DIELECTRIC, phong_exp=5, ambient=(0.3, 0.5, 0.7), diffuse=(0.0, 0.0, 0.0),
                             specular=(0.0, 0.0, 0.0), refraction_index=1.5, absorption_coeff=absorption),
                    floor_material(),
                    Material(type=A.MAT_NORMAL, phong_exp=3, ambient=(0.4, 0.6, 0.8), diffuse=(0.3, 0.5, 0.7),
                             specular=(0.2, 0.1, 0.3))]
    add_rect(sc, -1.0, True, 1)
    add_rect(sc, -1.5, False, 1)
    add_rect(sc, -3.0, True, 2)
    add_rect(sc, 1.5, False, 3)
    sc.lights.append(Light(type=A.LIGHT_POINT, position=(0.3, -2.2, -2.5), intensity=(30.0, 45.0, 60.0)))
    sc.lights.append(Light(type=A.LIGHT_POINT, position=(-0.4, 0.8, -7.0), intensity=(60.0, 45.0, 30.0)))
    return sc


def multisample():
    """Four samples a pixel under a point and an area light: the mean of four closed-form samples."""
    sc = direct("point", "none", 8, extra=("area",))
    sc.cameras = [camera(4)]
    return sc


def variant(sc):
    """The k_shade instantiation a scene's content selects (derive_view in csrc/rtg_host.cpp, launch_shade_t
    in csrc/rtg_device.hip), restated to name the GPU cases."""
    kinds = {l.type for l in sc.lights}
    brdf = any(m.brdf != A.BRDF_NONE for m in sc.materials)
    tex = brdf or any(o.textures for o in sc.objects)
    full = (brdf or bool(sc.textures) or sc.background_texture != -1 or sc.environment_light != -1
            or A.LIGHT_AREA in kinds or A.LIGHT_ENVIRONMENT in kinds)
    spot = A.LIGHT_SPOT in kinds
    heavy = spot or sc.environment_light != -1 or A.LIGHT_ENVIRONMENT in kinds
    if full:
        return "full" + ("+tex" if tex else "") + ("+heavy" if heavy else "")
    return "simple" + ("+spot" if spot else "")


# ---------------------------------------------------------------------------------------------- reference
def reference(sc, rng):
    """(image, Ref) in float64."""
    ref = shading_ref.Ref(sc, rng=rng, seed=SEED)
    return ref.render(0), ref


def unlit(sc):
    return dataclasses.replace(sc, lights=[], environment_light=-1)


def assert_lit(sc, img, rng, what):
    """At least half the pixels have a light term above 1 % of their ambient term: the frame against the same
    frame without lights."""
    amb = reference(unlit(sc), rng)[0]
    lit = (img - amb).max(axis=-1) > 0.01 * amb.max(axis=-1)
    assert amb.max(axis=-1).min() > 0 and 2 * lit.sum() >= lit.size, f"{what}: {lit.sum()} of {lit.size} pixels lit"


def spot_zones(ref):
    """Pixels per zone (full, falloff, outside) of the first light, each at least 2 degrees from a boundary."""
    rec = ref.records("spot", path=1)
    assert len(rec) == 12
    margin = np.radians(2.0)
    zones = [0, 0, 0]
    for _, _, _, _, (angle, fall, coverage) in rec:
        assert abs(angle - fall) >= margin and abs(angle - coverage) >= margin, \
            f"a pixel {np.degrees(angle):.2f} degrees off the axis is within 2 degrees of a zone boundary"
        zones[0 if angle < fall else (1 if angle < coverage else 2)] += 1
    return zones


def shadow_census(ref):
    """(lit, shadowed, least distance of a shading point from the shadow's edge on the floor)."""
    lx, ly, lz = SHADOW_LIGHT
    lit = dark = 0
    least = np.inf
    for _, _, _, _, (_, light_term, p) in ref.records("basic", path=1):
        k = (ly - p[1]) / (ly - OCCLUDER["y"])                     # the quad's shadow, projected from the light
        x0, x1 = (lx + (x - lx) * k for x in OCCLUDER["x"])
        z0, z1 = (lz + (z - lz) * k for z in OCCLUDER["z"])
        inside = x0 < p[0] < x1 and z0 < p[2] < z1
        if inside:
            d = min(p[0] - x0, x1 - p[0], p[2] - z0, z1 - p[2])
        else:
            d = np.hypot(max(x0 - p[0], 0, p[0] - x1), max(z0 - p[2], 0, p[2] - z1))
        least = min(least, d)
        assert inside == (light_term.max() == 0.0)
        dark += inside
        lit += not inside
    return lit, dark, least


def assert_slab(ref, absorbing):
    """The Fresnel reflectance at the first hit lies in (0.02, 0.5); with absorption the three Beer factors
    differ by more than 10 %."""
    rec = ref.records("dielectric", path=1)
    assert len(rec) == 12
    for _, _, _, _, (entering, fresnel, beer) in rec:
        assert entering and 0.02 < fresnel < 0.5
        if absorbing:
            b = np.sort(beer)
            assert b[1] > 1.1 * b[0] and b[2] > 1.1 * b[1]


# ---------------------------------------------------------------------------------------------- comparison
def deviation(got, ref):
    """Worst |got - ref| over the pixel's largest reference channel."""
    scale = ref.max(axis=-1, keepdims=True)
    return float((np.abs(np.asarray(got, np.float64) - ref) / scale).max())


def assert_close(got, ref, what):
    dev = deviation(got, ref)
    print(f"{what}: worst relative deviation {dev:.3g}")
    assert np.isfinite(np.asarray(got)).all() and ref.max(axis=-1).min() > 0
    assert (np.abs(np.asarray(got, np.float64) - ref) <= TOL * ref.max(axis=-1, keepdims=True)).all(), \
        f"{what}: {dev:.3g} of the pixel's largest channel"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)
