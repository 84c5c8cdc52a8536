"""Shadow queries whose light term the ambient sum absorbs (shade_ray, SceneView::absorb_skip; DESIGN.md
section 16).  With one light a Whitted node's colour is fl(amb + c) if the light is visible and amb if it is
blocked; where fl(amb + c) has the bits of amb in every channel -- the far side of a mesh, where the diffuse
term is 0 and the specular lobe has fallen below half an ulp of the ambient term -- the query cannot change
the node and is not traced.  RTG_ABSORB_SKIP=0 at scene creation traces it as before (same device code).

The scene: scenegen.uv_sphere(64, 32) (4,096 triangles) with the dragon's material under the benchmark's
camera, light and scene ambient, at 96x54 and 4 spp.  Every frame must equal the oracle's bit for bit, which
traces every query; the switch may change the number of shadow rays and nothing else."""
import numpy as np
import pytest

import pyoracle
import rtg
from rtg import _abi as A
from rtg import scenegen
from rtg.scene import Light, Material, Object, Scene

pytestmark = pytest.mark.gpu

LIGHT = dict(position=(3, 5, 4), intensity=(22000, 22000, 22000))        # scenegen.dragon1m's


def _bits(a):
    return np.nan_to_num(np.ascontiguousarray(a, np.float32)).view(np.int32)


def _scene(ka=1.0, spheres=False, lights=1, max_depth=6, nx=96, ny=54, spp=4):
    sc = Scene(max_depth=max_depth, background=(15, 15, 30), ambient=(15, 15, 15))
    sc.cameras.append(scenegen._cam((0, 0.35, 3.6), (0, -0.08, -1), (0, 1, 0), nx, ny, fov_deg=45, spp=spp,
                                    name="absorbed.png"))
    sc.materials += [
        Material(ambient=(ka, ka, ka), diffuse=(0.7, 0.55, 0.3), specular=(0.6, 0.6, 0.6), phong_exp=30),
        Material(type=A.MAT_MIRROR, ambient=(0.05, 0.05, 0.05), diffuse=(0.1, 0.1, 0.1),
                 specular=(0.3, 0.3, 0.3), mirror=(0.8, 0.8, 0.8), phong_exp=50),
        Material(type=A.MAT_DIELECTRIC, ambient=(0, 0, 0), diffuse=(0, 0, 0), specular=(0, 0, 0),
                 refraction_index=1.5, absorption_coeff=(0, 0, 0)),
    ]
    if spheres:         # the dragon scene's: the mirror sphere sees the mesh's dark side, the glass one stands in front
        s = scenegen._add_vertices(sc, [(-1.7, -0.3, -0.3), (1.2, -0.55, 1.2)])
        sc.objects.append(Object(type=A.OBJ_SPHERE, id=1, material=2, center=s, radius=0.7))
        sc.objects.append(Object(type=A.OBJ_SPHERE, id=2, material=3, center=s + 1, radius=0.45))
    v, f = scenegen.uv_sphere(64, 32)
    b = scenegen._add_vertices(sc, v)
    sc.objects.append(Object(type=A.OBJ_MESH, id=1, material=1, faces=(f + b).astype(np.int32)))
    sc.lights.append(Light(type=A.LIGHT_POINT, **LIGHT))
    if lights == 2:
        sc.lights.append(Light(type=A.LIGHT_POINT, position=(-4, 2, 3), intensity=(9000, 9000, 9000)))
    return sc


def _oracle(sc):
    o = pyoracle.Oracle(sc)
    img = o.render(0)[0]
    c = o.ray_counts()
    o.close()
    return img, c


def _arms(sc, monkeypatch, renders=(dict(),)):
    """Per arm ("on": the default, "off": RTG_ABSORB_SKIP=0): [(frame, stats)] of each render in `renders`."""
    out = {}
    for arm in ("on", "off"):
        if arm == "off":
            monkeypatch.setenv("RTG_ABSORB_SKIP", "0")
        else:
            monkeypatch.delenv("RTG_ABSORB_SKIP", raising=False)
        with rtg.Renderer(sc, device=0) as r:
            out[arm] = []
            for kw in renders:
                img = r.render(0, **kw)
                out[arm].append((img, r.stats()))
    monkeypatch.delenv("RTG_ABSORB_SKIP", raising=False)
    return out


def _check_skips(sc, monkeypatch, renders):
    """Cases A / B: both arms bitwise the oracle's frame, fewer shadow rays with the rule, the rest as before."""
    ref, c = _oracle(sc)
    out = _arms(sc, monkeypatch, renders)
    for k, kw in enumerate(renders):
        (on, son), (off, soff) = out["on"][k], out["off"][k]
        print(f"{kw}: shadow rays on / off / oracle: {son['shadow_rays']} / {soff['shadow_rays']} / {c['shadow']}")
        assert np.array_equal(np.isnan(on), np.isnan(ref)), kw
        assert np.array_equal(_bits(on), _bits(ref)), kw
        assert np.array_equal(_bits(off), _bits(ref)), kw
        assert np.array_equal(_bits(on), _bits(off)), kw
        assert son["shadow_rays"] < soff["shadow_rays"] <= c["shadow"], kw
        for st in (son, soff):
            assert (st["primary_rays"], st["secondary_rays"]) == (c["primary"], c["secondary"]), kw
    # every schedule traces the same queries
    assert len({s["shadow_rays"] for _, s in out["on"]}) == 1
    assert len({s["shadow_rays"] for _, s in out["off"]}) == 1


def _check_same(sc, monkeypatch, ref=None, strict=True):
    """Cases C / D: the switch changes neither the frame nor (strict) the number of shadow rays."""
    out = _arms(sc, monkeypatch)
    (on, son), (off, soff) = out["on"][0], out["off"][0]
    print(f"shadow rays on / off: {son['shadow_rays']} / {soff['shadow_rays']}")
    assert np.array_equal(np.isnan(on), np.isnan(off))
    assert np.array_equal(_bits(on), _bits(off))
    if ref is not None:
        assert np.array_equal(_bits(on), _bits(ref))
    if strict:
        assert son["shadow_rays"] == soff["shadow_rays"]
    else:
        assert son["shadow_rays"] <= soff["shadow_rays"]
    for k in ("primary_rays", "secondary_rays"):
        assert son[k] == soff[k], k
    return son


def test_a_absorbed_queries_are_skipped_and_the_frame_is_the_oracles(gpu, monkeypatch):
    _check_skips(_scene(), monkeypatch, (dict(),))


def test_b_deeper_levels_and_both_schedules(gpu, monkeypatch):
    sc = _scene(spheres=True, max_depth=3)
    _check_skips(sc, monkeypatch, (dict(), dict(schedule=A.SCHEDULE_STREAM), dict(streams=1),
                                   dict(schedule=A.SCHEDULE_STREAM, streams=1)))


def test_b_progressive_frame_skips_the_same_queries(gpu, monkeypatch):
    """rtg_frame shares shade_ray: a frame added in two chunks resolves to the one-shot render's bits in both
    arms, and its chunks trace the arm's number of shadow rays between them."""
    sc = _scene(spheres=True, max_depth=3)
    got = {}
    for arm in ("on", "off"):
        if arm == "off":
            monkeypatch.setenv("RTG_ABSORB_SKIP", "0")
        else:
            monkeypatch.delenv("RTG_ABSORB_SKIP", raising=False)
        with rtg.Renderer(sc, device=0) as r:
            ref = r.render(0)
            n0 = r.stats()["shadow_rays"]
            with r.frame(0) as f:
                n = 0
                for c in (1, 3):
                    f.add(c)
                    n += r.stats()["shadow_rays"]
                img = f.resolve()
        assert np.array_equal(_bits(img), _bits(ref)), arm
        assert n == n0, arm
        got[arm] = (img, n)
    assert np.array_equal(_bits(got["on"][0]), _bits(got["off"][0]))
    assert got["on"][1] < got["off"][1]


def test_c_zero_ambient_skips_nothing_more(gpu, monkeypatch):
    """amb = +0: fl(0 + c) has the bits of +0 only for c = +0 (the rule light_sample already has) or -0."""
    sc = _scene(ka=0.0)
    ref, c = _oracle(sc)
    st = _check_same(sc, monkeypatch, ref)
    assert 0 < st["shadow_rays"] <= c["shadow"]


def test_d_two_lights_are_left_alone(gpu, monkeypatch):
    sc = _scene(lights=2)
    ref, c = _oracle(sc)
    st = _check_same(sc, monkeypatch, ref)
    assert 0 < st["shadow_rays"] <= c["shadow"]


def test_d_area_light_path_keeps_its_frame(gpu, monkeypatch):
    """cornell: one area light, the non-lean single-light path (col + add in k_shadow)."""
    _check_same(scenegen.cornell(64, 36, spp=4), monkeypatch, strict=False)


def test_d_path_tracer_is_left_alone(gpu, monkeypatch):
    _check_same(scenegen.cornell_pt(32, 18, spp=16), monkeypatch)
