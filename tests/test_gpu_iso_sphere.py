"""Rays born inside an isolated glass sphere (round 7).  Two designs were built for them:

* the child split, kept: k_shade queues a block's refracted children before its reflected ones, so the
  rays inside the sphere fill whole waves of the next level instead of sharing every wave with the rays
  outside it (shade_ray, SceneView::child_split; RTG_CHILD_SPLIT=0 at scene creation restores the pairs);
* a pre-pass of closest_hit that let a ray inside a sphere certified as isolated skip the flat group and
  the object loop: measured and dropped (profiles/ab_iso_sphere.jsonl).

The scenes and ray sets below were written for the pre-pass -- origins at the centre, on both sides of
its inside margin (2^-10 R), on the surface and just outside; directions general, axis-aligned, with a
zero / negative-zero / denormal / 1e-6 component, |d| = 1e-3 and 1e3, aimed at the floor, the mesh and
the other sphere -- and stay as the check that nothing changes for such rays: every hit record and
every frame equals the oracle's bit for bit, with the children queued either way."""
import numpy as np
import pytest

import pyoracle
import rtg
from rtg import _abi as A
from rtg import scenegen
from rtg.scene import Instance, Object

pytestmark = pytest.mark.gpu

GC = np.float32([1.0, -0.3, 0.8])      # the glass sphere
GR = np.float32(0.4)
FLOOR_Y = -0.75                        # 0.05 below it
MC = np.float32([0.0, 0.0, 0.0])       # the mesh (after its translation)
SC2 = np.float32([-1.2, -0.2, 0.5])    # the second sphere
SR2 = np.float32(0.5)
MARGIN = 2.0 ** -10                    # the dropped pre-pass's: inside meant |o - c|^2 < (R (1 - 2^-10))^2


def _bits(a):
    return np.nan_to_num(np.ascontiguousarray(a, np.float32)).view(np.int32)


def _scene(nx=64, ny=48, spp=4, floor_y=FLOOR_Y, second=(SC2, SR2), second_blur=(0.0, 0.0, 0.0), rotated=False,
           cam=((0.2, 0.5, 3.4), (0.1, -0.2, -1.0), 50)):
    """A glass sphere 0.05 above a floor quad, a displaced icosphere (320 triangles, translated: it gets a
    world box, whose corner reaches into the glass sphere's ball, and a bounding sphere, which does not)
    and a second, mirror sphere; Whitted depth 6."""
    sc = scenegen.bunny5k(nx, ny, level=2, spp=spp)
    sc.cameras[0] = scenegen._cam(cam[0], cam[1], (0, 1, 0), nx, ny, fov_deg=cam[2], spp=spp, name="iso.png")
    sc.objects = []
    sc.vertices = np.zeros((0, 3), np.float32)
    v, f = scenegen.icosphere(2)
    disp = 1.0 + 0.03 * scenegen._perlin3(v + 2.0, 7)
    b = scenegen._add_vertices(sc, v * disp[:, None] * 0.75 - np.array([0.5, 0.25, -0.125]))
    c = scenegen._add_vertices(sc, [tuple(GC), tuple(second[0])])
    fl = scenegen._add_vertices(sc, [(-6, floor_y, 6), (6, floor_y, 6), (6, floor_y, -6), (-6, floor_y, -6)])
    sc.translations += [(0.5, 0.25, -0.125)]
    sc.objects.append(Object(type=A.OBJ_SPHERE, id=1, material=3, center=c, radius=float(GR)))
    sc.objects.append(Object(type=A.OBJ_MESH, id=1, material=1, faces=(f + b).astype(np.int32),
                             xforms=[(A.XF_TRANSLATION, len(sc.translations))]))
    sc.objects.append(Object(type=A.OBJ_MESH, id=2, material=2,
                             faces=np.array([[fl, fl + 1, fl + 2], [fl, fl + 2, fl + 3]], np.int32)))
    sc.objects.append(Object(type=A.OBJ_SPHERE, id=2, material=2, center=c + 1, radius=float(second[1]),
                             blur=second_blur))
    if rotated:
        sc.translations += [(-2.5, 0.6, -2.0)]
        sc.rotations += [(30.0, 0.0, 1.0, 0.0)]
        sc.instances.append(Instance(base_object=1, id=3, material=1, reset_transform=True,
                                     xforms=[(A.XF_ROTATION, len(sc.rotations)),
                                             (A.XF_TRANSLATION, len(sc.translations))]))
    return sc


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rays():
    """Origins x directions around the glass sphere (float32), and per ray the origin's class."""
    rng = np.random.default_rng(795)
    R = float(GR)
    rin = R * (1.0 - MARGIN)
    radii = [("centre", 0.0, 1), ("interior", None, 10), ("born", R - 0.002, 6),
             ("in_margin", rin * (1.0 - 1e-4), 6), ("out_margin", rin * (1.0 + 1e-4), 6),
             ("surface", R, 4), ("outside", R * (1.0 + 1e-3), 4)]
    org, cls = [], []
    for name, r, k in radii:
        for _ in range(k):
            u = _unit(rng.standard_normal(3))
            rr = rng.uniform(0.05, 0.97) * R if r is None else r
            org.append(GC.astype(np.float64) + u * rr)
            cls.append(name)
    org = np.float32(org)
    def general():                      # (a leading component of at least 0.1: gett() is well conditioned)
        while True:
            u = _unit(rng.standard_normal(3))
            if abs(u[0]) >= 0.1:
                return u

    # general directions, |d| = 1e-3 and 1e3, axis-aligned: an inside origin's run of these fills whole waves
    dirs = [general() for _ in range(112)]
    dirs += [general() * 1e-3 for _ in range(8)]
    dirs += [general() * 1e3 for _ in range(8)]
    dirs += [s * np.eye(3)[k] for k in range(3) for s in (1.0, -1.0)]
    for k in range(3):                                                              # one component special
        for special in (0.0, -0.0, 1e-40, -1e-40, 1e-6, -1e-6):
            for _ in range(3):
                d = _unit(rng.standard_normal(3))
                d[k] = special if abs(special) != 1e-6 else special * np.abs(d).max()
                dirs.append(d)
    dirs = [np.asarray(d, np.float64) for d in dirs]
    o = np.repeat(org, len(dirs), axis=0)
    d = np.tile(np.float32(dirs), (len(org), 1))
    c = np.repeat(np.array(cls), len(dirs))
    # per origin: at the floor, at the mesh and at the other sphere (with a little scatter)
    aim_o, aim_d, aim_c = [], [], []
    for p, name in zip(org, cls):
        for tgt, spread in ((np.float64([p[0], FLOOR_Y, p[2]]), np.float64([0.15, 0.0, 0.15])),
                            (MC.astype(np.float64), 0.15), (SC2.astype(np.float64), 0.15)):
            for _ in range(4):
                t = tgt + rng.normal(0, 1, 3) * spread
                aim_o.append(p)
                aim_d.append(_unit(t - p))
                aim_c.append(name)
    o = np.concatenate([o, np.float32(aim_o)])
    d = np.concatenate([d, np.float32(aim_d)])
    c = np.concatenate([c, np.array(aim_c)])
    # half in random order (mixed waves), half as generated (an origin's rays fill whole waves)
    perm = np.concatenate([rng.permutation(len(o)), np.arange(len(o))])
    return np.ascontiguousarray(o[perm]), np.ascontiguousarray(d[perm]), c[perm]


@pytest.fixture(scope="module")
def rays():
    return _rays()


def _assert_hits_equal(h, ref, what=""):
    for k in ("full", "object", "prim", "material"):
        assert np.array_equal(h[k], ref[k]), (what, k)
    m = ref["full"] == 1
    for k in ("t", "point", "normal"):
        assert np.array_equal(h[k][m].view(np.int32), ref[k][m].view(np.int32)), (what, k)


def test_rays_around_the_glass_sphere_match_oracle(gpu, rays):
    o, d, cls = rays
    sc = _scene()
    ref = pyoracle.Oracle(sc).trace(o, d)
    # what the ray set holds, by the oracle's own results: origins inside the sphere by the margin whose
    # hit is the sphere's far side (entry 0), inside ones with no such hit (a denormal leading component:
    # gett() <= 0), origins outside the margin, and hits on every other entry
    oc = o - GC
    q = (oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2]
    inside = q < np.float32((float(GR) * (1.0 - MARGIN)) ** 2)
    won = (ref["full"] == 1) & (ref["object"] == 0)
    assert (inside & won).sum() >= 1000 and (inside & ~won).sum() >= 50 and (~inside & won).sum() >= 200
    for name in ("centre", "interior", "born", "in_margin"):
        assert (inside & won & (cls == name)).any(), name
    for name in ("out_margin", "surface", "outside"):
        assert not (inside & (cls == name)).any(), name
    # whole waves of such rays and waves that mix them with others
    k = inside & won
    w = k[: len(k) // 64 * 64].reshape(-1, 64).sum(1)
    assert (w == 64).sum() >= 4 and ((w > 0) & (w < 64)).sum() >= 20
    hit_other = (ref["full"] == 1) & (ref["object"] != 0)
    assert set(np.unique(ref["object"][hit_other])) >= {1, 2, 3}       # mesh, floor and second sphere are reached
    with rtg.Renderer(sc, device=0) as r:
        h = r.trace(o, d)
    _assert_hits_equal(h, ref)


# the scenes in which the dropped pre-pass had to find no certificate
VARIANTS = {
    "floor_touches": lambda: _scene(floor_y=float(GC[1] - GR)),
    "sphere_overlaps": lambda: _scene(second=(GC + np.float32([0.6, 0.1, 0.0]), np.float32(0.3))),
    "glass_nest": lambda: scenegen.glass_nest(64, 48, spp=4),
    "rotated_instance": lambda: _scene(rotated=True),
    "blurred_sphere": lambda: _scene(second_blur=(0.3, 0.1, 0.0)),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_scene_variants_match_oracle(gpu, rays, name):
    sc = VARIANTS[name]()
    o, d, _ = rays
    if name == "glass_nest":            # its spheres are centred on the origin
        o = ((o - GC) * np.float32(4.9)).astype(np.float32)
    t = np.random.default_rng(3).random(len(o)).astype(np.float32)
    orc = pyoracle.Oracle(sc)
    ref_img = orc.render(0)[0]
    ref = orc.trace(o, d, t)
    with rtg.Renderer(sc, device=0) as r:
        img = r.render(0)
        h = r.trace(o, d, t)
    assert np.array_equal(np.isnan(img), np.isnan(ref_img))
    assert np.array_equal(_bits(img), _bits(ref_img)), name
    _assert_hits_equal(h, ref, name)


def test_close_up_frame_is_the_same_with_the_children_split_or_paired(gpu, monkeypatch):
    sc = _scene(cam=((1.05, -0.2, 1.7), (-0.05, -0.1, -0.9), 45))       # the glass sphere fills most of the view
    ref = pyoracle.Oracle(sc).render(0)[0]
    glass = pyoracle.Oracle(sc).trace(*_camera_rays(sc))
    assert np.mean((glass["full"] == 1) & (glass["object"] == 0)) > 0.5
    out = {}
    for mode in ("split", "paired"):
        if mode == "paired":
            monkeypatch.setenv("RTG_CHILD_SPLIT", "0")
        else:
            monkeypatch.delenv("RTG_CHILD_SPLIT", raising=False)
        with rtg.Renderer(sc, device=0) as r:
            img = r.render(0)
            r.render(0, collect_stats=1)
            out[mode] = (img, r.stats())
    assert np.array_equal(_bits(out["split"][0]), _bits(ref))
    assert np.array_equal(_bits(out["paired"][0]), _bits(out["split"][0]))
    a, b = out["split"][1], out["paired"][1]
    for k in ("primary_rays", "secondary_rays", "shadow_rays", "trace_steps", "trace_entry_visits"):
        assert a[k] == b[k], k
    # the same rays do the same work; split, fewer waves hold both a ray that walks the mesh and rays that
    # only cross the sphere, so the waves run fewer node steps in all (64 x each wave's longest walk).
    # This keeps the test from passing with the split never taken.
    print("trace_lane_slots split / paired:", a["trace_lane_slots"], b["trace_lane_slots"])
    assert a["trace_lane_slots"] < b["trace_lane_slots"]


def _camera_rays(sc):
    """Pixel-centre rays of camera 0 (Camera::getPrimaryRay), to check what the view shows."""
    cam = sc.cameras[0]
    pos, gaze, up = (np.asarray(x, np.float64) for x in (cam.position, cam.gaze, cam.up))
    gaze = gaze / np.linalg.norm(gaze)
    right = np.cross(gaze, up)
    right /= np.linalg.norm(right)
    upv = np.cross(right, gaze)
    l, r, b, t = cam.near_plane
    x, y = np.meshgrid(np.arange(cam.nx) + 0.5, np.arange(cam.ny) + 0.5)
    u = l + (r - l) * x / cam.nx
    v = t - (t - b) * y / cam.ny
    m = pos + gaze * cam.near_distance + u[..., None] * right + v[..., None] * upv
    d = (m - pos).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(np.float32(pos), (len(d), 1)), np.float32(d)
