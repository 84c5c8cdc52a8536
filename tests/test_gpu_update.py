"""rtg_scene_update on the GPU: after Renderer.update(B) every call gives the bits of a fresh
Renderer(B) -- renders on both schedules, both traversals and with the top-level BVH forced off and on,
feature buffers, frames added in chunks, closest-hit and occlusion queries -- and the hit records equal the
oracle's trace of B (pyoracle), so the expected values never come from the library alone.

The radius kernel (rtg_radius.hip) runs in an update for every transformed mesh entry of more than 8
triangles (kFlatMaxPrims: smaller meshes keep their records on the host); the one-mesh scenes below sweep its
wave, block and multi-block edges.  From 63 triangles on these meshes take their bounding sphere (a rotated
entry's world box is loose), so the kernel's result reaches the hash through TopObject::bs[3]."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

import pyoracle
import rtg
from rtg import _abi as A
from rtg import scenegen
from rtg.scene import Light, Material, Object, Scene

import update_cases as U

pytestmark = pytest.mark.gpu

TLAS_OFF, TLAS_ON = 1, 2
NRAYS = 2000
PASSES, STREAM = A.SCHEDULE_PASSES, A.SCHEDULE_STREAM


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def rays_for(sc, orc, n=NRAYS):
    """Rays as tests/test_gpu_queries.py draws them: half uniform in the padded vertex box, half re-shot from
    the oracle's hit points offset +-2 int_eps along the normal; times uniform in [0, 1]."""
    rng = np.random.default_rng(17)
    half = n // 2
    v = np.asarray(sc.vertices, np.float32)
    v = v[np.isfinite(v).all(axis=1)]
    lo, hi = v.min(axis=0) - 0.5, v.max(axis=0) + 0.5
    o1 = rng.uniform(lo, hi, (half, 3)).astype(np.float32)
    d1 = _unit(rng, half)
    times = rng.uniform(0, 1, n).astype(np.float32)
    h1 = orc.trace(o1, d1, times[:half])
    idx = np.flatnonzero(h1["full"] == 1)
    d2 = _unit(rng, n - half)
    if len(idx) == 0:
        o2 = rng.uniform(lo, hi, (n - half, 3)).astype(np.float32)
    else:
        idx = idx[np.arange(n - half) % len(idx)]
        sign = np.where(np.arange(n - half) % 2 == 0, np.float32(1), np.float32(-1))[:, None]
        o2 = (h1["point"][idx] + h1["normal"][idx] * (sign * np.float32(2 * sc.int_eps))).astype(np.float32)
    return np.concatenate([o1, o2]), np.concatenate([d1, d2]), times


_ORACLE = {}


def oracle_case(key, sc):
    """(origins, directions, times, oracle hits, tmax, expected occlusion) of scene `sc`, computed once per key."""
    if key not in _ORACLE:
        orc = pyoracle.Oracle(sc)
        o, d, times = rays_for(sc, orc)
        ref = orc.trace(o, d, times)
        orc.close()
        t = ref["t"].astype(np.float32)
        inf = np.float32(np.inf)
        n = len(o)
        tmax = np.choose(np.arange(n) % 4, [np.full(n, inf), np.nextafter(t, inf), t, np.float32(0.5) * t]).astype(np.float32)
        with np.errstate(invalid="ignore"):
            expected = (ref["full"] == 1) & (t < tmax)
        _ORACLE[key] = (o, d, times, ref, tmax, expected)
    return _ORACLE[key]


def same_hits(a, b):
    return all(np.array_equal(U.bits(a[k]) if a[k].dtype == np.float32 else a[k],
                              U.bits(b[k]) if b[k].dtype == np.float32 else b[k]) for k in a)


def check_queries(r, fresh, key, sc):
    """trace / occluded of the updated scene: the fresh scene's bits and the oracle's hits."""
    o, d, times, ref, tmax, expected = oracle_case(key, sc)
    for traversal in (0, 1):
        got, want = r.trace(o, d, times, traversal=traversal), fresh.trace(o, d, times, traversal=traversal)
        assert same_hits(got, want), (key, traversal)
        assert np.array_equal(got["full"], ref["full"]), (key, traversal)
        hit = ref["full"] == 1
        for k in ("object", "prim", "material"):
            assert np.array_equal(got[k][hit], ref[k][hit]), (key, traversal, k)
        for k in ("t", "point", "normal"):
            assert np.array_equal(U.bits(got[k])[hit], U.bits(ref[k])[hit]), (key, traversal, k)
        occ = r.occluded(o, d, tmax, times, traversal=traversal)
        assert np.array_equal(occ, fresh.occluded(o, d, tmax, times, traversal=traversal)), (key, traversal)
        assert np.array_equal(occ, expected), (key, traversal)


def check_images(r, fresh, key):
    for schedule in (PASSES, STREAM):
        for traversal in (0, 1):
            a, b = r.render(0, schedule=schedule, traversal=traversal), fresh.render(0, schedule=schedule, traversal=traversal)
            assert np.array_equal(U.bits(a), U.bits(b)), (key, schedule, traversal)
    fa, fb = r.aov(0), fresh.aov(0)
    for k in fa:
        assert np.array_equal(fa[k].view(np.int32), fb[k].view(np.int32)), (key, k)


def spp4(sc):
    """The scene with a 4-sample camera (frames in two chunks)."""
    sc = copy.deepcopy(sc)
    sc.cameras[0].num_samples = 4
    return sc


@pytest.mark.parametrize("tlas", [TLAS_OFF, TLAS_ON])
@pytest.mark.parametrize("name,variant", U.CASES)
def test_update_renders_as_a_fresh_scene(gpu, name, variant, tlas):
    a, b = U.pair(name, variant)
    a, b = spp4(a), spp4(b)
    with rtg.Renderer(a, device=gpu, tlas=tlas) as r, rtg.Renderer(b, device=gpu, tlas=tlas) as fresh:
        ha = r.top_hash()
        r.update(b)
        assert r.top_hash() == fresh.top_hash()
        sa, sb = r.build_stats(), fresh.build_stats()
        assert (sa["tlas_nodes"], sa["flat_group_entries"]) == (sb["tlas_nodes"], sb["flat_group_entries"])
        assert 0 < sa["upload_bytes"] < sb["upload_bytes"]
        for i in range(U.entries(b)):
            assert all(np.array_equal(U.bits(x), U.bits(y)) for x, y in zip(r.matrices(i), fresh.matrices(i)))
        key = (name, variant, tlas)
        check_images(r, fresh, key)
        with r.frame(0) as f:           # a frame made after the update, added in two chunks
            f.add(1)
            f.add(3)
            split = f.resolve()
        assert np.array_equal(U.bits(split), U.bits(fresh.render(0)))
        check_queries(r, fresh, (name, variant), b)
        r.update(a)                     # and back
        assert r.top_hash() == ha


# ---------------------------------------------------------------------------- the radius kernel
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 20480]
ON_THE_CARD = [t for t in SIZES if t > 8]      # more than kFlatMaxPrims triangles: records on the device only
AXIS = np.array([0.3, 1.0, -0.45])


def strip_mesh(T):
    """T triangles (k, k + 1, k + 2) over a Fibonacci lattice of T + 2 points of the unit sphere."""
    n = T + 2
    k = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * k / n)
    th = math.pi * (1 + 5 ** 0.5) * k
    p = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], -1)
    f = np.stack([np.arange(T), np.arange(T) + 1, np.arange(T) + 2], -1)
    return p.astype(np.float32), f


def one_mesh(T, angle_deg, nan_vertex=False):
    """One mesh of T triangles under a scale 1 : 1.1 : 0.9, a rotation about a skew axis and a translation."""
    sc = Scene(max_depth=2, background=(3, 4, 5), ambient=(10, 10, 10))
    sc.cameras.append(scenegen._cam((0.5, 0.2, 6.0), (0, 0, -1), (0, 1, 0), 8, 6, fov_deg=40, name="m.png"))
    sc.materials.append(Material(ambient=(1, 1, 1), diffuse=(0.6, 0.5, 0.4), specular=(0.3, 0.3, 0.3), phong_exp=10))
    v, f = strip_mesh(T)
    if nan_vertex:
        v[len(v) // 2, 1] = np.nan
    b = scenegen._add_vertices(sc, v)
    sc.rotations.append((float(angle_deg), float(AXIS[0]), float(AXIS[1]), float(AXIS[2])))
    sc.translations.append((0.4, -0.3, 0.2))
    sc.scalings.append((1.0, 1.1, 0.9))
    sc.objects.append(Object(type=A.OBJ_MESH, id=1, material=1, faces=(f + b).astype(np.int32),
                             xforms=[(A.XF_SCALING, 1), (A.XF_ROTATION, 1), (A.XF_TRANSLATION, 1)]))
    sc.lights.append(Light(type=A.LIGHT_POINT, position=(2, 5, 4), intensity=(9000, 9000, 9000)))
    return sc


@pytest.mark.parametrize("T", SIZES)
def test_radius_kernel_matches_the_host_pass(gpu, T):
    """Sizes 1 and 2 stay on the host (records kept); 63 ... 20480 run on the card (ON_THE_CARD)."""
    a, b = one_mesh(T, 15.0), one_mesh(T, 40.0)
    with rtg.Renderer(a, device=gpu) as r, rtg.Renderer(b, device=gpu) as fresh:
        r.update(b)
        assert r.top_hash() == fresh.top_hash(), (T, T in ON_THE_CARD)
        assert all(np.array_equal(U.bits(x), U.bits(y)) for x, y in zip(r.matrices(0), fresh.matrices(0)))
        check_images(r, fresh, T)
        check_queries(r, fresh, ("mesh", T), b)


def test_radius_kernel_propagates_nan(gpu):
    """A non-finite vertex: the maximum is NaN on either side, the entry gets no sphere, the hash is equal."""
    a, b = one_mesh(257, 15.0, nan_vertex=True), one_mesh(257, 40.0, nan_vertex=True)
    clean = one_mesh(257, 40.0)
    with rtg.Renderer(a, device=gpu) as r, rtg.Renderer(b, device=gpu) as fresh, rtg.Renderer(clean, device=gpu) as c:
        r.update(b)
        assert r.top_hash() == fresh.top_hash()
        assert r.top_hash() != c.top_hash()
        check_images(r, fresh, "nan")
        o, d, times, ref, tmax, expected = oracle_case("nan", b)
        assert same_hits(r.trace(o, d, times), fresh.trace(o, d, times))
        assert np.array_equal(r.occluded(o, d, tmax, times), fresh.occluded(o, d, tmax, times))


# ---------------------------------------------------------------------------- sequences, frames, workspaces
def _free_bytes():
    import torch

    return torch.cuda.mem_get_info()[0]         # hipMemGetInfo


def test_ten_updates_in_a_row(gpu):
    base = U.scene("cornell")
    free = []
    with rtg.Renderer(base, device=gpu) as r:
        for k in range(10):
            b = copy.deepcopy(base)
            b.rotations = [(30.0 + 13.0 * (k + 1), 0.0, 1.0, 0.1 * k)]
            r.update(b)
            img = r.render(0)
            with rtg.Renderer(b, device=gpu) as fresh:
                assert r.top_hash() == fresh.top_hash()
                assert np.array_equal(U.bits(img), U.bits(fresh.render(0))), k
            free.append(_free_bytes())
    # no growth: within one allocation granule (2 MiB) of the state after the 2nd update
    assert abs(free[9] - free[1]) <= 2 << 20, free


def test_live_frames_refuse_the_update(gpu):
    a, b = U.pair("cornell", "transforms")
    a, b = spp4(a), spp4(b)
    with rtg.Renderer(a, device=gpu) as r, rtg.Renderer(a, device=gpu) as calm:
        h = r.top_hash()
        with r.frame(0) as f, calm.frame(0) as g:
            f.add(2)
            g.add(2)
            desc, keep = b.to_desc(geometry=False)
            assert r.lib.rtg_scene_update(r.handle, C.byref(desc)) == -1
            assert b"live frames" in r.lib.rtg_last_error()
            assert r.top_hash() == h
            f.add(2)
            g.add(2)
            assert np.array_equal(U.bits(f.resolve()), U.bits(g.resolve()))
        r.update(b)                     # the frame is gone: the update succeeds
        with rtg.Renderer(b, device=gpu) as fresh:
            assert np.array_equal(U.bits(r.render(0)), U.bits(fresh.render(0)))


def test_update_leaves_the_query_workspace_alone(gpu):
    import torch

    a = U.scene("cornell")
    o, d, times, ref, tmax, expected = oracle_case(("cornell", "base"), a)
    rays = np.zeros((len(o), 7), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, d, times
    dev = torch.device(f"cuda:{gpu}")
    rays_t, tmax_t = torch.from_numpy(rays).to(dev), torch.from_numpy(tmax).to(dev)

    def occluded(r):
        out = torch.full((len(o),), 255, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        r.occluded_device(rays_t.data_ptr(), len(o), out.data_ptr(), tmax_ptr=tmax_t.data_ptr())
        return out.cpu().numpy()

    with rtg.Renderer(a, device=gpu) as r:
        before = occluded(r)
        assert np.array_equal(before, expected.astype(np.uint8))
        r.update(a)
        assert np.array_equal(occluded(r), before)


def test_light_count_changes_between_renders(gpu):
    """1 light -> 3 -> 1: the render workspace is laid out by the light count of each render."""
    one = U.scene("multilight")
    one.lights = one.lights[:1]
    three = U.scene("multilight")
    three.lights = three.lights[:3]
    with rtg.Renderer(one, device=gpu) as r, rtg.Renderer(one, device=gpu) as f1, rtg.Renderer(three, device=gpu) as f3:
        for sc, fresh in ((one, f1), (three, f3), (one, f1), (three, f3)):
            r.update(sc)
            assert r.top_hash() == fresh.top_hash()
            check_images(r, fresh, len(sc.lights))
