"""Occlusion queries and ray queries on device arrays on the GPU.

The contract: occluded[i] == (hit.full && hit.t < tmax[i]) with `hit` the closest hit of the same ray, time
and scene.  Every expected value comes from the oracle's trace (pyoracle.Oracle.trace), never from the
library under test, compared in float32.  Scenes: many spheres (the top-level BVH by default, SphereEnt),
cornell (instances, blur: ray times uniform in [0, 1]), a mesh (the BVH walk, the flat group if it forms) and
coincident entries (ties), each with the top-level BVH forced on and off.  Rays: half uniform in the scene's
padded vertex box, half re-shot from the oracle's hit points offset +-2 int_eps along the normal -- the
candidates within eps behind the origin, which separate "closest t < tmax" from "some hit below tmax".  tmax
cycles through values at, one ulp around and far from the oracle's t, and through inf / FLT_MAX / 0 / -1 / NaN."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
import rtg
from rtg import _abi as A
from rtg import scenegen
from rtg.render import hits_to_dict
from rtg.scene import Instance, Object

pytestmark = pytest.mark.gpu

TLAS_AUTO, TLAS_OFF, TLAS_ON = 0, 1, 2
N = 20000
FLT_MAX = np.finfo(np.float32).max
SIZES = [1, 63, 64, 65, 511, 512, 513, 20000, 100]


def _tie_scene():
    """Coincident entries (tests/test_gpu_tlas.py): the same sphere three times and the same mesh as an
    object and as two instances with identity transforms -- every hit is a tie broken by the loop order."""
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
    "spheres": lambda: scenegen.spheres(8, 6, spp=1, n=300),
    "cornell": lambda: scenegen.cornell(8, 6, spp=1),
    "bunny": lambda: scenegen.bunny5k(8, 6, level=2),
    "ties": _tie_scene,
}


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def make_case(name):
    """(scene, origins, directions, times or None, oracle hits, tmax, expected) of a scene: N rays."""
    sc = SCENES[name]()
    rng = np.random.default_rng(17)
    orc = pyoracle.Oracle(sc)
    half = N // 2
    v = np.asarray(sc.vertices, np.float32)
    lo, hi = v.min(axis=0) - 0.5, v.max(axis=0) + 0.5
    o1 = rng.uniform(lo, hi, (half, 3)).astype(np.float32)
    d1 = _unit(rng, half)
    times = rng.uniform(0, 1, N).astype(np.float32) if name == "cornell" else None
    h1 = orc.trace(o1, d1, None if times is None else times[:half])
    # the surface rays: from the hit points (cycled to fill the half), offset to either side of the surface
    idx = np.flatnonzero(h1["full"] == 1)
    assert len(idx) > 0
    idx = idx[np.arange(N - half) % len(idx)]
    sign = np.where(np.arange(N - half) % 2 == 0, np.float32(1), np.float32(-1))[:, None]
    o2 = (h1["point"][idx] + h1["normal"][idx] * (sign * np.float32(2 * sc.int_eps))).astype(np.float32)
    d2 = _unit(rng, N - half)
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    ref = orc.trace(o, d, times)
    orc.close()
    t = ref["t"].astype(np.float32)
    inf, nan, zero = np.float32(np.inf), np.float32(np.nan), np.float32(0)
    on_hit = [np.full(N, inf), np.full(N, FLT_MAX), np.nextafter(t, inf), np.float32(2) * t, t, np.nextafter(t, zero),
              np.float32(0.5) * t, np.full(N, zero), np.full(N, np.float32(-1)), np.full(N, nan)]
    on_miss = [np.full(N, inf), np.full(N, np.float32(1)), np.full(N, nan)]
    i = np.arange(N)
    tmax = np.where(ref["full"] == 1, np.choose(i % 10, on_hit), np.choose(i % 3, on_miss)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        expected = (ref["full"] == 1) & (t < tmax)
    return sc, o, d, times, ref, tmax, expected


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = make_case(name)
    return _CASES[name]


def _rays(o, d, times):
    r = np.zeros((len(o), 7), np.float32)
    r[:, 0:3], r[:, 3:6] = o, d
    if times is not None:
        r[:, 6] = times
    return r


def _host_hit_bytes(r, rays):
    """rtg_trace_closest's records for (n, 7) rays, as int32 (n, 11)."""
    n = len(rays)
    hits = np.zeros((n, 11), np.int32)
    A.check(r.lib.rtg_trace_closest(r.handle, rays.ctypes.data_as(C.POINTER(A.Ray)), n,
                                    hits.ctypes.data_as(C.POINTER(A.Hit)), 0), r.lib)
    return hits


class _Dev:
    """Device-form calls on torch tensors pre-filled with 255, on a stream of torch's that is not the default."""

    def __init__(self, gpu):
        import torch

        self.torch = torch
        self.dev = torch.device(f"cuda:{gpu}")
        self.stream = torch.cuda.Stream(self.dev)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def occluded(self, r, rays_t, n, tmax_t=None, traversal=0):
        out = self.torch.full((max(n, 1),), 255, dtype=self.torch.uint8, device=self.dev)
        self.torch.cuda.synchronize(self.dev)
        r.occluded_device(rays_t.data_ptr(), n, out.data_ptr(), tmax_ptr=0 if tmax_t is None else tmax_t.data_ptr(),
                          stream=self.stream.cuda_stream, traversal=traversal)
        return out.cpu().numpy()[:n]

    def closest(self, r, rays_t, n, traversal=0):
        out = self.torch.full((max(n, 1), 11), 255, dtype=self.torch.int32, device=self.dev)
        self.torch.cuda.synchronize(self.dev)
        r.trace_device(rays_t.data_ptr(), n, out.data_ptr(), stream=self.stream.cuda_stream, traversal=traversal)
        return out.cpu().numpy()[:n]


@pytest.mark.parametrize("name", list(SCENES))
def test_case_is_balanced(name):
    """At least 10 % of the queries expected occluded and at least 10 % not (the oracle alone)."""
    expected = case(name)[6]
    share = expected.mean()
    print(f"{name}: oracle hits {np.mean(case(name)[4]['full'] == 1):.3f}, expected occluded {share:.3f}")
    assert 0.10 <= share <= 0.90


@pytest.mark.parametrize("tlas", [TLAS_ON, TLAS_OFF])
@pytest.mark.parametrize("name", list(SCENES))
def test_occluded_matches_oracle(gpu, name, tlas):
    sc, o, d, times, ref, tmax, expected = case(name)
    dv = _Dev(gpu)
    rays = _rays(o, d, times)
    with rtg.Renderer(sc, device=gpu, tlas=tlas) as r:
        assert (r.build_stats()["tlas_nodes"] > 0) == (tlas == TLAS_ON)
        rays_t, tmax_t = dv.up(rays), dv.up(tmax)
        for traversal in (0, 1):
            got = r.occluded(o, d, tmax, times, traversal=traversal)
            assert got.dtype == np.bool_ and got.shape == (N,)
            bad = np.flatnonzero(got != expected)
            assert bad.size == 0, (name, tlas, traversal, bad[:8], tmax[bad[:8]], ref["t"][bad[:8]])
            every = r.occluded(o, d, None, times, traversal=traversal)
            assert np.array_equal(every, ref["full"] == 1), (name, tlas, traversal)
            # the device form on a torch stream: the host form's bytes
            dgot = dv.occluded(r, rays_t, N, tmax_t, traversal)
            assert np.array_equal(dgot, got.astype(np.uint8)), (name, tlas, traversal)
            assert np.array_equal(dv.occluded(r, rays_t, N, None, traversal), every.astype(np.uint8))
        assert np.array_equal(r.occluded(o, d, np.float32(1.5), times), (ref["full"] == 1) & (ref["t"] < np.float32(1.5)))
        # closest hits on device arrays: every byte of rtg_trace_closest's records
        host = _host_hit_bytes(r, rays)
        dhits = dv.closest(r, rays_t, N)
        assert dhits.shape == (N, 11) and np.array_equal(dhits, host), (name, tlas)
        hd, rd = hits_to_dict(dhits, N), r.trace(o, d, times)
        for k in rd:
            assert np.array_equal(hd[k].view(np.int32), rd[k].view(np.int32)), k
        assert np.array_equal(hd["full"], ref["full"]) and np.array_equal(hd["t"].view(np.int32), ref["t"].view(np.int32))


@pytest.mark.parametrize("name", list(SCENES))
def test_sizes_cross_wave_and_block_edges_and_reuse_the_workspace(gpu, name):
    """n = 1 .. 20000 .. 100 on one Renderer: the workspace grows, then is reused; each result is the
    matching prefix of the full one."""
    sc, o, d, times, ref, tmax, expected = case(name)
    dv = _Dev(gpu)
    rays = _rays(o, d, times)
    with rtg.Renderer(sc, device=gpu) as r:
        host = _host_hit_bytes(r, rays)
        rays_t, tmax_t = dv.up(rays), dv.up(tmax)
        for n in SIZES:
            assert np.array_equal(dv.occluded(r, rays_t, n, tmax_t), expected[:n].astype(np.uint8)), (name, n)
            assert np.array_equal(dv.closest(r, rays_t, n), host[:n]), (name, n)
            assert np.array_equal(r.occluded(o[:n], d[:n], tmax[:n], None if times is None else times[:n]),
                                  expected[:n]), (name, n)


def test_queries_do_not_alias_rendering(gpu):
    """A device query between two renders, and between two chunks of a frame, changes no bit of theirs."""
    sc, o, d, times, ref, tmax, expected = case("cornell")
    sc4 = scenegen.cornell(8, 6, spp=4)
    dv = _Dev(gpu)
    rays_t, tmax_t = dv.up(_rays(o, d, times)), dv.up(tmax)

    def query(r):
        assert np.array_equal(dv.occluded(r, rays_t, N, tmax_t), expected.astype(np.uint8))
        assert np.array_equal(hits_to_dict(dv.closest(r, rays_t, N), N)["full"], ref["full"])

    with rtg.Renderer(sc4, device=gpu) as r:
        before = r.render(0)
        query(r)
        after = r.render(0)
        assert np.array_equal(before.view(np.int32), after.view(np.int32))
        with r.frame(0) as f:
            f.add(4)
            whole = f.resolve()
        with r.frame(0) as f:
            f.add(2)
            query(r)
            f.add(2)
            split = f.resolve()
        assert np.array_equal(whole.view(np.int32), split.view(np.int32))


@pytest.mark.parametrize("tlas", [TLAS_ON, TLAS_OFF])
def test_nan_rays_are_not_occluded(gpu, tlas):
    sc, o, d, times, ref, tmax, expected = case("spheres")
    n = 256
    o2, d2 = o[:n].copy(), d[:n].copy()
    o2[0::4, 0] = np.nan
    d2[1::4, 2] = np.nan
    clean = np.arange(n) % 4 >= 2
    with rtg.Renderer(sc, device=gpu, tlas=tlas) as r:
        for traversal in (0, 1):
            got = r.occluded(o2, d2, None, traversal=traversal)
            assert not got[~clean].any()
            assert np.array_equal(got[clean], (ref["full"][:n] == 1)[clean])
