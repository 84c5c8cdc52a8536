"""Rendering caller-supplied primary rays on the GPU (rtg_render_rays / rtg_render_rays_device).

Every comparison is exact, on integer views of the floats.  The yardstick is the renderer itself: a camera's
own rays (Renderer.camera_rays) rendered through render_rays must give render()'s bits, whatever the scene,
the integrator, the traversal, the schedule and the batching; scenes whose radiance depends on nothing but the
ray (point / directional lights, no rough material, a plain background, one sample) show that the array is
really read, by permuting and reshaping the ray image."""
import ctypes as C

import numpy as np
import pytest

import rtg
from rtg import _abi as A
from rtg import scenegen

pytestmark = pytest.mark.gpu

NX, NY = 67, 35        # crosses the 64-pixel tile width; a partial last band and column
PT_ALL = A.PT_IMPORTANCE | A.PT_NEE | A.PT_RUSSIAN_ROULETTE


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


SCENES = {
    "simple": lambda: scenegen.simple(NX, NY),
    "cornell_dof": lambda: scenegen.cornell(NX, NY, spp=4, dof=True),
    "cornell_blur": lambda: scenegen.cornell(NX, NY, spp=4, dof=False),      # level 0 carries ray times
    "glass_nest": lambda: scenegen.glass_nest(NX, NY, spp=1, max_depth=6),
    "bgtex1": lambda: scenegen.bgtex(NX, NY, spp=1),                         # the transposed background
    "bgtex3": lambda: scenegen.bgtex(NX, NY, spp=3),                         # a sample count that is no square
    "envmap": lambda: scenegen.envmap(NX, NY, spp=4),
    "spheres": lambda: scenegen.spheres(NX, NY, spp=2, n=64),                # the top-level BVH's instantiations
    "cornell_pt": lambda: scenegen.cornell_pt(NX, NY, spp=16, flags=PT_ALL),
    "multilight": lambda: plain_multilight(),
}


def plain_multilight():
    """scenegen.multilight without its mirror's roughness -- the one thing in it whose random draws are keyed
    by the pixel: what is left (point, directional and spot lights, a plain background, one sample) makes a
    ray's radiance a function of the ray alone."""
    sc = scenegen.multilight(NX, NY)
    for m in sc.materials:
        m.is_rough = False
    return sc


class Case:
    """A scene resident on the GPU with its camera's rays and render() image, made once per module."""

    def __init__(self, name, gpu):
        self.scene = SCENES[name]()
        self.cam = self.scene.cameras[0]
        self.r = rtg.Renderer(self.scene, device=gpu)
        self.rays = self.r.camera_rays(0)
        self.ref = self.r.render(0)
        self.ref.setflags(write=False)
        for a in self.rays:
            a.setflags(write=False)

    def render_rays(self, rays=None, **kw):
        o, d, t = rays or self.rays
        return self.r.render_rays(o, d, t, integrator=self.cam.integrator, pt_flags=self.cam.pt_flags, **kw)


@pytest.fixture(scope="module")
def cases(gpu):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, gpu)
        return made[name]

    yield get
    for c in made.values():
        c.r.close()


# ---- 1. a camera's own rays give the renderer's bits
OWN = [
    ("simple", {}), ("simple", {"traversal": 1}),
    ("cornell_dof", {}), ("cornell_dof", {"traversal": 1}),
    ("cornell_dof", {"schedule": A.SCHEDULE_PASSES}), ("cornell_dof", {"schedule": A.SCHEDULE_STREAM}),
    ("cornell_dof", {"max_batch_rays": 1000, "streams": 2}),                 # several passes on two lanes
    ("cornell_blur", {}), ("cornell_blur", {"schedule": A.SCHEDULE_STREAM, "max_batch_rays": 300}),
    ("glass_nest", {}), ("bgtex1", {}), ("bgtex3", {}), ("envmap", {}), ("spheres", {}),
    ("cornell_pt", {"schedule": A.SCHEDULE_PASSES}), ("cornell_pt", {"schedule": A.SCHEDULE_STREAM}),
    ("cornell_pt", {"schedule": A.SCHEDULE_STREAM, "segment_pixels": 200, "max_batch_rays": 1000}),
]


@pytest.mark.parametrize("name,kw", OWN, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in kw.items()) or 'default'}" for n, kw in OWN])
def test_own_rays_give_render_bits(cases, name, kw):
    c = cases(name)
    if name == "spheres":
        assert c.r.build_stats()["tlas_nodes"] > 0
    if name == "cornell_blur":
        assert len(np.unique(c.rays[2])) > 1
    ref = c.ref if not kw else c.r.render(0, **kw)
    assert same(ref, c.ref), (name, kw, "render() itself")
    ref_stats = None
    if kw:
        ref_stats = c.r.stats()
    got = c.render_rays(**kw)
    assert got.shape == (NY, NX, 3)
    assert same(got, c.ref), (name, kw)
    st = c.r.stats()
    assert st["primary_rays"] == NX * NY * c.cam.num_samples
    if ref_stats is not None:       # the same trees behind the same primary rays
        assert (st["secondary_rays"], st["shadow_rays"]) == (ref_stats["secondary_rays"], ref_stats["shadow_rays"])
    if name != "glass_nest":                     # (from its centre the nest is one colour) not vacuous
        assert len(np.unique(bits(c.ref))) > 8


# ---- 2. the rays are really read
@pytest.mark.parametrize("name", ["glass_nest", "multilight", "simple"])
def test_permuted_and_reshaped_rays(cases, name):
    c = cases(name)
    assert c.cam.num_samples == 1
    o, d, t = c.rays
    perm = np.random.Generator(np.random.PCG64(20261021)).permutation(NX * NY)
    assert (perm != np.arange(NX * NY)).any()
    po = o.reshape(-1, 3)[perm].reshape(o.shape)
    pd = d.reshape(-1, 3)[perm].reshape(d.shape)
    pt = t.reshape(-1)[perm].reshape(t.shape)
    got = c.render_rays((po, pd, pt))
    want = c.ref.reshape(-1, 3)[perm].reshape(NY, NX, 3)
    assert same(got, want), name
    if name != "glass_nest":                     # (one colour from its centre: the permutation cannot show there)
        assert not same(got, c.ref)
    # the same rays as an (nx * ny) x 1 image: the same values in that order
    flat = c.render_rays((o.reshape(1, NX * NY, 1, 3), d.reshape(1, NX * NY, 1, 3), t.reshape(1, NX * NY, 1)))
    assert same(flat, c.ref.reshape(1, NX * NY, 3)), name


# ---- 3. shards
@pytest.mark.parametrize("stride,block", [(2, 1), (2, 4), (3, 1), (3, 4)])
def test_shards(cases, stride, block):
    c = cases("cornell_dof")
    lib = c.r.lib
    for off in range(stride):
        owned = np.array([(y // block) % stride == off for y in range(NY)])
        assert owned.sum() == lib.rtg_shard_rows(NY, off, stride, block)
        img = c.render_rays(row_offset=off, row_stride=stride, row_block=block)
        assert c.r.stats()["primary_rays"] == int(owned.sum()) * NX * c.cam.num_samples
        assert same(img[owned], c.ref[owned]), (stride, block, off)
        assert not bits(img[~owned]).any(), (stride, block, off)
        comp = c.render_rays(row_offset=off, row_stride=stride, row_block=block, compact_rows=1)
        assert same(comp, c.ref[owned]), (stride, block, off, "compact")


# ---- 4. the device form
def test_device_form(cases, gpu):
    import torch
    for name in ("cornell_dof", "cornell_pt"):
        c = cases(name)
        ns = c.cam.num_samples
        o, d, t = c.rays
        host = np.concatenate([o, d, t[..., None]], axis=-1).reshape(-1, 7)
        rays = torch.from_numpy(np.ascontiguousarray(host)).to(f"cuda:{gpu}")
        keep = rays.clone()
        out = torch.full((NY, NX, 3), -7.0, dtype=torch.float32, device=f"cuda:{gpu}")
        c.r.render_rays_device(rays.data_ptr(), NX, NY, ns, out.data_ptr(), integrator=c.cam.integrator,
                               pt_flags=c.cam.pt_flags)
        assert same(out.cpu().numpy(), c.ref), name
        assert torch.equal(rays.view(torch.int32), keep.view(torch.int32)), name
        s = torch.cuda.Stream(device=gpu)
        out.fill_(-7.0)
        torch.cuda.synchronize(gpu)
        c.r.render_rays_device(rays.data_ptr(), NX, NY, ns, out.data_ptr(), stream=s.cuda_stream,
                               integrator=c.cam.integrator, pt_flags=c.cam.pt_flags)
        assert same(out.cpu().numpy(), c.ref), (name, "stream")


# ---- 5. validation
def _raw_render_rays(c, rays7, out, **kw):
    """rtg_render_rays on an (ny, nx, ns, 7) array into `out`; returns (status, message)."""
    ny, nx, ns = rays7.shape[:3]
    im = A.RayImage(nx, ny, ns, c.cam.integrator, c.cam.pt_flags)
    opt = c.r.opts(**kw)
    rc = c.r.lib.rtg_render_rays(c.r.handle, C.byref(im), rays7.ctypes.data, C.byref(opt), out.ctypes.data)
    return rc, c.r.lib.rtg_last_error().decode()


BAD = [("nan_origin", 1, np.nan), ("inf_direction", 4, np.inf), ("neg_inf_time", 6, -np.inf), ("zero_direction", None, 0.0)]


@pytest.mark.parametrize("what,col,value", BAD, ids=[b[0] for b in BAD])
def test_bad_rays_are_refused(cases, what, col, value):
    c = cases("cornell_dof")
    ns = c.cam.num_samples
    o, d, t = c.rays
    rays7 = np.ascontiguousarray(np.concatenate([o, d, t[..., None]], axis=-1))
    first = (9 * NX + 65) * ns + 2            # row 9, beyond the first 64-pixel tile
    second = (30 * NX + 3) * ns + 1
    flat = rays7.reshape(-1, 7)
    for idx in (second, first):
        if col is None:
            flat[idx, 3:6] = (0.0, -0.0, 0.0)
        else:
            flat[idx, col] = value
    out = np.full((NY, NX, 3), -7.0, np.float32)
    rc, msg = _raw_render_rays(c, rays7, out)
    assert rc == -1 and f"ray {first} " in msg, (rc, msg)
    assert (out == -7.0).all()
    with pytest.raises(rtg.RtgError, match=f"RTG_ERR_INVALID.*ray {first} "):
        c.r.render_rays(rays7[..., 0:3], rays7[..., 3:6], rays7[..., 6], integrator=c.cam.integrator, pt_flags=c.cam.pt_flags)
    # a shard that owns only the second bad ray names that one; one that owns neither renders its rows
    rc, msg = _raw_render_rays(c, rays7, out, row_offset=30 // 4 % 4, row_stride=4, row_block=4)
    assert rc == -1 and f"ray {second} " in msg, (rc, msg)
    assert (out == -7.0).all()
    off = next(k for k in range(4) if k not in (9 // 4 % 4, 30 // 4 % 4))
    rc, msg = _raw_render_rays(c, rays7, out, row_offset=off, row_stride=4, row_block=4)
    assert rc == 0, msg
    owned = np.array([(y // 4) % 4 == off for y in range(NY)])
    assert same(out[owned], c.ref[owned]) and not bits(out[~owned]).any()


def test_bad_rays_device_form(cases, gpu):
    import torch
    c = cases("simple")
    o, d, t = c.rays
    host = np.concatenate([o, d, t[..., None]], axis=-1).reshape(-1, 7).copy()
    host[1234, 5] = np.nan
    host[2000, 0] = np.inf
    rays = torch.from_numpy(host).to(f"cuda:{gpu}")
    out = torch.full((NY, NX, 3), -7.0, dtype=torch.float32, device=f"cuda:{gpu}")
    with pytest.raises(rtg.RtgError, match="RTG_ERR_INVALID.*ray 1234 "):
        c.r.render_rays_device(rays.data_ptr(), NX, NY, 1, out.data_ptr())
    assert bool((out == -7.0).all())


# ---- 6. neighbours are undisturbed
def test_neighbours_are_undisturbed(cases):
    c = cases("cornell_dof")
    before = c.r.render(0)
    with c.r.frame(0, moments=True) as fa, c.r.frame(0, moments=True) as fb:
        fa.add(2)
        fb.add(2)
        got = c.render_rays(row_offset=1, row_stride=2)          # between fb's two add() calls
        assert c.r.stats()["primary_rays"] == c.r.lib.rtg_shard_rows(NY, 1, 2, 1) * NX * c.cam.num_samples
        fb.add(2)
        fa.add(2)
        assert same(fa.resolve(), fb.resolve()) and same(fb.resolve(), c.ref)
        ma, mb = fa.moments(), fb.moments()
        assert same(ma[0], mb[0]) and same(ma[1], mb[1])
    assert same(got[1::2], c.ref[1::2])
    assert same(c.r.render(0), before) and same(before, c.ref)


# ---- 7. generated rays
def test_generated_rays(cases):
    c = cases("simple")
    o, d, t = rtg.equirect_rays((0.0, 0.2, 0.0), 32, 16, spp=3, seed=5)
    pano = c.r.render_rays(o, d, t, seed=1)
    assert pano.shape == (16, 32, 3) and np.isfinite(pano).all()
    assert len(np.unique(bits(pano))) > 4
    o, d, t = rtg.ortho_rays((0.0, 0.3, 0.0), (0, 0, -1), (0, 1, 0), 3.0, 1.5, 32, 16)
    img = c.r.render_rays(o, d, t)
    assert img.shape == (16, 32, 3) and np.isfinite(img).all()
    miss = c.r.trace(o.reshape(-1, 3), d.reshape(-1, 3), t.reshape(-1))["full"].reshape(16, 32) == 0
    assert miss.any() and (~miss).any()
    bg = np.asarray(c.scene.background, np.float32)
    assert same(img[miss], np.broadcast_to(bg, img[miss].shape))
    assert (img[~miss] != bg).any()
