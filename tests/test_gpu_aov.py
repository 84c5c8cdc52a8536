"""First-hit feature buffers and camera rays on the GPU (rtg_render_aov / rtg_camera_rays).

Every comparison is exact, on integer views of the floats.  The yardstick is the oracle's `trace` on the
rays `camera_rays` returns, reduced per pixel by the contract's restatement
`s = f32(0); for k: s = f32(s + v_k); s / f32(hits)`; that the rays are the renderer's own is shown by
rebuilding an ambient-only render from one-sample windows."""
import copy
import subprocess

import numpy as np
import pytest

import rtg
from rtg import _abi as A
from rtg import native, scenegen
from rtg.scene import Light, Material, Object, Scene, Texture, parse_xml, write_xml

pytestmark = pytest.mark.gpu

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b))


def reduce_trace(tr, shape):
    """The contract restated on a trace of (ny, nx, count) rays: per pixel the in-order float32 sums of
    the hit samples' t and normal divided by float32(hits), and the first sample's ids."""
    ny, nx, cnt = shape
    full = tr["full"].reshape(ny, nx, cnt) != 0
    t = tr["t"].reshape(ny, nx, cnt)
    n = tr["normal"].reshape(ny, nx, cnt, 3)
    hits = full.sum(-1).astype(np.int32)
    sd = np.zeros((ny, nx), f32)
    sn = np.zeros((ny, nx, 3), f32)
    for k in range(cnt):
        sd = np.where(full[:, :, k], sd + t[:, :, k], sd)
        sn = np.where(full[:, :, k, None], sn + n[:, :, k], sn)
    assert sd.dtype == f32 and sn.dtype == f32
    den = np.maximum(hits, 1).astype(f32)
    hit = hits > 0
    first = full[:, :, 0]
    return {"hits": hits,
            "depth": np.where(hit, sd / den, f32(0)),
            "normal": np.where(hit[..., None], sn / den[..., None], f32(0)),
            "object": np.where(first, tr["object"].reshape(shape)[:, :, 0], -1).astype(np.int32),
            "prim": np.where(first, tr["prim"].reshape(shape)[:, :, 0], -1).astype(np.int32),
            "material": np.where(first, tr["material"].reshape(shape)[:, :, 0], 0).astype(np.int32)}


def window_of(tr, shape, first, count):
    """The trace of the sub-window [first, first + count) of a trace over `shape` rays."""
    return {k: v.reshape(shape + v.shape[1:])[:, :, first:first + count].reshape((-1,) + v.shape[1:])
            for k, v in tr.items()}


KEYS = ("hits", "depth", "normal", "object", "prim", "material")

ORACLE_CASES = [
    ("simple", lambda: scenegen.simple(24, 16), 0, [(0, 0)]),
    ("bunny", lambda: scenegen.bunny5k(67, 45, level=2), 0, [(0, 0)]),
    ("bunny_exhaustive", lambda: scenegen.bunny5k(67, 45, level=2), 1, [(0, 0)]),
    ("textured", lambda: scenegen.textured(48, 36, spp=4), 0, [(0, 0), (1, 2), (3, 1)]),
    ("cornell_dof", lambda: scenegen.cornell(48, 27, spp=4, dof=True), 0, [(0, 0)]),
    ("cornell", lambda: scenegen.cornell(48, 27, spp=4, dof=False), 0, [(0, 0)]),
    ("spheres_tlas", lambda: scenegen.spheres(48, 27, spp=4, n=64), 0, [(0, 0)]),
]


@pytest.mark.parametrize("name,make,traversal,windows", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_against_the_oracle(gpu, name, make, traversal, windows):
    import pyoracle
    sc = make()
    cam = sc.cameras[0]
    total = cam.num_samples
    shape = (cam.ny, cam.nx, total)
    with rtg.Renderer(sc, device=gpu) as r:
        if name == "spheres_tlas":
            assert r.build_stats()["tlas_nodes"] > 0
        o, d, t = r.camera_rays(0)
        assert o.shape == shape + (3,) and d.shape == shape + (3,) and t.shape == shape
        orc = pyoracle.Oracle(sc)
        ref = orc.trace(o.reshape(-1, 3), d.reshape(-1, 3), t.reshape(-1))
        orc.close()
        own = r.trace(o.reshape(-1, 3), d.reshape(-1, 3), t.reshape(-1), traversal=traversal)
        for first, count in windows:
            n = count or total - first
            want = reduce_trace(window_of(ref, shape, first, n), (cam.ny, cam.nx, n))
            mine = reduce_trace(window_of(own, shape, first, n), (cam.ny, cam.nx, n))
            got = r.aov(0, first_sample=first, sample_count=count, traversal=traversal)
            for k in KEYS:
                assert same(got[k], want[k]), (name, first, count, k)
                assert same(got[k], mine[k]), (name, first, count, k, "Renderer.trace")
            if (first, count) != (0, 0):       # a window's rays are the full call's
                wo, wd, wt = r.camera_rays(0, first_sample=first, sample_count=count)
                assert same(wo, o[:, :, first:first + n]) and same(wd, d[:, :, first:first + n])
                assert same(wt, t[:, :, first:first + n])
                continue
            # not vacuous: hit pixels, miss pixels and, with several samples, a silhouette pixel
            assert (want["hits"] == n).any() and (want["hits"] == 0).any()
            assert (want["object"] >= 0).any() and (want["object"] == -1).any()
            if total > 1:
                assert ((want["hits"] > 0) & (want["hits"] < n)).any()
        if total > 1 and not cam.is_dof:
            assert len(np.unique(t)) > 1        # ray times
        else:
            assert not t.any()


def ambient_only(sc):
    """No lights, every material plain with its own non-dyadic ambient: a hit sample's colour is exactly
    fl(ambientLight * ka) of its material."""
    sc = copy.deepcopy(sc)
    sc.lights = []
    for k, m in enumerate(sc.materials):
        m.type, m.brdf, m.is_rough = A.MAT_NORMAL, A.BRDF_NONE, False
        m.ambient = (0.1 + 0.07 * k, 0.15 + 0.07 * k, 0.2 + 0.07 * k)
    return sc


@pytest.mark.parametrize("name,make", [("cornell", lambda: scenegen.cornell(48, 27, spp=4)),
                                       ("simple", lambda: scenegen.simple(24, 16))])
def test_the_rays_are_the_renderers(gpu, name, make):
    """An ambient-only render rebuilt in numpy from one-sample windows' material ids equals
    Renderer.render (and the oracle) bit for bit: a camera-ray difference at any silhouette pixel
    would change a bit."""
    import pyoracle
    sc = ambient_only(make())
    cam = sc.cameras[0]
    n = cam.num_samples
    amb = np.asarray(sc.ambient, f32)
    colours = np.stack([amb * np.asarray(m.ambient, f32) for m in sc.materials])       # fl(ambientLight * ka)
    assert colours.dtype == f32 and len({tuple(c) for c in colours}) == len(colours)
    back = np.asarray(sc.background, f32)
    with rtg.Renderer(sc, device=gpu) as r:
        img = r.render(0)
        s = np.zeros((cam.ny, cam.nx, 3), f32)
        mixed = np.zeros((cam.ny, cam.nx), bool)
        prev = None
        for k in range(n):
            mat = r.aov(0, first_sample=k, sample_count=1)["material"]
            s = s + np.where((mat > 0)[..., None], colours[np.maximum(mat, 1) - 1], back)
            if prev is not None:
                mixed |= mat != prev
            prev = mat
        assert s.dtype == f32
        rebuilt = s / f32(n)
    assert same(rebuilt, img)
    orc = pyoracle.Oracle(sc)
    ref = orc.render(0)[0]
    orc.close()
    assert same(img, ref)
    assert (prev > 0).any() and (prev == 0).any()
    if n > 1:
        assert mixed.any()          # pixels whose samples see different materials


def test_albedo_untextured(gpu):
    sc = scenegen.multilight(40, 30)
    with rtg.Renderer(sc, device=gpu) as r:
        a = r.aov(0)
    kd = np.stack([np.asarray(m.diffuse, f32) for m in sc.materials])
    hit = a["hits"] == 1
    assert hit.any() and (~hit).any() and len(np.unique(a["material"][hit])) >= 4
    want = np.where(hit[..., None], kd[np.maximum(a["material"], 1) - 1], f32(0))
    assert same(a["albedo"], want)


KD = (0.3, 0.55, 0.7)


def decal_scene(decal, interp, normalizer, nx=40, ny=30):
    """One image texture on a sphere and on a two-triangle mesh, 1 spp."""
    rng = np.random.default_rng(17)
    sc = Scene(max_depth=1, background=(3, 4, 5), ambient=(20, 20, 20))
    sc.cameras.append(scenegen._cam((0, 1.2, 4), (0, -0.25, -1), (0, 1, 0), nx, ny, fov_deg=50, name="decal.png"))
    sc.textures.append(Texture(kind=A.TEX_IMAGE, decal=decal, interp=interp, normalizer=normalizer,
                               texels=rng.uniform(1, 255, (12, 16, 3)).astype(f32), image_id=1))
    sc.materials.append(Material(ambient=(1, 1, 1), diffuse=KD, specular=(0.3, 0.3, 0.3), phong_exp=10))
    c = scenegen._add_vertices(sc, [(0.0, 0.7, -0.5)])
    sc.objects.append(Object(type=A.OBJ_SPHERE, id=1, material=1, center=c, radius=0.7, textures=[1]))
    fl = scenegen._add_vertices(sc, [(-2, 0, 2), (2, 0, 2), (2, 0, -3), (-2, 0, -3)])
    sc.texcoords = np.array([(0, 0), (2, 0), (2, 2), (0, 2)], f32)
    sc.objects.append(Object(type=A.OBJ_MESH, id=1, material=1, textures=[1],
                             faces=np.array([[fl, fl + 1, fl + 2], [fl, fl + 2, fl + 3]], np.int32),
                             texture_offset=-(fl - 1)))
    sc.images = ["decal.ppm"]
    sc.lights.append(Light(type=A.LIGHT_POINT, position=(1, 5, 3), intensity=(20000, 20000, 20000)))
    return sc


@pytest.mark.parametrize("normalizer", [255, 1])
@pytest.mark.parametrize("interp", [A.INTERP_NN, A.INTERP_BILINEAR], ids=["nn", "bilinear"])
def test_albedo_textured(gpu, interp, normalizer):
    """replace_all renders the texture colour itself (bit-exact against the oracle elsewhere), so the albedo
    is that colour over the normalizer; replace_kd shares it; blend_kd averages it with kd."""
    with rtg.Renderer(decal_scene(A.DECAL_REPLACE_ALL, interp, normalizer), device=gpu) as r:
        img = r.render(0)
        a_all = r.aov(0)
    hit = a_all["hits"] == 1
    assert set(np.unique(a_all["object"])) == {-1, 0, 1}
    tc_over_tn = img / f32(normalizer)
    assert tc_over_tn.dtype == f32
    want = np.where(hit[..., None], tc_over_tn, f32(0))
    assert same(a_all["albedo"], want)
    assert len(np.unique(bits(want[hit]))) > 50          # a varied texture, not one colour
    with rtg.Renderer(decal_scene(A.DECAL_REPLACE_KD, interp, normalizer), device=gpu) as r:
        a_kd = r.aov(0)
    assert same(a_kd["albedo"], a_all["albedo"]) and same(a_kd["hits"], a_all["hits"])
    with rtg.Renderer(decal_scene(A.DECAL_BLEND_KD, interp, normalizer), device=gpu) as r:
        a_blend = r.aov(0)
    blend = (np.asarray(KD, f32) + want) * f32(0.5)
    assert blend.dtype == f32
    assert same(a_blend["albedo"], np.where(hit[..., None], blend, f32(0)))


def test_albedo_perlin_replace_kd(gpu):
    sc = scenegen.textured(48, 36, spp=1)
    with rtg.Renderer(sc, device=gpu) as r:
        a = r.aov(0)
    on = a["object"] == 5                     # the sphere with the Perlin replace_kd texture
    assert on.sum() > 10
    alb = a["albedo"][on]
    assert same(alb[:, 0], alb[:, 1]) and same(alb[:, 0], alb[:, 2])
    kd = np.asarray(sc.materials[sc.objects[5].material - 1].diffuse, f32)
    assert (alb != kd).any(axis=1).all()
    assert len(np.unique(bits(alb[:, 0]))) > 5


@pytest.fixture(scope="module")
def bunny(gpu):
    sc = scenegen.bunny5k(67, 45, level=2)
    with rtg.Renderer(sc, device=gpu) as r:
        yield r, r.aov(0)


ALL = ("hits", "depth", "normal", "albedo", "object", "prim", "material")


@pytest.mark.parametrize("offset", [0, 1, 2])
def test_shards_and_layout(bunny, offset):
    r, full = bunny
    cam = r.scene.cameras[0]
    owned = np.array([(y // 4) % 3 == offset for y in range(cam.ny)])
    assert 0 < owned.sum() < cam.ny
    part = r.aov(0, row_offset=offset, row_stride=3, row_block=4)
    comp = r.aov(0, row_offset=offset, row_stride=3, row_block=4, compact_rows=1)
    assert r.stats()["primary_rays"] == r.stats()["total_rays"] == int(owned.sum()) * cam.nx
    for k in ALL:
        assert same(part[k][owned], full[k][owned]), k
        blank = {"object": -1, "prim": -1}.get(k, 0)
        assert (part[k][~owned] == blank).all() and same(part[k][~owned], np.full_like(part[k][~owned], blank)), k
        assert same(comp[k], full[k][owned]), k


def test_single_buffers(bunny):
    """Each buffer alone, the others NULL, holds the same bits."""
    r, full = bunny
    cam = r.scene.cameras[0]
    cd, o, ao = cam.desc(), r.opts(), A.AovOpts()
    ids = np.stack([full["object"], full["prim"], full["material"]], -1)
    for field, ref in (("hits", full["hits"]), ("depth", full["depth"]), ("normal", full["normal"]),
                       ("albedo", full["albedo"]), ("ids", ids)):
        out = np.full(ref.shape, 77, ref.dtype)
        b = A.AovBuffers()
        setattr(b, field, out.ctypes.data_as(A.PI if ref.dtype == np.int32 else A.PF))
        A.check(r.lib.rtg_render_aov(r.handle, cd, o, ao, b), r.lib)
        assert same(out, ref), field


def test_independent_of_scheduling_options(gpu):
    sc = scenegen.cornell(48, 27, spp=4)
    cam = sc.cameras[0]
    with rtg.Renderer(sc, device=gpu) as r:
        base = r.aov(0)
        st = r.stats()
        assert st["primary_rays"] == st["total_rays"] == cam.nx * cam.ny * 4 and st["render_ms"] > 0
        assert st["secondary_rays"] == st["shadow_rays"] == 0
        for kw in ({"streams": 1}, {"streams": 3}, {"schedule": A.SCHEDULE_PASSES}, {"schedule": A.SCHEDULE_STREAM},
                   {"max_batch_rays": 1000}, {"tile_band": 2}, {"collect_stats": 1, "collect_timing": 1}):
            other = r.aov(0, **kw)
            for k in ALL:
                assert same(other[k], base[k]), (kw, k)
        r.aov(0, first_sample=1, sample_count=2)
        assert r.stats()["primary_rays"] == cam.nx * cam.ny * 2
        assert not same(r.aov(0, seed=1)["depth"], base["depth"])          # the seed is honoured


def test_several_passes(gpu):
    """A frame of more than 8M sample slots is traced in several passes (pixel ranges); its buffers equal
    the restatement over the one-sample windows, each of which is a single pass."""
    sc = scenegen.simple(1024, 1024)
    sc.cameras[0].num_samples = 9
    with rtg.Renderer(sc, device=gpu) as r:
        full = r.aov(0)
        assert r.stats()["passes"] > 1 and r.stats()["primary_rays"] == 9 << 20
        hits = np.zeros((1024, 1024), np.int32)
        sums = {k: np.zeros(full[k].shape, f32) for k in ("depth", "normal", "albedo")}
        for k in range(9):
            one = r.aov(0, first_sample=k, sample_count=1)
            assert r.stats()["passes"] == 1
            if k == 0:
                for key in ("object", "prim", "material"):
                    assert same(one[key], full[key]), key
            hit = one["hits"] == 1
            hits += hit
            for key, s in sums.items():
                m = hit if s.ndim == 2 else hit[..., None]
                sums[key] = np.where(m, s + one[key], s)
    assert same(hits, full["hits"]) and ((hits > 0) & (hits < 9)).any()
    den = np.maximum(hits, 1).astype(f32)
    for key, s in sums.items():
        d, any_hit = (den, hits > 0) if s.ndim == 2 else (den[..., None], (hits > 0)[..., None])
        assert same(np.where(any_hit, s / d, f32(0)), full[key]), key


def test_leaves_a_live_frame_alone(gpu):
    sc = scenegen.cornell(48, 27, spp=4)
    with rtg.Renderer(sc, device=gpu) as r:
        with r.frame(0) as f:
            f.add(2)
            f.add(2)
            undisturbed = f.resolve()
        with r.frame(0) as f:
            f.add(2)
            before = f.state()["sums"]
            a = r.aov(0)
            assert same(f.state()["sums"], before) and f.samples_done == 2
            f.add(2)
            assert same(f.resolve(), undisturbed)
        assert same(undisturbed, r.render(0))
        assert same(r.aov(0)["depth"], a["depth"])


def test_cli_aov_files(gpu, tmp_path):
    """rtg_cli --aov writes three more files per camera, byte-identical to rtg.render_scene(aov=True), and
    leaves the camera's own image as a run without --aov writes it."""
    sc = scenegen.cornell(32, 24, spp=4)
    sc.cameras[0].image_name = "a.png"
    second = copy.deepcopy(sc.cameras[0])
    second.image_name, second.num_samples = "b.exr", 1
    sc.cameras.append(second)
    xml = write_xml(sc, str(tmp_path / "aov.xml"))
    dirs = {k: tmp_path / k for k in ("cli", "plain", "py")}
    for d in dirs.values():
        d.mkdir()
    p = subprocess.run([native.CLI_PATH, xml, "--aov", "--out-dir", str(dirs["cli"]), "--device", str(gpu)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([native.CLI_PATH, xml, "--out-dir", str(dirs["plain"]), "--device", str(gpu)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    written = rtg.render_scene(parse_xml(xml), out_dir=str(dirs["py"]), device=gpu, aov=True)
    names = ["a.png", "a_normal.png", "a_albedo.png", "a_depth.png", "b.exr", "b_normal.exr", "b_albedo.exr", "b_depth.exr"]
    assert sorted(x.name for x in dirs["cli"].iterdir()) == sorted(names)
    assert sorted(x.name for x in dirs["py"].iterdir()) == sorted(names) and len(written) == len(names)
    assert sorted(x.name for x in dirs["plain"].iterdir()) == ["a.png", "b.exr"]
    for n in names:
        assert (dirs["cli"] / n).read_bytes() == (dirs["py"] / n).read_bytes(), n
    for n in ("a.png", "b.exr"):
        assert (dirs["cli"] / n).read_bytes() == (dirs["plain"] / n).read_bytes(), n
    assert len({(dirs["cli"] / n).read_bytes() for n in names}) == len(names)
