"""Texturing on the GPU against the oracle, over tests/texture_cases.py: every decal on spheres, flat and
smooth meshes and standalone triangles; scaled, rotated, translated, instanced and motion-blurred entries;
textures of mixed sizes down to 1 x 1; one-light scenes (lean shadow records, the absorbed-term rule);
rays at the sphere poles, the u seam and texel boundaries.

Frames meet the project's bar (NaN masks equal, L-inf < 1e-3 on the 0..255 framebuffer); hit records are
compared bit for bit, NaN normals (sphere poles: acos of a ratio one ulp over 1; zero UV determinants) by
their masks."""
import copy
import functools

import numpy as np
import pytest

import pyoracle
import rtg
import texture_cases as tc
from rtg import _abi as A

pytestmark = pytest.mark.gpu

TOL = 1e-3          # test_gpu_parity.py's bar
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _cmp(img, ref):
    d = np.abs(img.astype(np.float64) - ref.astype(np.float64))
    nan_mismatch = int(np.sum(np.isnan(img) != np.isnan(ref)))
    d = np.where(np.isnan(d), 0.0, d)
    return float(d.max()), float((d > 0).mean()), nan_mismatch


def same_frame(a, b):
    return bool(np.array_equal(np.isnan(a), np.isnan(b))) and \
        bool(np.array_equal(bits(np.nan_to_num(a)), bits(np.nan_to_num(b))))


FRAMES = {}
for _set in tc.SIZE_SETS:
    for _one in (False, True):
        for _blur in (False, True):
            for _spp in (1, 3):
                FRAMES[f"tex_{_set}{'_one' if _one else ''}{'_blur' if _blur else ''}_{_spp}spp"] = \
                    functools.partial(tc.tex_matrix, tc.SIZE_SETS[_set], one_light=_one, blur=_blur, spp=_spp)
for _spp in (1, 3):
    FRAMES[f"tri_{_spp}spp"] = functools.partial(tc.tri_matrix, spp=_spp)
    FRAMES[f"degenerate_{_spp}spp"] = functools.partial(tc.degenerate_uv, spp=_spp)


@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_matches_oracle(gpu, name):
    sc = FRAMES[name]()
    with rtg.Renderer(sc, device=gpu) as r:
        img = r.render(0)
        st = r.stats()
    o = pyoracle.Oracle(sc)
    ref, obj, _, _ = o.render(0)
    counts = o.ray_counts()
    o.close()
    linf, frac, nanm = _cmp(img, ref)
    print(f"{name}: Linf={linf:.3g} differing={frac:.2e} nan_mismatch={nanm} "
          f"shadow={st['shadow_rays']}/{counts['shadow']}")
    assert len(np.unique(obj[obj >= 0])) >= 2 and (obj < 0).any()       # entries and background in view
    assert nanm == 0
    assert linf < TOL
    if len(sc.lights) == 1:
        assert 0 < st["shadow_rays"] <= counts["shadow"]


SCHEDULED = {"tex_mixed_blur": functools.partial(tc.tex_matrix, tc.SIZE_SETS["mixed"], blur=True, spp=2),
             "tri": functools.partial(tc.tri_matrix, spp=2)}


@pytest.mark.parametrize("name", list(SCHEDULED))
def test_stream_schedule_equals_passes(gpu, name):
    sc = SCHEDULED[name]()
    with rtg.Renderer(sc, device=gpu) as r:
        a = r.render(0, schedule=A.SCHEDULE_PASSES)
        b = r.render(0, schedule=A.SCHEDULE_STREAM)
    assert same_frame(a, b)
    assert len(np.unique(bits(a))) > 100


@pytest.mark.parametrize("flags", [A.PT_IMPORTANCE | A.PT_NEE | A.PT_RUSSIAN_ROULETTE, 0], ids=["INR", "plain"])
@pytest.mark.parametrize("name", list(SCHEDULED))
def test_path_traced_frame_matches_oracle(gpu, name, flags):
    sc = SCHEDULED[name]()
    cam = sc.cameras[0]
    cam.integrator, cam.pt_flags, cam.num_samples = A.INTEGRATOR_PATH, flags, 2
    with rtg.Renderer(sc, device=gpu) as r:
        img = r.render(0)
    o = pyoracle.Oracle(sc)
    ref = o.render(0)[0]
    o.close()
    linf, frac, nanm = _cmp(img, ref)
    print(f"path {name} flags={flags}: Linf={linf:.3g} differing={frac:.2e} nan_mismatch={nanm}")
    assert len(np.unique(bits(ref))) > 100
    assert nanm == 0
    assert linf < TOL


# ------------------------------------------------------------------------------------------------ hit records
BUILDERS, RAYS, reference = tc.BUILDERS, tc.RAYS, tc.reference
TRACES = [(b, g) for b in BUILDERS for g in RAYS[b]]


@pytest.mark.parametrize("builder,gen", TRACES, ids=[f"{b}-{g}" for b, g in TRACES])
def test_hit_records_match_oracle(gpu, builder, gen):
    (o, d, t), ref = reference(builder, gen)
    m = ref["full"] == 1
    nan = np.isnan(ref["normal"]).any(1) & m
    print(f"{builder} {gen}: rays={len(o)} hits={int(m.sum())} nan_normals={int(nan.sum())}")
    # not vacuous, by the oracle alone
    assert m.sum() >= 1000
    if gen == "pole_rays":
        assert nan.any() and (m & ~nan).any()
    elif builder == "degenerate_uv":
        assert nan.sum() >= 0.1 * m.sum()
    else:
        assert not nan.any()
    with rtg.Renderer(BUILDERS[builder](), device=gpu) as r:
        for trav in (0, 1):
            h = r.trace(o, d, t, traversal=trav)
            for k in ("full", "object", "prim", "material"):
                assert np.array_equal(h[k], ref[k]), (trav, k)
            assert np.array_equal(bits(h["t"][m]), bits(ref["t"][m])), trav
            assert np.array_equal(bits(h["point"][m]), bits(ref["point"][m])), trav
            gn, rn = h["normal"][m], ref["normal"][m]
            assert np.array_equal(np.isnan(gn), np.isnan(rn)), trav
            fin = ~np.isnan(rn)
            assert np.array_equal(bits(gn[fin]), bits(rn[fin])), trav


# ------------------------------------------------------------------------------------------------ AOV
KD_DECALS = (A.DECAL_REPLACE_KD, A.DECAL_BLEND_KD, A.DECAL_REPLACE_ALL)
# float32 Perlin against the float64 restatement tests/texture_cases.perlin_f64: the point handed to Perlin is
# the object-space hit, rebuilt here from the world point through the float64 inverse model, off by a few
# float32 ulp of coordinates below 8 (4 * 2^-21 = 2e-6) per axis, times a gradient of at most 2 * noise_scale
# = 6 per axis: 3 * 6 * 2e-6 = 3.6e-5, which also covers the float32 evaluation itself (measured at 1.7e-6 in
# test_texture_kat.py).  A bound by reasoning, not a measurement: Perlin has no replace_all render to take the
# bits from; the test prints what it observes (1.85e-6 at the most on MI355X)
PERLIN_ALBEDO_TOL = 4e-5


def final_decal(sc, o):
    """(decal, texture) left in the hit record by the object's texture list: the last kd-kind texture wins."""
    out = (A.DECAL_NONE, None)
    for ti in o.textures:
        t = sc.textures[ti - 1]
        if (t.kind == A.TEX_IMAGE and t.decal in KD_DECALS) or (t.kind == A.TEX_PERLIN and t.decal == A.DECAL_REPLACE_KD):
            out = (t.decal, t)
    return out


@pytest.mark.parametrize("name", ["tex_matrix", "tri_matrix"])
def test_aov_normal_and_albedo(gpu, name):
    """The AOV normal is Renderer.trace's on the camera's own rays; the albedo is k_aov's decal rule (kd,
    tc / tn, or their mean) on the oracle's hit: tc of an image texture is what the oracle renders with that
    texture's decal set to replace_all, tc of a Perlin texture the float64 restatement at the hit point."""
    sc = BUILDERS[name]()
    assert sc.cameras[0].num_samples == 1
    ny, nx = sc.cameras[0].ny, sc.cameras[0].nx
    with rtg.Renderer(sc, device=gpu) as r:
        a = r.aov(0)
        o, d, t = (v.reshape(-1, 3) if v.ndim == 4 else v.reshape(-1) for v in r.camera_rays(0))
        own = r.trace(o, d, t)
    orc = pyoracle.Oracle(sc)
    ref = orc.trace(o, d, t)
    orc.close()
    hit = (ref["full"] == 1).reshape(ny, nx)
    assert np.array_equal(a["hits"] == 1, hit) and np.array_equal(own["full"], ref["full"])
    # the contract's one-sample mean: (0 + n) / 1, which turns a component of -0 into +0
    want_n = np.where(hit[..., None], (np.zeros((ny, nx, 3), f32) + own["normal"].reshape(ny, nx, 3)) / f32(1), f32(0))
    assert want_n.dtype == f32
    assert np.array_equal(np.isnan(a["normal"]), np.isnan(want_n))
    assert np.array_equal(bits(np.nan_to_num(a["normal"])), bits(np.nan_to_num(want_n)))
    assert np.array_equal(a["object"], np.where(hit, ref["object"].reshape(ny, nx), -1))
    # the texture colour of image decals: the same scene with those decals turned into replace_all
    every = copy.deepcopy(sc)
    for tx in every.textures:
        if tx.kind == A.TEX_IMAGE and tx.decal in KD_DECALS:
            tx.decal = A.DECAL_REPLACE_ALL
    orc = pyoracle.Oracle(every)
    tc_img = orc.render(0)[0]
    orc.close()
    entries = {i: (ob, tc.model_matrix(sc, ob.xforms), ob.material) for i, ob in enumerate(sc.objects)}
    for e in tc.textured_entries(sc):
        if e["top"] >= len(sc.objects):
            entries[e["top"]] = (e["obj"], e["M"], sc.instances[e["top"] - len(sc.objects)].material)
    top = ref["object"].reshape(ny, nx)
    point = ref["point"].reshape(ny, nx, 3)
    seen = set()
    for i in np.unique(top[hit]):
        if i not in entries:
            continue                              # an instance of an untextured base
        ob, M, mat = entries[int(i)]
        on = hit & (top == i)
        kd = np.asarray(sc.materials[mat - 1].diffuse, f32)
        decal, tx = final_decal(sc, ob)
        got = a["albedo"][on]
        seen.add((decal, None if tx is None else tx.kind, i >= len(sc.objects)))
        if tx is not None and tx.kind == A.TEX_PERLIN:
            assert np.array_equal(bits(got[:, 0]), bits(got[:, 1])) and np.array_equal(bits(got[:, 0]), bits(got[:, 2]))
            p_obj = (point[on].astype(np.float64) - M[:3, 3]) @ np.linalg.inv(M[:3, :3]).T
            want = tc.perlin_f64(p_obj, tx.noise_scale, tx.noise_conv)
            print(f"{name} entry {i}: Perlin albedo |float32 - float64 restatement| = {np.abs(got[:, 0] - want).max():.3g}")
            assert np.abs(got[:, 0] - want).max() <= PERLIN_ALBEDO_TOL, (i, np.abs(got[:, 0] - want).max())
            continue
        if decal == A.DECAL_NONE:
            want = np.broadcast_to(kd, got.shape)
        else:
            over = tc_img[on] / f32(tx.normalizer)
            assert over.dtype == f32
            want = (kd + over) * f32(0.5) if decal == A.DECAL_BLEND_KD else over
        assert np.array_equal(np.isnan(got), np.isnan(want)), i
        assert np.array_equal(bits(np.nan_to_num(got)), bits(np.nan_to_num(f32(0) + np.asarray(want, f32)))), i
    kinds = {(s[0], s[1]) for s in seen}
    assert {(A.DECAL_REPLACE_KD, A.TEX_IMAGE), (A.DECAL_BLEND_KD, A.TEX_IMAGE), (A.DECAL_REPLACE_ALL, A.TEX_IMAGE),
            (A.DECAL_REPLACE_KD, A.TEX_PERLIN), (A.DECAL_NONE, None)} <= kinds
    if name == "tex_matrix":
        assert any(s[2] for s in seen)            # an instanced entry
    assert not np.asarray(a["albedo"])[~hit].any()
