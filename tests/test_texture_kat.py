"""Known answers for object texturing that do not rest on the oracle's own output: closed forms from the
reference's text (src/Texture.cpp:41-131, src/Shape.cpp:400-616, src/Perlin.cpp:27-97).  Every check runs
against the oracle on the CPU and, marked gpu, against librtg, so both cannot be wrong in the same way.

  constant 1 x 1 texture   replace_all gives the colour; replace_kd / blend_kd give the untextured frame with
                           the decal's diffuse; a bump map of a constant image leaves the normal alone
  W x H distinct texels    nearest lookup reads tex[int(v * H), int(u * W)]: rows are v
  Perlin                   0 / 0.5 / 0 at lattice points, absval = |none|, linear = (none + 1) / 2, and the
                           float64 restatement tests/texture_cases.perlin_f64, negative coordinates included
"""
import numpy as np
import pytest

import pyoracle
import texture_cases as tc
from rtg import _abi as A
from rtg import scenegen
from rtg.scene import Instance, Light, Material, Object, Scene, Texture

f32 = np.float32
ERR_INVALID = -1          # RTG_ERR_INVALID (include/rtg.h)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ backends
class OracleSide:
    def render(self, sc, cam=0):
        o = pyoracle.Oracle(sc)
        img, obj, _, _ = o.render(cam)
        o.close()
        return img, obj

    def trace(self, sc, o, d, t=None):
        orc = pyoracle.Oracle(sc)
        h = orc.trace(o, d, t)
        orc.close()
        return h


class GpuSide:
    def __init__(self, device):
        self.device = device

    def render(self, sc, cam=0):
        import rtg
        with rtg.Renderer(sc, device=self.device) as r:
            return r.render(cam), r.aov(cam)["object"]

    def trace(self, sc, o, d, t=None):
        import rtg
        with rtg.Renderer(sc, device=self.device) as r:
            return r.trace(o, d, t)


ORACLE = OracleSide()        # where a test needs the oracle's hit points whichever side it checks


@pytest.fixture(params=["oracle", pytest.param("gpu", marks=pytest.mark.gpu)])
def side(request):
    if request.param == "gpu":
        return GpuSide(request.getfixturevalue("gpu"))
    return ORACLE


def primary_rays(cam):
    """Pixel-centre rays of a pinhole camera (Camera::getPrimaryRay, src/Camera.cpp:63-72), float64 rounded to
    float32, row-major."""
    pos = np.asarray(cam.position, np.float64)
    gaze = np.asarray(cam.gaze, np.float64)
    gaze = gaze / np.linalg.norm(gaze)
    right = np.cross(np.asarray(cam.up, np.float64), -gaze)
    right /= np.linalg.norm(right)
    up = np.cross(-gaze, right)
    l, r, b, t = cam.near_plane
    row, col = np.mgrid[0:cam.ny, 0:cam.nx]
    u = l + (r - l) * (col.reshape(-1) + 0.5) / cam.nx
    v = t - (t - b) * (row.reshape(-1) + 0.5) / cam.ny
    d = gaze * cam.near_distance + u[:, None] * right + v[:, None] * up
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.repeat(pos[None], len(d), 0).astype(f32), d.astype(f32)


# ------------------------------------------------------------------------------------------------ constant texture
KD = (0.3, 0.55, 0.7)
UNIT_UV = [(0, 0), (1, 0), (1, 1), (0, 1)]


def const_scene(texture=None, diffuse=KD, max_depth=1, nx=40, ny=30):
    """A sphere over a quad, both with `texture` (or none), one point light, background in view."""
    sc = Scene(max_depth=max_depth, background=(3, 4, 5), ambient=(20, 20, 20))
    sc.cameras.append(scenegen._cam((0, 1.5, 4.5), (0, -0.3, -1), (0, 1, 0), nx, ny, fov_deg=50, name="kat.png"))
    sc.materials.append(Material(ambient=(1, 1, 1), diffuse=tuple(diffuse), specular=(0.3, 0.3, 0.3), phong_exp=10))
    texs = []
    if texture is not None:
        sc.textures.append(texture)
        sc.images = ["const.ppm"]
        texs = [1]
    c = scenegen._add_vertices(sc, [(0.2, 0.7, -0.4)])
    sc.objects.append(Object(type=A.OBJ_SPHERE, id=1, material=1, center=c, radius=0.7, textures=list(texs)))
    fl = scenegen._add_vertices(sc, [(-2, 0, 2), (2, 0, 2), (2, 0, -3), (-2, 0, -3)])
    sc.texcoords = np.array(UNIT_UV, f32)
    sc.objects.append(Object(type=A.OBJ_MESH, id=1, material=1, textures=list(texs),
                             faces=np.array([[fl, fl + 1, fl + 2], [fl, fl + 2, fl + 3]], np.int32),
                             texture_offset=-(fl - 1)))
    sc.lights.append(Light(type=A.LIGHT_POINT, position=(1, 5, 3), intensity=(20000, 20000, 20000)))
    return sc


def const_texture(decal, interp, colour, normalizer, shape=(1, 1)):
    texels = np.broadcast_to(np.asarray(colour, f32), shape + (3,)).copy()
    return Texture(kind=A.TEX_IMAGE, decal=decal, interp=interp, normalizer=normalizer, bump_factor=3.0,
                   texels=texels, image_id=1)


COLOURS = [((200.0, 120.0, 40.0), 255), ((0.8, 0.45, 0.15), 1)]


@pytest.mark.parametrize("colour,normalizer", COLOURS, ids=["n255", "n1"])
def test_constant_replace_all(side, colour, normalizer):
    """Scene::Shading returns the texture colour itself (src/Scene.cpp:230-241).  Nearest: the texel, bit for
    bit.  Bilinear: the four weights (1-a)(1-b), (1-a)b, a(1-b), ab sum to 1 only after rounding, each
    product and each of the three additions within half an ulp: within 4 ulp of the colour."""
    c = np.asarray(colour, f32)
    img, obj = side.render(const_scene(const_texture(A.DECAL_REPLACE_ALL, A.INTERP_NN, colour, normalizer), max_depth=0))
    hit = obj >= 0
    assert set(np.unique(obj)) == {-1, 0, 1} and hit.sum() > 300
    assert np.array_equal(bits(img[hit]), np.broadcast_to(bits(c), img[hit].shape))
    assert not np.array_equal(bits(img[~hit][0]), bits(c))
    bil, obj2 = side.render(const_scene(const_texture(A.DECAL_REPLACE_ALL, A.INTERP_BILINEAR, colour, normalizer),
                                        max_depth=0))
    assert np.array_equal(obj2, obj)
    ulp = np.abs(bits(bil[hit]).astype(np.int64) - bits(c).astype(np.int64))
    print("bilinear: largest ulp distance", int(ulp.max()))
    assert ulp.max() <= 4


@pytest.mark.parametrize("interp", [A.INTERP_NN, A.INTERP_BILINEAR], ids=["nn", "bilinear"])
@pytest.mark.parametrize("colour,normalizer", COLOURS, ids=["n255", "n1"])
def test_constant_replace_kd_and_blend_kd(side, colour, normalizer, interp):
    """replace_kd shades with colour / normalizer, blend_kd with (kd + colour / normalizer) * 0.5f (e.g.
    PointLight::Diffuse, src/Light.cpp:206-223), both in float32: the frame is the untextured one with that
    diffuse reflectance, bit for bit.  (Nearest only for the bit-exact claim; bilinear's colour is within 4
    ulp, so its frame is compared to 1e-3 of the 0..255 range.)"""
    over = np.asarray(colour, f32) / f32(normalizer)
    blend = (np.asarray(KD, f32) + over) * f32(0.5)
    assert over.dtype == f32 and blend.dtype == f32
    for decal, kd in ((A.DECAL_REPLACE_KD, over), (A.DECAL_BLEND_KD, blend)):
        img, obj = side.render(const_scene(const_texture(decal, interp, colour, normalizer)))
        plain, obj0 = side.render(const_scene(None, diffuse=kd))
        assert np.array_equal(obj, obj0) and (obj >= 0).sum() > 300
        assert not np.isnan(img).any()
        if interp == A.INTERP_NN:
            assert np.array_equal(bits(img), bits(plain)), decal
        else:
            assert np.abs(img.astype(np.float64) - plain).max() < 1e-3, decal
        base, _ = side.render(const_scene(None))
        assert not np.array_equal(bits(base), bits(plain))       # the decal's diffuse is not the material's


def bump_rays(sc, n=3000, seed=5):
    """Rays toward points of the sphere and of the quad.  Two quirks of the reference bound what a closed form
    can say about its hit points, and the rays keep clear of both: Sphere::bvhIntersect's discriminant
    cancels at grazing incidence (src/Shape.cpp:347-398), leaving the point off the sphere by up to 1e-4, so
    the sphere's rays arrive within about 20 degrees of its normal; and Helper.cpp:39-49 re-derives a hit's t
    from the x components alone (Ray::gett, src/Ray.cpp:21-36), so every ray has |d.x| > 0.3.  The sphere's
    points stay off its poles (|cos theta| < 0.9)."""
    rng = np.random.default_rng(seed)
    V = np.asarray(sc.vertices, np.float64)
    sph = sc.objects[0]
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u = u[(np.abs(u[:, 1]) < 0.9) & (np.abs(u[:, 0]) > 0.5) & (u[:, 1] > -0.3)]
    ps = V[sph.center - 1] + sph.radius * u
    os_ = ps + 2.0 * u + rng.uniform(-0.3, 0.3, ps.shape)
    pq = np.stack([rng.uniform(-1.9, 1.9, n), np.zeros(n), rng.uniform(-2.9, 1.9, n)], 1)
    oq = pq + np.stack([rng.uniform(1.5, 2.5, n) * rng.choice([-1.0, 1.0], n), rng.uniform(1.0, 3.0, n),
                        rng.uniform(1.0, 3.0, n)], 1)
    p, o = np.concatenate([ps, pq]), np.concatenate([os_, oq])
    d = p - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert (np.abs(d[:, 0]) > 0.3).all()
    return o.astype(f32), d.astype(f32)


def bump_restated(sc, hits):
    """normalized(cross(dpv, dpu)) with du = dv = 0 in float64 at the hit points (src/Shape.cpp:441-478 for the
    sphere, 556-600 for the triangle), turned to the geometric normal's side."""
    p = hits["point"].astype(np.float64)
    out = np.full(p.shape, np.nan)
    V = np.asarray(sc.vertices, np.float64)
    sph = hits["object"] == 0
    c, R = V[sc.objects[0].center - 1], float(f32(sc.objects[0].radius))
    lc = p[sph] - c
    theta = np.arccos(np.clip(lc[:, 1] / R, -1, 1))
    phi = np.arctan2(lc[:, 2], lc[:, 0])
    dpdu = np.stack([2 * np.pi * lc[:, 2], np.zeros(len(lc)), -2 * np.pi * lc[:, 0]], 1)
    dpdv = np.stack([np.pi * lc[:, 1] * np.cos(phi), -np.pi * R * np.sin(theta), np.pi * lc[:, 1] * np.sin(phi)], 1)
    n = np.cross(dpdv, dpdu)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    out[sph] = np.where(((n * lc).sum(1) > 0)[:, None], n, -n)
    quad = hits["object"] == 1
    f = np.asarray(sc.objects[1].faces)
    uv = np.asarray(UNIT_UV, np.float64)
    for k in (0, 1):
        a, b, cc = V[f[k] - 1]
        i = f[k] - 1 + sc.objects[1].texture_offset
        TB = np.linalg.inv(np.array([uv[i[1]] - uv[i[0]], uv[i[2]] - uv[i[0]]])) @ np.array([b - a, cc - a])
        nn = np.cross(TB[1], TB[0])
        nn /= np.linalg.norm(nn)
        geo = np.cross(cc - b, a - b)
        out[quad & (hits["prim"] == k)] = nn if nn @ geo > 0 else -nn
    return out


# the largest |oracle float32 normal - float64 restatement| measured on the CPU over the hits the test keeps
# (1 x 1 and 3 x 2 constant images alike): 2.24e-7 on the sphere, 0 on the quad; times 4
BUMP_MEASURED = 2.24e-7
BUMP_TOL = 4 * BUMP_MEASURED


@pytest.mark.parametrize("shape", [(1, 1), (2, 3)], ids=["1x1", "3x2"])
def test_constant_bump_leaves_the_normal(side, shape):
    """A bump map of a constant image has du = dv = 0, so the bumped normal is normalized(cross(dpdv, dpdu)), the
    surface's own normal: on the quad and on the sphere `trace` gives the untextured normal.  The tolerance
    is BUMP_TOL = 8.96e-7: 4 x the largest rounding difference between the oracle and the float64 restatement
    bump_restated, measured on the CPU at 2.24e-7.  On the sphere the closed form itself equals the geometric
    normal only as far as the reported point lies on the sphere (Sphere::TextureComputation takes sin theta from
    the radius, the rest from the point; float32 leaves the point up to 1.5e-6 off): that float64 gap, computed
    per hit from the oracle's points (up to 1.76e-6 here), is added to BUMP_TOL for the comparison with the
    untextured record (largest excess over the gap measured on the CPU: 1.32e-7)."""
    sc = const_scene(const_texture(A.DECAL_BUMP_NORMAL, A.INTERP_NN, (90.0, 60.0, 30.0), 255, shape))
    o, d = bump_rays(sc)
    ref = ORACLE.trace(sc, o, d)
    m = ref["full"] == 1
    # the rays aimed at the quad meet the sphere too, anywhere: keep, by the oracle's untextured record, the
    # sphere hits bump_rays' doc describes (off the poles, within 26 degrees of the normal)
    flat = ORACLE.trace(const_scene(None), o, d)
    centre = np.asarray(sc.vertices, np.float64)[sc.objects[0].center - 1]
    cos_t = (ref["point"][:, 1] - centre[1]) / sc.objects[0].radius
    head_on = np.abs((flat["normal"] * d).sum(1)) > 0.9
    m &= (ref["object"] == 1) | ((np.abs(cos_t) < 0.9) & head_on)
    assert ((ref["object"] == 0) & m).sum() > 500 and ((ref["object"] == 1) & m).sum() > 500
    want = bump_restated(sc, ref)
    assert not np.isnan(want[m]).any()
    h = side.trace(sc, o, d)
    plain = side.trace(const_scene(None), o, d)
    assert np.array_equal(h["full"], ref["full"]) and np.array_equal(h["object"], ref["object"])
    assert np.array_equal(plain["object"], ref["object"])
    err = np.abs(h["normal"][m] - want[m]).max()
    geo = np.where((ref["object"] == 0)[:, None], ref["point"].astype(np.float64) - centre, want)
    geo /= np.linalg.norm(geo, axis=1, keepdims=True)
    gap = np.abs(want[m] - geo[m]).max(1)
    off = np.abs(h["normal"][m].astype(np.float64) - plain["normal"][m]).max(1)
    print(f"bump {shape}: |n - restated| = {err:.3g}, |n - untextured| = {off.max():.3g}, "
          f"|restated - geometric| = {gap.max():.3g}")
    assert err <= BUMP_TOL
    print(f"bump {shape}: largest |n - untextured| - gap = {(off - gap).max():.3g}")
    assert (off <= BUMP_TOL + gap).all()


# ------------------------------------------------------------------------------------------------ texel lookup
def lookup_scene(w, h, nx=40, ny=30):
    """The unit-texcoord quad [-1, 1]^2 just inside a pinhole camera's frame, replace_all, nearest, texel (row j,
    column i) = 3 * (j * w + i) + channel."""
    sc = Scene(max_depth=0, background=(3, 4, 5), ambient=(20, 20, 20))
    sc.cameras.append(scenegen._cam((0.03, -0.02, 2.0), (0, 0, -1), (0, 1, 0), nx, ny, fov_deg=57, name="lookup.png"))
    tex = (3 * np.arange(w * h).reshape(h, w, 1) + np.arange(3)).astype(f32)
    assert tex.max() <= 255 and len(np.unique(tex)) == tex.size
    sc.textures.append(Texture(kind=A.TEX_IMAGE, decal=A.DECAL_REPLACE_ALL, interp=A.INTERP_NN, normalizer=255,
                               texels=tex, image_id=1))
    sc.images = ["lookup.ppm"]
    sc.materials.append(Material(ambient=(1, 1, 1), diffuse=KD))
    b = scenegen._add_vertices(sc, [(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)])
    sc.texcoords = np.array(UNIT_UV, f32)
    sc.objects.append(Object(type=A.OBJ_MESH, id=1, material=1, textures=[1],
                             faces=np.array([[b, b + 1, b + 2], [b, b + 2, b + 3]], np.int32), texture_offset=-(b - 1)))
    sc.lights.append(Light(type=A.LIGHT_POINT, position=(0, 0, 3), intensity=(1000, 1000, 1000)))
    return sc, tex


@pytest.mark.parametrize("w,h", [(5, 3), (2, 1), (1, 7), (8, 6)])
def test_nearest_lookup_reads_row_v_column_u(side, w, h):
    """GetColorAtCoordinates (src/Texture.cpp:111-118): i = u * width, j = v * height, texel (row j, column i).
    uv is recomputed in float64 from the oracle's hit point of each pixel's primary ray; hits within 1e-3
    texel of a texel boundary are left out (at most 2 % of the frame: a boundary band of 2e-3 texel against
    pixels a fifth of a texel or more wide).  A w / h swap in the row stride fails here by itself."""
    sc, tex = lookup_scene(w, h)
    cam = sc.cameras[0]
    o, d = primary_rays(cam)
    ref = ORACLE.trace(sc, o, d)
    img, obj = side.render(sc)
    hit = ref["full"] == 1
    assert 0.6 < hit.mean() < 1 and (ref["object"][hit] == 0).all()
    assert np.array_equal(obj.reshape(-1), np.where(hit, ref["object"], -1))      # the render's id buffer
    p = ref["point"][hit].astype(np.float64)
    u, v = (p[:, 0] + 1) / 2, (p[:, 1] + 1) / 2
    assert (u > 0).all() and (u < 1).all() and (v > 0).all() and (v < 1).all()
    fu, fv = u * w - np.floor(u * w), v * h - np.floor(v * h)
    clear = (np.minimum(fu, 1 - fu) > 1e-3) & (np.minimum(fv, 1 - fv) > 1e-3)
    print(f"{w}x{h}: {(~clear).mean():.2%} of hits near a texel boundary")
    assert (~clear).mean() <= 0.02
    want = tex[(v * h).astype(np.int64), (u * w).astype(np.int64)]
    assert len(np.unique(want[clear], axis=0)) == w * h              # every texel is seen
    assert np.array_equal(bits(img.reshape(-1, 3)[hit][clear]), bits(want[clear]))


# ------------------------------------------------------------------------------------------------ Perlin
SCALE = 2.0
# the largest |float32 colour - perlin_f64| measured on the CPU (oracle) over perlin_scene's 40 x 30 frame:
# 1.68e-6 for none and absval, 8.3e-7 for linear (the float32 noise itself and the float32 hit point, times a
# gradient of up to 2 * SCALE per axis); times 4
PERLIN_MEASURED = 1.68e-6
PERLIN_TOL = 4 * PERLIN_MEASURED


def perlin_scene(nc, nx=40, ny=30, lattice=()):
    """A plane z = 0 facing a directional light of radiance 1 head-on, nothing in the way, ambient 0, no
    specular: colour = 1 * (p / 1 * cos 0) = the Perlin value p.  Camera 0 sees x in about [-2.4, 2.4]; one more
    1 x 1 camera gazes at each point of `lattice` (at a slant: the reference's traversal loses a ray along an
    axis on a flat box), so its one ray meets the plane within a float32 ulp or two of that point, on any side."""
    sc = Scene(max_depth=0, background=(0, 0, 0), ambient=(0, 0, 0))
    sc.cameras.append(scenegen._cam((0.1, -0.2, 4.0), (0, 0, -1), (0, 1, 0), nx, ny, fov_deg=48, name="perlin.png"))
    for x, y in lattice:
        sc.cameras.append(scenegen._cam((x + 0.3, y + 0.2, 1.0), (-0.3, -0.2, -1.0), (0, 1, 0), 1, 1, fov_deg=10,
                                        name="lattice.png"))
    sc.textures.append(Texture(kind=A.TEX_PERLIN, decal=A.DECAL_REPLACE_KD, noise_conv=nc, noise_scale=SCALE))
    sc.materials.append(Material(ambient=(0, 0, 0), diffuse=KD, specular=(0, 0, 0), phong_exp=1))
    b = scenegen._add_vertices(sc, [(-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0)])
    sc.objects.append(Object(type=A.OBJ_MESH, id=1, material=1, textures=[1],
                             faces=np.array([[b, b + 1, b + 2], [b, b + 2, b + 3]], np.int32)))
    sc.lights.append(Light(type=A.LIGHT_DIRECTIONAL, direction=(0, 0, -1), intensity=(1, 1, 1)))
    return sc


LATTICE = [(0.0, 0.0), (0.5, -1.5), (-2.0, 1.0), (-0.5, -0.5), (1.5, 2.0), (-3.0, -2.5)]
NCS = {"none": A.NC_NONE, "linear": A.NC_LINEAR, "absval": A.NC_ABSVAL}


def test_perlin_known_answers(side):
    """src/Perlin.cpp:52-84.  At a lattice point the offset to that corner is 0 and the other seven corners
    have a weight factor Weight(1) = -6 + 15 - 10 + 1 = 0: the noise is 0, so none / linear / absval give
    0 / 0.5 / 0 (a hit 2e-7 off the point moves the noise by its gradient, at most 2 * SCALE per axis, times
    that: 2.4e-6 at the worst, inside the tolerance).  Over a frame, absval = |none| and linear = (none + 1) / 2 pixel for pixel, and each equals
    the float64 restatement at the oracle's hit points, negative coordinates (GetFromShuffled's index < 0
    branch) included.  Tolerance PERLIN_TOL = 6.72e-6: 4 x the largest float32-against-float64 difference
    measured on the CPU against the restatement, 1.68e-6."""
    frames = {}
    for name, nc in NCS.items():
        sc = perlin_scene(nc, lattice=LATTICE)
        img, obj = side.render(sc)
        assert (obj == 0).all()
        assert np.array_equal(bits(img[..., 0]), bits(img[..., 1])) and np.array_equal(bits(img[..., 0]), bits(img[..., 2]))
        frames[name] = img[..., 0].astype(np.float64)
        shots = [side.render(sc, k + 1) for k in range(len(LATTICE))]
        assert all(obj1[0, 0] == 0 for _, obj1 in shots)
        at_lattice = np.array([img1[0, 0, 0] for img1, _ in shots], np.float64)
        print(name, "at lattice points:", at_lattice)
        assert np.abs(at_lattice - (0.5 if name == "linear" else 0.0)).max() <= PERLIN_TOL
        cam = sc.cameras[0]
        o, d = primary_rays(cam)
        ref = ORACLE.trace(sc, o, d)
        assert (ref["full"] == 1).all()
        p = ref["point"].astype(np.float64)
        assert (p[:, 0] < -1).any() and (p[:, 1] < -1).any() and (p[:, 0] > 1).any() and (p[:, 1] > 1).any()
        want = tc.perlin_f64(p, SCALE, nc).reshape(cam.ny, cam.nx)
        err = np.abs(frames[name] - want).max()
        print(f"{name}: |float32 - float64 restatement| = {err:.3g}, values in [{want.min():.3f}, {want.max():.3f}]")
        assert err <= PERLIN_TOL
    none = frames["none"]
    assert none.min() < -0.1 and none.max() > 0.1                   # a signed field, not a constant
    assert np.abs(frames["absval"] - np.abs(none)).max() <= PERLIN_TOL
    assert np.abs(frames["linear"] - (none + 1) / 2).max() <= PERLIN_TOL


# ------------------------------------------------------------------------------------------------ coverage
@pytest.mark.parametrize("builder", list(tc.BUILDERS))
def test_every_textured_entry_is_hit(builder):
    """The precondition of tests/test_gpu_texture.py's hit-record cases, on the oracle's output only: at least
    50 rays of the builder's ray classes hit each textured entry, the instances included."""
    sc = tc.BUILDERS[builder]()
    tops = [e["top"] for e in tc.textured_entries(sc)]
    total = np.zeros(len(sc.objects) + len(sc.instances), np.int64)
    for gen in tc.RAYS[builder]:
        ref = tc.reference(builder, gen)[1]
        total += np.bincount(ref["object"][ref["full"] == 1], minlength=len(total))
    print(builder, total[tops])
    assert len(tops) >= 2 and total[tops].min() >= 50


# ------------------------------------------------------------------------------------------------ validation
def bad_descriptions():
    """Scene descriptions with one index out of range each (what librtg's validate() refuses)."""
    out = {}

    def variant(name, change, base=None):
        sc = base() if base else scenegen.textured(8, 6)
        change(sc)
        out[name] = sc

    def add_instance(base):
        return lambda sc: sc.instances.append(Instance(base_object=base, id=9, material=1))
    variant("instance base too large", lambda sc: add_instance(len(sc.objects))(sc))
    variant("instance base negative", add_instance(-1))
    variant("object texture index too large", lambda sc: setattr(sc.objects[0], "textures", [len(sc.textures) + 1]))
    variant("object texture index zero", lambda sc: setattr(sc.objects[0], "textures", [0]))
    variant("object texture count", lambda sc: setattr(sc.objects[0], "textures", [1, 2, 3]))
    variant("background texture", lambda sc: setattr(sc, "background_texture", len(sc.textures)))
    variant("environment light texture", lambda sc: setattr(sc.lights[-1], "texture", len(sc.textures)),
            base=lambda: scenegen.envmap(8, 6))
    variant("environment light texture negative", lambda sc: setattr(sc.lights[-1], "texture", -1),
            base=lambda: scenegen.envmap(8, 6))
    variant("environment light index", lambda sc: setattr(sc, "environment_light", len(sc.lights)))
    return out


BAD = bad_descriptions()


@pytest.mark.parametrize("name", list(BAD))
def test_oracle_refuses_bad_indices(name):
    """orc_scene_create returns an error for the descriptions librtg refuses; it used to build them and
    crash in orc_render."""
    import ctypes as C
    lib = pyoracle.load()
    desc, keep = BAD[name].to_desc()
    h = C.c_void_p()
    assert lib.orc_scene_create(C.byref(desc), C.byref(h)) == ERR_INVALID
    assert not h.value
    good = scenegen.textured(8, 6)
    pyoracle.Oracle(good).close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BAD))
def test_librtg_refuses_bad_indices(gpu, name):
    import ctypes as C
    import rtg
    lib = rtg.load_library()
    desc, keep = BAD[name].to_desc()
    h = C.c_void_p()
    bo = A.BuildOpts(A.RTG_BVH_AUTO, 0, 0, 0)
    assert lib.rtg_scene_create_ex(C.byref(desc), int(gpu), C.byref(bo), C.byref(h)) == ERR_INVALID
    assert not h.value
