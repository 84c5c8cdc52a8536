"""Scenes and ray sets for the texturing tests (tests/test_gpu_texture.py, tests/test_texture_kat.py).

Scene builders (small frames, fixed seeds):

  tex_matrix      scenegen.textured's layout with every image texture of its own size and random texels, one
                  texture with normalizer 1, a Perlin replace_kd with NC_NONE, scaled / rotated / translated /
                  motion-blurred spheres, an instance of a textured sphere (resetTransform) and of the
                  textured floor (not reset), optionally only the point light
  tri_matrix      every decal (and two-texture pairs in both orders) over a flat quad, a smooth icosphere,
                  a standalone Triangle and a transformed quad; texcoords below 0, above 1 and exactly
                  integral; one mesh whose textureOffset sends two of three texcoord indices out of range
  degenerate_uv   bump and replace_normal quads with a zero UV determinant in one triangle each

Ray generators for `trace` (float64 maths rounded to float32, at most 8000 rays): pole_rays, seam_rays,
texel_edge_rays, random_rays.  They return (origins, directions, times).
"""
from __future__ import annotations

import functools
import math

import numpy as np

from rtg import _abi as A
from rtg import scenegen
from rtg.scene import Instance, Light, Material, Object, Scene, Texture

f32 = np.float32

SIZE_SETS = {
    "mixed": [(5, 3), (64, 64), (1, 7), (2, 1), (7, 1)],
    "ones": [(1, 1)] * 5,
    "thin": [(2, 2), (3, 2), (2, 3), (64, 1), (1, 64)],
}
MAX_RAYS = 8000


def random_texels(rng, w, h, unit=False):
    """(h, w, 3) float32: uint8 values, or floats in [0, 1] for a texture with normalizer 1."""
    if unit:
        return rng.random((h, w, 3)).astype(f32)
    return rng.integers(0, 256, (h, w, 3)).astype(np.uint8).astype(f32)


# ------------------------------------------------------------------------------------------------ builders
def tex_matrix(sizes, one_light=False, blur=False, nx=48, ny=36, spp=1, seed=7):
    """`blur` adds a motion blur to two of the plain spheres.  It does not switch the scene's blur off: the
    sphere instance is blurred in every variant, so every tex_matrix scene has motion blur (has_blur on);
    transformed textured entries without any blur in the scene are tri_matrix's quads."""
    rng = np.random.default_rng(seed)
    sc = scenegen.textured(nx, ny, spp)
    assert len(sizes) == 5 and [t.kind for t in sc.textures[:5]] == [A.TEX_IMAGE] * 5
    for k, (w, h) in enumerate(sizes):
        t = sc.textures[k]
        t.texels = random_texels(rng, w, h, unit=(k == 1))
        t.image_id = k + 1
        if k == 1:
            t.normalizer = 1                     # the blend_kd texture
    sc.images = [f"tex{k}.ppm" for k in range(5)]
    sc.textures.append(Texture(kind=A.TEX_PERLIN, decal=A.DECAL_REPLACE_KD, noise_conv=A.NC_NONE, noise_scale=2.5))
    sc.objects[8].textures = [len(sc.textures)]  # the sphere that had no texture
    sc.scalings += [(1.1, 0.8, 1.2), (0.9, 1.15, 0.85)]
    sc.rotations += [(20.0, 1.0, 2.0, 0.5), (-15.0, 0.3, 1.0, -0.7)]
    sc.translations += [(0.1, 0.25, -0.2), (-0.15, 0.1, 0.3), (0.0, 1.3, 0.6), (0.0, 0.4, 0.0)]
    for k in (0, 1, 2):                          # scaling then rotation about a skew axis
        sc.objects[k].xforms = [(A.XF_SCALING, 1 + k % 2), (A.XF_ROTATION, 1 + (k + 1) % 2)]
    for k in (3, 4, 5):
        sc.objects[k].xforms = [(A.XF_TRANSLATION, 1 + k % 2)]
    if blur:
        sc.objects[6].blur = (0.0, 0.3, 0.1)
        sc.objects[7].blur = (0.2, 0.0, -0.1)
    # base_object: 0-based index into objects
    sc.instances.append(Instance(base_object=2, id=20, material=3, reset_transform=True,
                                 xforms=[(A.XF_SCALING, 2), (A.XF_TRANSLATION, 3)], blur=(0.15, 0.1, 0.0)))
    sc.instances.append(Instance(base_object=9, id=21, material=2, reset_transform=False,
                                 xforms=[(A.XF_ROTATION, 2), (A.XF_TRANSLATION, 4)]))
    if one_light:
        sc.lights = [l for l in sc.lights if l.type == A.LIGHT_POINT]
        assert len(sc.lights) == 1
    return sc


QUAD_UVS = ([(-1.5, -0.25), (2, -0.25), (2, 3), (-1.5, 3)], [(0, 0), (1, 0), (1, 1), (0, 1)])
TRI_TEXSETS = [[1], [2], [3], [4], [5], [6], [7], [1, 3], [3, 1], [7, 4], [4, 7]]


def _tri_textures(sc, rng):
    sizes = [(5, 3), (8, 6), (7, 4), (16, 12), (3, 5)]
    decals = ((A.DECAL_REPLACE_KD, A.INTERP_NN), (A.DECAL_BLEND_KD, A.INTERP_BILINEAR),
              (A.DECAL_BUMP_NORMAL, A.INTERP_NN), (A.DECAL_REPLACE_NORMAL, A.INTERP_BILINEAR),
              (A.DECAL_REPLACE_ALL, A.INTERP_BILINEAR))
    for k, ((w, h), (decal, interp)) in enumerate(zip(sizes, decals)):
        sc.textures.append(Texture(kind=A.TEX_IMAGE, decal=decal, interp=interp, normalizer=255, bump_factor=1.5,
                                   texels=random_texels(rng, w, h), image_id=k + 1))
    sc.images = [f"tri{k}.ppm" for k in range(5)]
    sc.textures.append(Texture(kind=A.TEX_PERLIN, decal=A.DECAL_REPLACE_KD, noise_conv=A.NC_ABSVAL, noise_scale=3.0))
    sc.textures.append(Texture(kind=A.TEX_PERLIN, decal=A.DECAL_BUMP_NORMAL, noise_conv=A.NC_LINEAR,
                               noise_scale=5.0, bump_factor=0.5))


def _add(sc, verts, uvs):
    """Vertices with one texcoord each, so that texcoord index = vertex index (textureOffset 0: what a
    standalone Triangle always uses)."""
    b = scenegen._add_vertices(sc, verts)
    sc.texcoords = np.concatenate([np.asarray(sc.texcoords, f32).reshape(-1, 2), np.asarray(uvs, f32).reshape(-1, 2)])
    assert len(sc.texcoords) == len(sc.vertices)
    return b


def tri_matrix(nx=48, ny=36, spp=1, seed=11):
    rng = np.random.default_rng(seed)
    sc = Scene(max_depth=2, background=(5, 5, 5), ambient=(20, 20, 20))
    sc.cameras.append(scenegen._cam((0, 0, 9.5), (0, 0, -1), (0, 1, 0), nx, ny, fov_deg=46, spp=spp, name="tri.png"))
    _tri_textures(sc, rng)
    brdfs = [A.BRDF_NONE, A.BRDF_MBP, A.BRDF_TS, A.BRDF_OP]
    for k, br in enumerate(brdfs):
        sc.materials.append(Material(ambient=(0.5, 0.5, 0.5), diffuse=(0.6, 0.5 + 0.1 * k, 0.4), specular=(0.7, 0.7, 0.7),
                                     phong_exp=20 + 5 * k, brdf=br, refraction_index=1.8, absorption_index=0.5))
    sc.scalings += [(1.2, 0.8, 1.0), (0.8, 1.1, 1.3)]
    sc.rotations += [(25.0, 1.0, 2.0, 0.5), (-20.0, 0.4, -1.0, 0.8)]
    iv, ifc = scenegen.icosphere(1)
    ncol = len(TRI_TEXSETS)
    for col, ts in enumerate(TRI_TEXSETS):
        x = (col - (ncol - 1) / 2) * 1.0
        mat = 1 + col % len(brdfs)
        # row 0: flat two-triangle quad facing the camera
        y = 2.1
        uv = QUAD_UVS[col % 2]
        b = _add(sc, [(x - 0.42, y - 0.5, 0), (x + 0.42, y - 0.5, 0), (x + 0.42, y + 0.5, 0), (x - 0.42, y + 0.5, 0)], uv)
        sc.objects.append(Object(type=A.OBJ_MESH, id=4 * col + 1, material=mat, textures=list(ts),
                                 faces=np.array([[b, b + 1, b + 2], [b, b + 2, b + 3]], np.int32)))
        # row 1: smooth icosphere, texcoords from the vertex positions
        y = 0.7
        b = _add(sc, iv * 0.42 + np.array([x, y, 0.0]), np.stack([1.3 * iv[:, 0] + 0.1 * iv[:, 2],
                                                                  1.3 * iv[:, 1] - 0.2 * iv[:, 2]], 1))
        sc.objects.append(Object(type=A.OBJ_MESH, id=4 * col + 2, material=mat, textures=list(ts), smooth=True,
                                 faces=(ifc + b).astype(np.int32)))
        # row 2: standalone Triangle
        y = -0.7
        b = _add(sc, [(x - 0.45, y - 0.5, 0), (x + 0.45, y - 0.5, 0), (x, y + 0.5, 0)], [(0, 0), (1, 0), (0.5, 1.5)])
        sc.objects.append(Object(type=A.OBJ_TRIANGLE, id=4 * col + 3, material=mat, textures=list(ts), v=(b, b + 1, b + 2)))
        # row 3: transformed quad (scaling, rotation about a skew axis, then into its cell)
        y = -2.1
        uv = QUAD_UVS[(col + 1) % 2]
        b = _add(sc, [(-0.4, -0.45, 0), (0.4, -0.45, 0), (0.4, 0.45, 0), (-0.4, 0.45, 0)], uv)
        sc.translations.append((x, y, 0.0))
        sc.objects.append(Object(type=A.OBJ_MESH, id=4 * col + 4, material=mat, textures=list(ts),
                                 faces=np.array([[b, b + 1, b + 2], [b, b + 2, b + 3]], np.int32),
                                 xforms=[(A.XF_SCALING, 1 + col % 2), (A.XF_ROTATION, 1 + (col + 1) % 2),
                                         (A.XF_TRANSLATION, len(sc.translations))]))
    # the first column's flat quad: its texcoord indices are b-1 .. b+2 plus the offset; only the first
    # vertex's stays in range (the last texcoord), the other two of each triangle fall back to (0, 0)
    q = sc.objects[0]
    first = int(q.faces[0, 0])
    q.texture_offset = len(sc.texcoords) - first
    idx = np.asarray(q.faces) - 1 + q.texture_offset
    assert ((idx >= len(sc.texcoords)).sum(1) == 2).all()
    sc.lights.append(Light(type=A.LIGHT_POINT, position=(0, 3, 6), intensity=(20000, 20000, 20000)))
    sc.lights.append(Light(type=A.LIGHT_DIRECTIONAL, direction=(-0.3, -0.5, -1.0), intensity=(1.5, 1.5, 1.5)))
    sc.lights.append(Light(type=A.LIGHT_SPOT, position=(-3, 4, 6), direction=(0.4, -0.6, -1.0),
                           intensity=(30000, 20000, 20000), coverage_deg=60, falloff_deg=30))
    return sc


def degenerate_uv(nx=32, ny=24, spp=1, seed=13):
    """Two quads whose first triangle has two vertices with one texcoord: a zero UV determinant, invdet = inf,
    NaN normals on that triangle (bump and replace_normal)."""
    rng = np.random.default_rng(seed)
    sc = Scene(max_depth=1, background=(5, 5, 5), ambient=(20, 20, 20))
    sc.cameras.append(scenegen._cam((0, 0, 4), (0, 0, -1), (0, 1, 0), nx, ny, fov_deg=50, spp=spp, name="deg.png"))
    sc.textures.append(Texture(kind=A.TEX_IMAGE, decal=A.DECAL_BUMP_NORMAL, interp=A.INTERP_NN, normalizer=255,
                               bump_factor=2.0, texels=random_texels(rng, 6, 4), image_id=1))
    sc.textures.append(Texture(kind=A.TEX_IMAGE, decal=A.DECAL_REPLACE_NORMAL, interp=A.INTERP_BILINEAR, normalizer=255,
                               texels=random_texels(rng, 4, 6), image_id=2))
    sc.images = ["deg0.ppm", "deg1.ppm"]
    sc.materials.append(Material(ambient=(0.5, 0.5, 0.5), diffuse=(0.6, 0.5, 0.4), specular=(0.5, 0.5, 0.5), phong_exp=20))
    for k, x in enumerate((-0.9, 0.9)):
        b = _add(sc, [(x - 0.8, -0.8, 0), (x + 0.8, -0.8, 0), (x + 0.8, 0.8, 0), (x - 0.8, 0.8, 0)],
                 [(0, 0), (1, 0), (1, 0), (0, 1)])
        sc.objects.append(Object(type=A.OBJ_MESH, id=k + 1, material=1, textures=[k + 1],
                                 faces=np.array([[b, b + 1, b + 2], [b, b + 2, b + 3]], np.int32)))
    sc.lights.append(Light(type=A.LIGHT_POINT, position=(0, 2, 4), intensity=(8000, 8000, 8000)))
    return sc


# ------------------------------------------------------------------------------------------------ entries
def _rot(angle_deg, axis):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(angle_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    return M


def model_matrix(sc, xforms):
    """The composite of `xforms`, the first listed applied first (src/Helper.cpp:146-183), in float64."""
    M = np.eye(4)
    for ty, ix in xforms:
        X = np.eye(4)
        if ty == A.XF_TRANSLATION:
            X[:3, 3] = sc.translations[ix - 1]
        elif ty == A.XF_SCALING:
            X[:3, :3] = np.diag(np.asarray(sc.scalings[ix - 1], np.float64))
        elif ty == A.XF_ROTATION:
            r = sc.rotations[ix - 1]
            X = _rot(r[0], r[1:])
        else:
            X = np.asarray(sc.composites[ix - 1], np.float64).reshape(4, 4).T
        M = X @ M
    return M


def textured_entries(sc):
    """The textured top-level entries (objects, then instances): dicts with the hit records' `top` index, the
    base object, the float64 model matrix and the blur vector."""
    out = []
    for i, o in enumerate(sc.objects):
        if o.textures:
            out.append({"top": i, "obj": o, "M": model_matrix(sc, o.xforms), "blur": np.asarray(o.blur, np.float64)})
    for k, it in enumerate(sc.instances):
        base = sc.objects[it.base_object]
        if base.textures:
            M = model_matrix(sc, it.xforms)
            if not it.reset_transform:
                M = M @ model_matrix(sc, base.xforms)
            out.append({"top": len(sc.objects) + k, "obj": base, "M": M, "blur": np.asarray(it.blur, np.float64)})
    return out


def _triangles(sc, o):
    """(F, 3, 3) float64 vertices and (F, 3, 2) texcoords (out-of-range indices give (0, 0)) of a mesh or Triangle."""
    V = np.asarray(sc.vertices, np.float64)
    tc = np.asarray(sc.texcoords, np.float64).reshape(-1, 2)
    f = np.asarray(o.faces if o.type == A.OBJ_MESH else [o.v], np.int64).reshape(-1, 3)
    off = o.texture_offset if o.type == A.OBJ_MESH else 0
    idx = f - 1 + off
    ok = (idx >= 0) & (idx < len(tc))
    uv = np.where(ok[..., None], tc[np.clip(idx, 0, max(len(tc) - 1, 0))] if len(tc) else 0.0, 0.0)
    return V[f - 1], uv


def _world_rays(e, p_obj, o_obj, rng):
    """Rays from object-space origins toward object-space points of entry `e`, in world space at a random time."""
    n = len(p_obj)
    t = rng.random(n).astype(f32)
    shift = e["blur"][None] * t.astype(np.float64)[:, None]
    M = e["M"]
    pw = p_obj @ M[:3, :3].T + M[:3, 3] + shift
    ow = o_obj @ M[:3, :3].T + M[:3, 3] + shift
    d = pw - ow
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return ow.astype(f32), d.astype(f32), t


def _cat(parts):
    o = np.concatenate([p[0] for p in parts])[:MAX_RAYS]
    d = np.concatenate([p[1] for p in parts])[:MAX_RAYS]
    t = np.concatenate([p[2] for p in parts])[:MAX_RAYS]
    assert o.dtype == f32 and d.dtype == f32 and t.dtype == f32 and len(o) <= MAX_RAYS
    return o, d, t


def _ulps(x32, k):
    """float32 array moved by k (integer array, |k| small) units in the last place."""
    b = np.ascontiguousarray(x32, f32).view(np.int32).astype(np.int64)
    mag = np.where(b < 0, -(b & 0x7FFFFFFF), b) + k
    out = np.where(mag < 0, (-mag) | 0x80000000, mag).astype(np.uint32)
    return out.view(f32)


def _cone(axis, n, rng, spread=0.9):
    """Unit vectors within about `spread` radians of the rows of `axis`."""
    v = axis + spread * 0.6 * rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    flip = (v * axis).sum(1) < 0.2
    v[flip] = axis[flip]
    return v


def _sphere_entries(sc):
    return [e for e in textured_entries(sc) if e["obj"].type == A.OBJ_SPHERE]


# ------------------------------------------------------------------------------------------------ ray sets
def pole_rays(sc, seed=101):
    """Aimed at centre +- (0, R, 0) of every textured sphere entry, exactly and up to 4 float32 ulp off."""
    rng = np.random.default_rng(seed)
    es = _sphere_entries(sc)
    per = MAX_RAYS // (2 * len(es))
    V = np.asarray(sc.vertices, f32)
    parts = []
    for e in es:
        c = V[e["obj"].center - 1]
        R = f32(e["obj"].radius)
        for sgn in (1.0, -1.0):
            pole = np.repeat((c + np.array([0, sgn * R, 0], f32))[None].astype(f32), per, 0)
            k = rng.integers(-4, 5, (per, 3))
            k[: per // 3] = 0                            # a third exactly at the pole
            p = _ulps(pole, k).astype(np.float64)
            axis = np.repeat(np.array([[0.0, sgn, 0.0]]), per, 0)
            # the lower poles sit on or just above the floor: start close to them
            dist = rng.uniform(0.5, 3.0, (per, 1)) if sgn > 0 else rng.uniform(0.03, 0.2, (per, 1))
            o = p + _cone(axis, per, rng) * dist
            parts.append(_world_rays(e, p, o, rng))
    return _cat(parts)


def seam_rays(sc, seed=103):
    """Aimed at the phi = +-pi meridian of every textured sphere entry (x < centre, z on both sides of it by
    0, a few ulp and up to 1e-5 R), where the texture coordinate u wraps between 1 and 0."""
    rng = np.random.default_rng(seed)
    es = _sphere_entries(sc)
    per = MAX_RAYS // len(es)
    V = np.asarray(sc.vertices, np.float64)
    parts = []
    for e in es:
        c = V[e["obj"].center - 1]
        R = float(f32(e["obj"].radius))
        th = rng.uniform(0.15, math.pi - 0.15, per)
        dz = np.where(rng.random(per) < 0.5, rng.integers(-4, 5, per) * (R * 2.0 ** -24), rng.uniform(-1e-5, 1e-5, per) * R)
        n = np.stack([-np.sin(th), np.cos(th), dz / R], 1)
        p = c + R * n
        o = p + _cone(n / np.linalg.norm(n, axis=1, keepdims=True), per, rng) * rng.uniform(0.5, 3.0, (per, 1))
        parts.append(_world_rays(e, p, o, rng))
    return _cat(parts)


def _quad_entries(sc):
    return [e for e in textured_entries(sc) if e["obj"].type == A.OBJ_MESH and len(e["obj"].faces) == 2]


def texel_edge_rays(sc, seed=107):
    """Aimed at points of the textured quads whose float64 uv is an exact multiple of 1/w or 1/h of one of the
    quad's image textures, exactly and one float32 ulp either side (triangles with a zero UV determinant
    have no such points and are left out)."""
    rng = np.random.default_rng(seed)
    es = _quad_entries(sc)
    per = MAX_RAYS // (2 * len(es))
    parts = []
    for e in es:
        o = e["obj"]
        dims = [sc.textures[t - 1].texels.shape[:2] for t in o.textures if sc.textures[t - 1].kind == A.TEX_IMAGE]
        if not dims:
            dims = [(4, 4)]
        P, UV = _triangles(sc, o)
        for f in range(2):
            a, b, c = P[f]
            A2 = np.array([UV[f, 1] - UV[f, 0], UV[f, 2] - UV[f, 0]]).T      # uv = uv0 + A2 @ (beta, gamma)
            if abs(np.linalg.det(A2)) < 1e-12:
                continue
            bg = rng.random((per * 4, 2))
            bg = bg[bg.sum(1) < 1]
            uv = UV[f, 0] + bg @ A2.T
            h, w = dims[rng.integers(0, len(dims))]
            snap_u = rng.random(len(uv)) < 0.5
            uv[snap_u, 0] = np.round(uv[snap_u, 0] * w) / w
            uv[~snap_u, 1] = np.round(uv[~snap_u, 1] * h) / h
            bg = np.linalg.solve(A2, (uv - UV[f, 0]).T).T
            bg = bg[(bg[:, 0] > 0.01) & (bg[:, 1] > 0.01) & (bg.sum(1) < 0.99)][:per]
            p32 = (a + bg[:, :1] * (b - a) + bg[:, 1:] * (c - a)).astype(f32)
            k = np.repeat(rng.integers(-1, 2, (len(p32), 1)), 3, 1)       # exactly, or one ulp either side
            p = _ulps(p32, k).astype(np.float64)
            nrm = np.cross(c - b, a - b)
            nrm /= np.linalg.norm(nrm)
            org = p + _cone(np.repeat(nrm[None], len(p), 0), len(p), rng) * rng.uniform(0.5, 3.0, (len(p), 1))
            parts.append(_world_rays(e, p, org, rng))
    return _cat(parts)


def _surface_points(sc, e, n, rng):
    o = e["obj"]
    if o.type == A.OBJ_SPHERE:
        c = np.asarray(sc.vertices, np.float64)[o.center - 1]
        u = rng.standard_normal((n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        return c + float(f32(o.radius)) * u
    P, _ = _triangles(sc, o)
    f = rng.integers(0, len(P), n)
    bg = rng.random((n, 2))
    flip = bg.sum(1) > 1
    bg[flip] = 1 - bg[flip]
    return P[f, 0] + bg[:, :1] * (P[f, 1] - P[f, 0]) + bg[:, 1:] * (P[f, 2] - P[f, 0])


def random_rays(sc, n=MAX_RAYS, seed=109):
    """As test_trace_matches_oracle: origins uniform in the scene's box grown by 1, unit directions, times in
    [0, 1); two thirds of the directions go toward a random surface point of a random textured entry (where
    it is at the ray's time), the rest are uniform."""
    rng = np.random.default_rng(seed)
    es = textured_entries(sc)
    pts = np.concatenate([_surface_points(sc, e, 64, rng) @ e["M"][:3, :3].T + e["M"][:3, 3] for e in es])
    lo, hi = pts.min(0) - 1, pts.max(0) + 1
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.standard_normal((n, 3))
    t = rng.random(n).astype(f32)
    which = rng.integers(0, len(es), n)
    aimed = rng.random(n) < 2 / 3
    for k, e in enumerate(es):
        m = aimed & (which == k)
        p = _surface_points(sc, e, int(m.sum()), rng)
        pw = p @ e["M"][:3, :3].T + e["M"][:3, 3] + e["blur"][None] * t[m].astype(np.float64)[:, None]
        d[m] = pw - o[m]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(f32), d.astype(f32), t


# ------------------------------------------------------------------------------------------------ trace cases
BUILDERS = {"tex_matrix": functools.partial(tex_matrix, SIZE_SETS["mixed"], blur=True),
            "tri_matrix": tri_matrix,
            "degenerate_uv": degenerate_uv}
RAYS = {"tex_matrix": ("pole_rays", "seam_rays", "texel_edge_rays", "random_rays"),
        "tri_matrix": ("texel_edge_rays", "random_rays"),
        "degenerate_uv": ("random_rays",)}


@functools.lru_cache(maxsize=None)
def reference(builder, gen):
    """((origins, directions, times), the oracle's hit records) of one builder and ray class: computed once,
    shared by the tests that need it and read-only."""
    import pyoracle
    sc = BUILDERS[builder]()
    o, d, t = globals()[gen](sc)
    assert len(o) <= MAX_RAYS
    orc = pyoracle.Oracle(sc)
    ref = orc.trace(o, d, t)
    orc.close()
    for v in (o, d, t, *ref.values()):
        v.setflags(write=False)
    return (o, d, t), ref


# ------------------------------------------------------------------------------------------------ Perlin
PERLIN_TABLE = np.array([(1, 1, 0), (-1, 1, 0), (1, -1, 0), (-1, -1, 0), (1, 0, 1), (-1, 0, 1), (1, 0, -1), (-1, 0, -1),
                         (0, 1, 1), (0, -1, 1), (0, 1, -1), (0, -1, -1), (1, 1, 0), (-1, 1, 0), (0, -1, 1), (0, -1, -1)],
                        np.float64)
PERLIN_SHUFFLED = np.array([12, 7, 15, 6, 11, 0, 4, 9, 13, 3, 14, 8, 2, 5, 1, 10])


def perlin_f64(p, scale, nc):
    """src/Perlin.cpp:27-97 restated in float64 numpy on (n, 3) points: the sum over the cell's eight lattice
    points of gradient . offset times the quintic weights; numpy's % is the non-negative remainder that
    GetFromShuffled's `index < 0` branch produces."""
    pt = np.asarray(p, np.float64) * float(scale)
    base = np.floor(pt).astype(np.int64)
    P = lambda i: PERLIN_SHUFFLED[i % 16]
    w = lambda x: -6 * np.abs(x) ** 5 + 15 * np.abs(x) ** 4 - 10 * np.abs(x) ** 3 + 1
    value = np.zeros(len(pt))
    for i in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                lat = base + np.array([i, j, k])
                g = PERLIN_TABLE[P(lat[:, 0] + P(lat[:, 1] + P(lat[:, 2])))]
                l = pt - lat
                value += (g * l).sum(1) * w(l[:, 0]) * w(l[:, 1]) * w(l[:, 2])
    if nc == A.NC_LINEAR:
        return (value + 1) * 0.5
    if nc == A.NC_ABSVAL:
        return np.abs(value)
    return value
