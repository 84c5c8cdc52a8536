"""float64 closed forms of the reference's Whitted shading, written from src/Light.cpp, src/Scene.cpp,
src/Camera.cpp and src/Material.h (numpy and math only; not a translation of oracle/rtg_oracle.c).  A helper
of tests/test_shading_kat.py and tests/test_gpu_shading_kat.py, not a test.

Scope: scenes whose objects are horizontal rectangles `y = const` (a mesh of coplanar triangles each, huge for
a plane, small for an occluder), so a hit is `t = (y - o.y) / d.y` and no BVH, triangle test or transform can
hide an error of the shading arithmetic.  Scene inputs are rounded to float32 first, as the ABI does, then
widened; everything after that is float64.  The uniforms of the sampled parts (camera jitter, area light,
environment light) come from the oracle's Philox stream through `rng(seed, pixel, sample, path, purpose,
light, iteration, lane)`: Philox is pinned by Random123 vectors and the counter layout is this project's own
choice (pixel `y*nx + x`, sample index, path 1 at the root, `2*path` for the refracted and `2*path + 1` for
the reflected child; purposes 1 camera, 3 area light, 4 environment light).

Left out on purpose:
  * total internal reflection: the reference takes its Beer distance from the hit record of a ray with a NaN
    direction (Scene.cpp:99-110), so the formulas do not determine the value; `render` raises if a case
    reaches it;
  * a transmitted ray that misses: its Beer distance comes from a hit record nobody filled in (the `= {}` of
    src/Helper.cpp:21 leaves the Eigen vectors of src/defs.h:13-22 unset; DESIGN.md §2 lists the oracle's
    choice of (0, 0, 0) among its conventions); `render` raises there too, so the glass scenes are closed
    above and below;
  * rough mirrors, textures (but for a uniform environment map, whose texel lookup cannot matter), motion
    blur, depth of field, instancing and transforms;
  * the path tracer (tests/test_pathtrace.py and tests/test_gpu_pathtrace.py hold it to the furnace).
"""
import math

import numpy as np

from rtg import _abi as A

RNG_CAMERA, RNG_AREA, RNG_ENV = 1, 3, 4
BRDF_EPSILON = 0.001                    # Light::_epsilon (src/Light.h:16), the cut of the "original" BRDFs


def f64(v):
    """A scene input as the ABI hands it on: rounded to float32, then widened."""
    return np.asarray(np.asarray(v, np.float32), np.float64)


def _unit(v):
    return v / math.sqrt(float(v @ v))


def _norm(v):
    return math.sqrt(float(v @ v))


class Rect:
    """One object: the rectangle its coplanar triangles cover, normal by the winding (Shape.cpp:143)."""

    def __init__(self, scene, obj):
        if obj.type != A.OBJ_MESH or obj.xforms or obj.textures or obj.smooth or any(obj.blur):
            raise ValueError("shading_ref: objects are plain untransformed flat meshes")
        pts = f64(scene.vertices)[np.asarray(obj.faces, np.int64).reshape(-1, 3) - 1]     # (F, 3 corners, xyz)
        if not np.all(pts[..., 1] == pts[0, 0, 1]):
            raise ValueError("shading_ref: every object lies in one plane y = const")
        normals = {float(np.sign(np.cross(c - b, a - b)[1])) for a, b, c in pts}
        if len(normals) != 1 or 0.0 in normals:
            raise ValueError("shading_ref: the faces of an object share one winding")
        self.y = float(pts[0, 0, 1])
        self.normal = np.array([0.0, normals.pop(), 0.0])
        self.x0, self.x1 = float(pts[..., 0].min()), float(pts[..., 0].max())
        self.z0, self.z1 = float(pts[..., 2].min()), float(pts[..., 2].max())
        self.material = scene.materials[obj.material - 1]


class Hit:
    def __init__(self, t, point, rect):
        self.t, self.point, self.normal, self.material = t, point, rect.normal, rect.material


def ortho_u(v):
    """GeometryHelpers::GetOrthonormalUVector (src/Helper.cpp:322-342)."""
    a = np.abs(v)
    idx = 0 if (a[0] <= a[1] and a[0] <= a[2]) else (1 if (a[1] <= a[0] and a[1] <= a[2]) else 2)
    nl = v.copy()
    nl[idx] = 1.0
    return _unit(np.cross(v, nl))


class Ref:
    """The reference's renderer over a scene of rectangles.  `rng` is pyoracle.rng_uniform."""

    def __init__(self, scene, rng=None, seed=0x5EED2026):
        if scene.instances:
            raise ValueError("shading_ref: no instances")
        self.scene, self.rng, self.seed = scene, rng, seed
        self.rects = [Rect(scene, o) for o in scene.objects]
        self.eps = float(np.float32(scene.shadow_eps))
        self.ambient = f64(scene.ambient)
        self.depth = int(scene.max_depth)
        self.lights = [self._light(i, l) for i, l in enumerate(scene.lights)]
        self.log = []                   # (pixel, sample, path, kind, values) records for the tests' own checks

    # ------------------------------------------------------------------ constructors (src/Light.cpp)
    def _light(self, index, l):
        d = dict(type=l.type, index=index, pos=f64(l.position), inten=f64(l.intensity))
        if l.type in (A.LIGHT_DIRECTIONAL, A.LIGHT_SPOT):
            d["dir"] = _unit(f64(l.direction))                     # Light.cpp:256-257, 327-330
        if l.type == A.LIGHT_SPOT:                                 # SpotLight::SpotLight Light.cpp:327-336
            d["coverage"] = float(f64(l.coverage_deg)) * 0.5 * (math.pi / 180.0)
            d["fall"] = float(f64(l.falloff_deg)) * 0.5 * (math.pi / 180.0)
        if l.type == A.LIGHT_AREA:                                 # AreaLight::AreaLight Light.cpp:442-455
            d["normal"] = _unit(f64(l.direction))
            d["u"] = ortho_u(d["normal"])
            d["v"] = np.cross(d["normal"], d["u"])
            d["size"] = float(f64(l.size))
        if l.type == A.LIGHT_ENVIRONMENT:
            tex = f64(self.scene.textures[l.texture].texels)
            if not np.all(tex == tex[0, 0]):
                raise ValueError("shading_ref: the environment map is uniform")
            d["texel"] = tex[0, 0]
        return d

    # ------------------------------------------------------------------ intersection
    def intersect(self, o, d):
        """BVHMethods::FindIntersection (src/Helper.cpp:32-51) over rectangles: the nearest `distance > 0`, the
        first object on a tie."""
        best = None
        for r in self.rects:
            if d[1] == 0.0:
                continue
            t = (r.y - o[1]) / d[1]
            if not t > 0.0 or (best is not None and not t < best.t):
                continue
            p = o + d * t
            if r.x0 <= p[0] <= r.x1 and r.z0 <= p[2] <= r.z1:
                best = Hit(t, p, r)
        return best

    # ------------------------------------------------------------------ camera (src/Camera.cpp)
    def _camera(self, cam):
        c = {}
        gaze, up = f64(cam.gaze), f64(cam.up)
        c["gaze"] = _unit(gaze)                                    # the constructor, Camera.cpp:33-42
        w = _unit(gaze) if cam.left_handed else _unit(-gaze)
        c["right"] = _unit(np.cross(up, w))
        c["up"] = np.cross(w, c["right"])
        c["pos"] = f64(cam.position)
        c["l"], c["r"], c["b"], c["t"] = (float(x) for x in f64(cam.near_plane))
        c["dist"] = float(f64(cam.near_distance))
        c["nx"], c["ny"] = cam.nx, cam.ny
        n = 1
        while n * n < cam.num_samples:                             # Camera.cpp:21-28
            n += 1
        c["grid"], c["total"] = n, cam.num_samples
        c["pw"] = (c["r"] - c["l"]) / cam.nx                       # Camera.cpp:45-52
        c["ph"] = (c["t"] - c["b"]) / cam.ny
        return c

    @staticmethod
    def primary_ray(c, col, row):
        """Camera::getPrimaryRay (Camera.cpp:63-72): the pixel centre."""
        u = c["l"] + (c["r"] - c["l"]) * (col + 0.5) / c["nx"]
        v = c["t"] - (c["t"] - c["b"]) * (row + 0.5) / c["ny"]
        m = c["pos"] + c["gaze"] * c["dist"] + u * c["right"] + v * c["up"]
        return c["pos"], _unit(m - c["pos"])

    def sample_ray(self, c, col, row, pixel, s):
        """Camera::PixelLBCorner (Camera.cpp:84-92) and Camera::getSampleRay (Camera.cpp:94-113), no depth of
        field; the ray's time (the third uniform) moves nothing here."""
        u = c["l"] + col * c["pw"]
        v = c["t"] - (row + 1) * c["ph"]
        m = c["pos"] + c["gaze"] * c["dist"] + u * c["right"] + v * c["up"]
        i, j = s % c["grid"], s // c["grid"]
        x_chi = float(self.rng(self.seed, pixel, s, 1, RNG_CAMERA, 0, 0, 0))
        y_chi = float(self.rng(self.seed, pixel, s, 1, RNG_CAMERA, 0, 0, 1))
        m = m + (i + x_chi) * (c["pw"] / c["grid"]) * c["right"] + (j + y_chi) * (c["ph"] / c["grid"]) * c["up"]
        return c["pos"], _unit(m - c["pos"])

    # ------------------------------------------------------------------ BRDFs (src/Light.cpp)
    @staticmethod
    def fresnel_conductor(n_t, k_t, ray, normal):
        """Light::Fresnel (Light.cpp:18-28), the same text as Scene::ConductorFresnel (Scene.cpp:135-146)."""
        cos_t = -float(ray @ normal)
        two = 2 * n_t * cos_t
        c2 = cos_t ** 2
        nk = n_t ** 2 + k_t ** 2
        rs = (nk - two + c2) / (nk + two + c2)
        rp = (nk * c2 - two + 1) / (nk * c2 + two + 1)
        return 0.5 * (rs + rp)

    @staticmethod
    def geometry_ts(wi, wo, wh, n):
        """Light::GeometryTS (Light.cpp:49-60)."""
        left = 2.0 * float(n @ wh) * float(n @ wo) / float(wo @ wh)
        right = 2.0 * float(n @ wh) * float(n @ wi) / float(wi @ wh)
        return min(1.0, min(left, right))

    @staticmethod
    def distribution_ts(cos_alpha, p):
        """Light::DistributionTS (Light.cpp:12-16)."""
        return (p + 2.0) / (2.0 * math.pi) * cos_alpha ** p

    def term_brdf(self, wi, wo, n, m):
        """Light::TermBRDF (Light.cpp:62-155)."""
        kd, ks, p, b = f64(m.diffuse), f64(m.specular), int(m.phong_exp), m.brdf
        if b in (A.BRDF_MP, A.BRDF_OP, A.BRDF_MPN):                # Light.cpp:63-93
            wr = _unit(-wi + n * 2 * float(n @ wi))
            cos_angle = max(0.0, float(wr @ wo))
        elif b in (A.BRDF_MBP, A.BRDF_OBP, A.BRDF_MBPN):           # Light.cpp:94-121
            cos_angle = max(0.0, float(n @ _unit(wo + wi)))
        if b in (A.BRDF_MP, A.BRDF_MBP):
            return kd + ks * cos_angle ** p
        if b in (A.BRDF_OP, A.BRDF_OBP):
            cos_i = max(0.0, float(wi @ n))
            if cos_i < BRDF_EPSILON:
                return np.zeros(3)
            return kd + ks * cos_angle ** p / cos_i
        if b == A.BRDF_MPN:
            return kd / math.pi + ks * ((p + 2) / (2 * math.pi)) * cos_angle ** p
        if b == A.BRDF_MBPN:
            return kd / math.pi + ks * ((p + 8) / (8 * math.pi)) * cos_angle ** p
        if b in (A.BRDF_TS, A.BRDF_TSF):                           # Light.cpp:122-154
            wh = _unit(wo + wi)
            diffuse = kd / math.pi
            cos_alpha, cos_theta, cos_phi = float(wh @ n), float(wi @ n), float(wo @ n)
            spec = ks * self.geometry_ts(wi, wo, wh, n) * self.distribution_ts(cos_alpha, p)
            spec = spec / (4.0 * cos_phi * cos_theta)
            if b == A.BRDF_TSF:
                f = self.fresnel_conductor(float(f64(m.refraction_index)), float(f64(m.absorption_index)), -wo, n)
                diffuse, spec = diffuse * (1 - f), spec * f
            return diffuse + spec
        raise ValueError(f"shading_ref: BRDF {b}")

    def surface(self, radiance, wi, wo, n, m):
        """What every light's BasicShading does with its radiance once the point is lit: Light::BRDF
        (Light.cpp:157-162), or Diffuse + Specular without one (PointLight::Diffuse Light.cpp:206-223,
        PointLight::Specular Light.cpp:225-236; the other lights repeat the text)."""
        if m.brdf != A.BRDF_NONE:
            return radiance * self.term_brdf(wi, wo, n, m) * max(0.0, float(wi @ n))
        diffuse = radiance * (f64(m.diffuse) * max(0.0, float(n @ wi)))
        alpha = max(0.0, float(n @ _unit(wo + wi)))
        return diffuse + radiance * (f64(m.specular) * alpha ** int(m.phong_exp))

    # ------------------------------------------------------------------ shadows and lights (src/Light.cpp)
    def shadow_towards(self, hit, target):
        """PointLight::IsShadow (Light.cpp:188-204), SpotLight::IsShadow (Light.cpp:359-375), AreaLight::IsShadow
        (Light.cpp:473-488): the nearest hit of a ray from `p + n * ShadowRayEpsilon`, compared by distance."""
        d = target - hit.point
        nr = self.intersect(hit.point + hit.normal * self.eps, d / _norm(d))
        return nr is not None and _norm(hit.point - target) > _norm(hit.point - nr.point)

    def shadow_dir(self, hit, direction):
        """DirectionalLight::IsShadow (Light.cpp:270-275), EnvironmentLight::IsShadow (Light.cpp:581-594): any
        hit."""
        return self.intersect(hit.point + hit.normal * self.eps, direction) is not None

    def light_shading(self, L, d, hit, m, key):
        pixel, sample, path = key
        wo, n, p = -d, hit.normal, hit.point
        zero = np.zeros(3)
        if L["type"] == A.LIGHT_POINT:                             # PointLight::BasicShading Light.cpp:238-250
            if self.shadow_towards(hit, L["pos"]):
                return zero
            radiance = L["inten"] / _norm(p - L["pos"]) ** 2       # ComputeLightContribution Light.cpp:178-182
            return self.surface(radiance, _unit(L["pos"] - p), wo, n, m)
        if L["type"] == A.LIGHT_DIRECTIONAL:                       # DirectionalLight::BasicShading Light.cpp:309-321
            if self.shadow_dir(hit, -L["dir"]):
                return zero
            return self.surface(L["inten"], -L["dir"], wo, n, m)
        if L["type"] == A.LIGHT_SPOT:                              # SpotLight::BasicShading Light.cpp:409-436
            if self.shadow_towards(hit, L["pos"]):
                return zero
            angle = math.acos(float(_unit(p - L["pos"]) @ L["dir"]))          # FindAngle Light.cpp:338-341
            self.log.append((pixel, sample, path, "spot", (angle, L["fall"], L["coverage"])))
            if not angle < L["coverage"]:
                return zero
            radiance = L["inten"] / _norm(p - L["pos"]) ** 2
            c = self.surface(radiance, _unit(L["pos"] - p), wo, n, m)
            if angle < L["fall"]:
                return c
            cf, cc = math.cos(L["fall"]), math.cos(L["coverage"])             # FallOf Light.cpp:343-348
            return c * ((math.cos(angle) - cc) / (cf - cc)) ** 4
        if L["type"] == A.LIGHT_AREA:                              # AreaLight::BasicShading Light.cpp:522-545
            u_chi = float(self.rng(self.seed, pixel, sample, path, RNG_AREA, L["index"], 0, 0)) - 0.5
            v_chi = float(self.rng(self.seed, pixel, sample, path, RNG_AREA, L["index"], 0, 1)) - 0.5
            s = L["pos"] + L["u"] * L["size"] * u_chi + L["v"] * L["size"] * v_chi
            if self.shadow_towards(hit, s):
                return zero
            cos_theta = abs(float(_unit(p - s) @ L["normal"]))     # FindAreaFactor Light.cpp:457-463
            radiance = L["inten"] * (L["size"] * L["size"] * (cos_theta / _norm(p - s) ** 2))
            return self.surface(radiance, _unit(s - p), wo, n, m)
        if L["type"] == A.LIGHT_ENVIRONMENT:                       # EnvironmentLight::BasicShading Light.cpp:628-660
            u = ortho_u(n)
            w = np.cross(n, u)
            it = 0
            while True:
                x, y, z = (float(self.rng(self.seed, pixel, sample, path, RNG_ENV, L["index"], it, k)) * 2 - 1.0
                           for k in range(3))
                direction = (p + u * x + n * y + w * z) - p
                length = _norm(direction)
                if abs(length - 1.0) < 1e-5 or abs(float(direction @ n)) < 1e-6:
                    raise ValueError("shading_ref: a rejection test too close to call in float32")
                if float(direction @ n) > 0 and length <= 1:
                    direction = direction / length
                    break
                it += 1
            if self.shadow_dir(hit, direction):
                return zero
            radiance = L["texel"] * 2 * math.pi                    # ComputeLightContribution Light.cpp:563-575
            return self.surface(radiance, direction, wo, n, m)
        raise ValueError("shading_ref: light type")

    def basic_shading(self, d, hit, m, key):
        """Scene::BasicShading (Scene.cpp:243-267) with Scene::ambient (Scene.cpp:22-30)."""
        ambient = self.ambient * f64(m.ambient)
        lit = np.zeros(3)
        for L in self.lights:
            lit = lit + self.light_shading(L, d, hit, m, key)
        self.log.append((key[0], key[1], key[2], "basic", (ambient, lit, hit.point)))
        return ambient + lit

    # ------------------------------------------------------------------ recursion (src/Scene.cpp)
    def reflect(self, o, d, hit):
        """Scene::MirrorReflectance (Scene.cpp:32-55), not rough."""
        wo = -d
        wr = _unit(-wo + hit.normal * 2 * float(hit.normal @ wo))
        ro = hit.point + hit.normal * self.eps
        return ro, wr, self.intersect(ro, wr)

    def recursive_shading(self, o, d, hit, depth, key):
        """Scene::RecursiveShading (Scene.cpp:148-219)."""
        if hit is None:
            return np.zeros(3)                                     # a miss is black, not the background
        pixel, sample, path = key
        m = hit.material
        if m.type == A.MAT_NORMAL or depth <= 0:
            return self.basic_shading(d, hit, m, key)
        refl_key, refr_key = (pixel, sample, 2 * path + 1), (pixel, sample, 2 * path)
        if m.type == A.MAT_MIRROR:
            ro, rd, rh = self.reflect(o, d, hit)
            rc = f64(m.mirror) * self.recursive_shading(ro, rd, rh, depth - 1, refl_key)
            return self.basic_shading(d, hit, m, key) + rc
        if m.type == A.MAT_CONDUCTOR:
            f = self.fresnel_conductor(float(f64(m.refraction_index)), float(f64(m.absorption_index)), d, hit.normal)
            ro, rd, rh = self.reflect(o, d, hit)
            rc = f64(m.mirror) * (f * self.recursive_shading(ro, rd, rh, depth - 1, refl_key))
            return self.basic_shading(d, hit, m, key) + rc
        # Scene::DielectricRefraction (Scene.cpp:57-118)
        nt = float(f64(m.refraction_index))
        entering = float(d @ hit.normal) < 0
        if entering:
            snell, normal, n_t, n_i = 1.0 / nt, hit.normal, nt, 1.0
        else:
            snell, normal, n_t, n_i = nt, -hit.normal, 1.0, nt
        cos_theta = -float(d @ normal)
        root = 1 - snell ** 2 * (1 - cos_theta ** 2)
        if root < 0:
            raise ValueError("shading_ref: total internal reflection is left out")
        td = _unit((d + normal * cos_theta) * snell - normal * math.sqrt(root))
        to = hit.point - self.eps * normal
        th = self.intersect(to, td)
        cos_t, cos_i = -float(td @ normal), -float(d @ normal)     # Scene::FresnelReflectance Scene.cpp:120-128
        r_par = (n_t * cos_i - n_i * cos_t) / (n_t * cos_i + n_i * cos_t)
        r_per = (n_i * cos_i - n_t * cos_t) / (n_i * cos_i + n_t * cos_t)
        fresnel = 0.5 * (r_par ** 2 + r_per ** 2)
        if th is None:
            raise ValueError("shading_ref: a transmitted ray that misses leaves the Beer distance undefined")
        beer = np.exp(-f64(m.absorption_coeff) * _norm(th.point - hit.point))   # Scene::BeerLaw Scene.cpp:130-133
        self.log.append((pixel, sample, path, "dielectric", (entering, fresnel, beer)))
        ro, rd, rh = self.reflect(o, d, hit)
        if entering:                                               # Scene.cpp:169-182
            inside = beer * ((1 - fresnel) * self.recursive_shading(to, td, th, depth - 1, refr_key))
            reflected = fresnel * self.recursive_shading(ro, rd, rh, depth - 1, refl_key)
            return self.basic_shading(d, hit, m, key) + inside + reflected
        outside = (1 - fresnel) * self.recursive_shading(to, td, th, depth - 1, refr_key)   # Scene.cpp:194-207
        reflected = beer * (fresnel * self.recursive_shading(ro, rd, rh, depth - 1, refl_key))
        return outside + reflected

    # ------------------------------------------------------------------ frames (src/Scene.cpp)
    def render(self, camera=0):
        """Scene::SingleSample (Scene.cpp:365-384) or Scene::MultiSample (Scene.cpp:386-411) per pixel.  Every
        camera ray must hit: the background is not part of the closed forms."""
        cam = self.scene.cameras[camera] if isinstance(camera, int) else camera
        if cam.is_dof:
            raise ValueError("shading_ref: no depth of field")
        c = self._camera(cam)
        img = np.zeros((cam.ny, cam.nx, 3))
        self.log = []
        for row in range(cam.ny):
            for col in range(cam.nx):
                pixel = row * cam.nx + col
                total = np.zeros(3)
                for s in range(c["total"]):
                    o, d = self.sample_ray(c, col, row, pixel, s) if c["total"] > 1 else self.primary_ray(c, col, row)
                    hit = self.intersect(o, d)
                    if hit is None:
                        raise ValueError("shading_ref: a camera ray misses the scene")
                    total = total + self.recursive_shading(o, d, hit, self.depth, (pixel, s, 1))
                img[row, col] = total / c["total"]
        if not np.isfinite(img).all():
            raise ValueError("shading_ref: a non-finite value (the reference's NanCheck is not modelled)")
        return img

    def records(self, kind, path=None):
        return [r for r in self.log if r[3] == kind and (path is None or r[2] == path)]
