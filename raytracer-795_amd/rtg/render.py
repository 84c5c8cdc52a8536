"""Host mirror of `Scene::renderScene()` / `Image` over the librtg C ABI.

    sc = rtg.parse_xml("scene.xml")        # new Scene(xml)         (src/Scene.cpp:455)
    rtg.render_scene(sc)                   # pScene->renderScene()  (src/Scene.cpp:294)

`Renderer` keeps the flattened scene resident on one GPU (rtg_scene_create) and renders
cameras into host or device framebuffers; `save_image` writes what Image::saveImage does
(src/Image.cpp:26-107): a P3 text PPM clamped to 255 when the name contains ".png",
otherwise an OpenEXR file (half RGB).
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib

import numpy as np

from . import _abi as A
from .scene import Camera, Scene

DEFAULT_SEED = 0x5EED2026


class Renderer:
    def __init__(self, scene: Scene, device: int = 0, bvh_builder: int = A.RTG_BVH_AUTO, tlas: int = 0,
                 traversal_tree: int = 0, uniform_walk: int = 0):
        self.lib = A.load_library()
        self.scene = scene
        desc, self._keep = scene.to_desc()
        h = C.c_void_p()
        bo = A.BuildOpts(bvh_builder, tlas, traversal_tree, uniform_walk)
        A.check(self.lib.rtg_scene_create_ex(C.byref(desc), int(device), C.byref(bo), C.byref(h)), self.lib)
        self.handle = h
        self.device = device
        self._frames = []

    def close(self):
        if getattr(self, "handle", None):
            for f in list(getattr(self, "_frames", ())):      # a scene with live frames refuses to go
                f.close()
            self.lib.rtg_scene_destroy(self.handle)
            self.handle = None

    def frame(self, camera: Camera | int = 0, first_sample: int = 0, sample_count: int = 0, moments: bool = False,
              order: int = 0, **kw) -> "Frame":
        """A progressive frame of `camera` (rtg_frame): samples first_sample ..
        first_sample + sample_count - 1 of its num_samples (0 = through the last), added in chunks
        with Frame.add; order 1 spreads every prefix over the pixel (§15); `kw`: the render options."""
        cam = self.scene.cameras[camera] if isinstance(camera, int) else camera
        return Frame(self, cam, first_sample, sample_count, moments, self.opts(**kw), order)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @staticmethod
    def opts(seed=DEFAULT_SEED, row_offset=0, row_stride=1, traversal=0, max_batch_rays=0, collect_stats=0,
             collect_timing=0, streams=0, row_block=1, compact_rows=0, num_devices=0, devices=None, schedule=0,
             tile_band=0, segment_pixels=0, segment_nodes=0):
        o = A.RenderOpts()
        o.schedule = schedule
        o.tile_band, o.segment_pixels, o.segment_nodes = tile_band, segment_pixels, segment_nodes
        o.seed = seed
        o.row_offset, o.row_stride, o.row_block = row_offset, row_stride, row_block
        o.traversal = traversal
        o.max_batch_rays = max_batch_rays
        o.collect_stats = collect_stats
        o.collect_timing = collect_timing
        o.streams = streams
        o.compact_rows = compact_rows
        o.num_devices = num_devices
        if devices is not None:
            arr = (C.c_int32 * len(devices))(*devices)
            o.devices = C.cast(arr, C.POINTER(C.c_int32))
            o._devices_keepalive = arr
        return o

    def render(self, camera: Camera | int = 0, **kw) -> np.ndarray:
        cam = self.scene.cameras[camera] if isinstance(camera, int) else camera
        o = self.opts(**kw)
        rows = (self.lib.rtg_shard_rows(cam.ny, o.row_offset, o.row_stride, o.row_block) if o.compact_rows
                else cam.ny)
        out = np.empty((rows, cam.nx, 3), np.float32)
        cd = cam.desc()
        A.check(self.lib.rtg_render(self.handle, C.byref(cd), C.byref(o), out.ctypes.data_as(A.PF)), self.lib)
        return out

    def render_device(self, camera: Camera | int, out_ptr: int, stream: int = 0, **kw):
        """Render into caller-owned device memory (e.g. a torch CUDA tensor's data_ptr)."""
        cam = self.scene.cameras[camera] if isinstance(camera, int) else camera
        cd = cam.desc()
        o = self.opts(**kw)
        A.check(self.lib.rtg_render_device(self.handle, C.byref(cd), C.byref(o), C.c_void_p(out_ptr),
                                           C.c_void_p(stream)), self.lib)

    def render_ranked(self, camera: Camera | int, comm: "Comm", frame_ptr: int, stream: int = 0, **kw):
        """One rank of a one-process-per-GPU render (rtg_render_ranked): this rank's row-block shard,
        gathered over RCCL into `frame_ptr` (device memory, rank 0; other ranks may pass 0)."""
        cam = self.scene.cameras[camera] if isinstance(camera, int) else camera
        cd = cam.desc()
        o = self.opts(**kw)
        A.check(self.lib.rtg_render_ranked(self.handle, C.byref(cd), C.byref(o), comm.handle,
                                           C.c_void_p(frame_ptr or None), C.c_void_p(stream)), self.lib)

    def stats(self) -> dict:
        s = A.RenderStats()
        A.check(self.lib.rtg_last_render_stats(self.handle, C.byref(s)), self.lib)
        return {k: (list(v) if isinstance(v, C.Array) else v)
                for k, v in ((k, getattr(s, k)) for k, _ in A.RenderStats._fields_)}

    def trace(self, origins: np.ndarray, directions: np.ndarray, times=None, traversal=0) -> dict:
        n = len(origins)
        rays = (A.Ray * max(n, 1))()
        o = np.asarray(origins, np.float32).reshape(-1, 3)
        d = np.asarray(directions, np.float32).reshape(-1, 3)
        t = np.zeros(n, np.float32) if times is None else np.asarray(times, np.float32)
        buf = np.frombuffer(rays, dtype=np.float32, count=7 * max(n, 1)).reshape(-1, 7)
        buf[:n, 0:3], buf[:n, 3:6], buf[:n, 6] = o, d, t
        hits = (A.Hit * max(n, 1))()
        A.check(self.lib.rtg_trace_closest(self.handle, rays, n, hits, traversal), self.lib)
        return hits_to_dict(hits, n)

    def build_stats(self) -> dict:
        b = A.BuildStats()
        A.check(self.lib.rtg_scene_build_stats(self.handle, C.byref(b)), self.lib)
        return {k: getattr(b, k) for k, _ in A.BuildStats._fields_}

    def bvh(self, obj: int):
        return _bvh(self.lib.rtg_scene_object_bvh, self.handle, obj)

    def matrices(self, top: int):
        inv = np.zeros(16, np.float32)
        it = np.zeros(16, np.float32)
        A.check(self.lib.rtg_scene_object_matrices(self.handle, top, inv.ctypes.data_as(A.PF),
                                                   it.ctypes.data_as(A.PF)), self.lib)
        return inv, it

    def vertex_normals(self):
        out = np.zeros((len(self.scene.vertices), 3), np.float32)
        A.check(self.lib.rtg_scene_vertex_normals(self.handle, out.ctypes.data_as(A.PF)), self.lib)
        return out


def hits_to_dict(hits, n: int) -> dict:
    raw = np.frombuffer(hits, dtype=np.int32, count=11 * max(n, 1)).reshape(-1, 11)[:n]
    f = raw.view(np.float32)
    return {"full": raw[:, 0].copy(), "object": raw[:, 1].copy(), "prim": raw[:, 2].copy(),
            "material": raw[:, 3].copy(), "t": f[:, 4].copy(), "point": f[:, 5:8].copy(),
            "normal": f[:, 8:11].copy()}


# ---------------------------------------------------------------------------- Image
def _is_png(name: str) -> bool:
    """Image::IsPNG (src/Image.cpp:36-60): the substring ".png" anywhere in the name."""
    c = 0
    for ch in name:
        if ch == ".":
            c = 1
        elif ch == "p" and c == 1:
            c = 2
        elif ch == "n" and c == 2:
            c = 3
        elif ch == "g" and c == 3:
            return True
        else:
            c = 0
    return False


def ppm_p3_bytes(rgb: np.ndarray) -> bytes:
    """Image::SavePng (src/Image.cpp:62-103): values > 255 clamped, (unsigned char) cast,
    P3 text with a trailing space after every value and a newline per row."""
    h, w, _ = rgb.shape
    v = np.asarray(rgb, np.float32).copy()
    v[v > 255] = 255
    # (unsigned char)_data[i] (src/Image.cpp:96) as x86-64 gcc compiles it: cvttss2si to a 32-bit
    # int (truncation toward zero), low byte kept: -1 -> 255, -255.5 -> 1, -300 -> 212; NaN and
    # values below -2^31 give 0x80000000 -> 0
    ok = v >= np.float32(-2147483648.0)
    u8 = np.where(ok, np.trunc(np.where(ok, v, 0)), 0).astype(np.int64) & 0xFF
    lines = [f"P3\n{w} {h}\n255\n"]
    for y in range(h):
        lines.append(" ".join(str(int(x)) for x in u8[y].reshape(-1)) + " \n")
    return "".join(lines).encode()


def exr_half_bytes(rgb: np.ndarray) -> bytes:
    """Minimal scanline OpenEXR, ZIP compression off, HALF B/G/R channels (what
    ExrLibrary::SaveExr requests, src/Helper.cpp:361-412)."""
    h, w, _ = rgb.shape
    half = np.asarray(rgb, np.float32).astype(np.float16)

    def attr(name, typ, data):
        return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(data)) + data

    chl = b""
    for ch in ("B", "G", "R"):
        chl += ch.encode() + b"\0" + struct.pack("<iB3xii", 1, 0, 1, 1)
    chl += b"\0"
    hdr = b"\x76\x2f\x31\x01" + struct.pack("<i", 2)
    hdr += attr("channels", "chlist", chl)
    hdr += attr("compression", "compression", b"\0")
    hdr += attr("dataWindow", "box2i", struct.pack("<iiii", 0, 0, w - 1, h - 1))
    hdr += attr("displayWindow", "box2i", struct.pack("<iiii", 0, 0, w - 1, h - 1))
    hdr += attr("lineOrder", "lineOrder", b"\0")
    hdr += attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
    hdr += attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0))
    hdr += attr("screenWindowWidth", "float", struct.pack("<f", 1.0))
    hdr += b"\0"
    table_off = len(hdr)
    line_bytes = w * 2 * 3
    first = table_off + 8 * h
    offsets = b"".join(struct.pack("<Q", first + y * (8 + line_bytes)) for y in range(h))
    body = bytearray()
    for y in range(h):
        body += struct.pack("<ii", y, line_bytes)
        for c in (2, 1, 0):
            body += half[y, :, c].astype("<f2").tobytes()
    return hdr + offsets + bytes(body)


def save_image(name: str, rgb: np.ndarray) -> str:
    """Image::saveImage (src/Image.cpp:26-34)."""
    data = ppm_p3_bytes(rgb) if _is_png(name) else exr_half_bytes(rgb)
    with open(name, "wb") as fh:
        fh.write(data)
    return name


def tonemap(img: np.ndarray, key=0.18, burn=1.0, saturation=1.0, gamma=2.2, device: int = 0) -> np.ndarray:
    """hw5 Photographic tone mapping on the GPU (rtg_tonemap): 0..255 floats."""
    lib = A.load_library()
    a = np.ascontiguousarray(img, np.float32)
    out = np.zeros_like(a)
    tm = A.TonemapDesc(A.TMO_PHOTOGRAPHIC, key, burn, saturation, gamma)
    A.check(lib.rtg_tonemap(device, a.ctypes.data_as(A.PF), a.shape[1], a.shape[0], C.byref(tm),
                            out.ctypes.data_as(A.PF)), lib)
    return out


def tonemapped_name(name: str) -> str:
    """Where a camera's tone-mapped image goes: its ImageName with the extension set to .png."""
    stem, _ = os.path.splitext(name)
    return stem + ".png"


class Comm:
    """An RCCL communicator of librtg (rtg_comm_init_rank) for rtg_render_ranked."""

    @staticmethod
    def unique_id() -> bytes:
        lib = A.load_library()
        buf = (C.c_uint8 * A.RTG_COMM_ID_BYTES)()
        A.check(lib.rtg_comm_unique_id(buf), lib)
        return bytes(buf)

    def __init__(self, uid: bytes, nranks: int, rank: int, device: int, timeout_ms: int = 0):
        """timeout_ms bounds every wait of this rank (set-up, failure agreement, gather; the latter two
        count from this rank's shard end, so the bound must cover the peers' remaining render time); 0 = no
        deadline.  With a bound, a rank whose peers do not join returns an error instead of hanging."""
        self.lib = A.load_library()
        if len(uid) != A.RTG_COMM_ID_BYTES:
            raise ValueError("communicator id must be 128 bytes")
        buf = (C.c_uint8 * A.RTG_COMM_ID_BYTES).from_buffer_copy(uid)
        h = C.c_void_p()
        A.check(self.lib.rtg_comm_init_rank_timeout(buf, int(nranks), int(rank), int(device), int(timeout_ms),
                                                    C.byref(h)), self.lib)
        self.handle = h
        self.rank, self.nranks, self.device = rank, nranks, device

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rtg_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_scene(scene: Scene, out_dir: str | None = None, device: int = 0, seed: int = DEFAULT_SEED, aov: bool = False, denoise: bool = False) -> list:
    """Scene::renderScene (src/Scene.cpp:294-363): every camera rendered and saved.  A camera
    with a hw5 <Tonemap> also gets its tone-mapped image (tonemapped_name; a .png ImageName is
    written tone-mapped instead of clamped)."""
    written = []
    print("BVH construction complete.")
    with Renderer(scene, device) as r:
        for cam in scene.cameras:
            den = _render_denoised(r, cam, seed) if denoise else None     # rtg_cli --denoise
            img = r.render(cam, seed=seed) if den is None else den[0]
            name = cam.image_name if out_dir is None else os.path.join(out_dir, os.path.basename(cam.image_name))
            tm = None if cam.tonemap is None else tonemap(img, *cam.tonemap, device=device)
            if tm is None or not _is_png(name):
                written.append(save_image(name, img))
            if tm is not None:
                written.append(save_image(tonemapped_name(name), tm))
            if aov:      # rtg_cli --aov: the feature images over the camera's full sample range
                for suffix, data in aov_images(r.aov(cam, seed=seed)):
                    written.append(save_image(aov_name(name, suffix), data))
            if den is not None:
                written.append(save_image(denoised_name(name), den[1]))
    return written


def _render_denoised(r: Renderer, cam: Camera, seed: int):
    """(image, denoised image) of a camera through one frame with moments: all samples added at once
    resolve to Renderer.render's bits."""
    with r.frame(cam, moments=True, seed=seed) as f:
        f.add(cam.num_samples)
        return f.resolve(), f.denoise()


def aov_name(name: str, suffix: str) -> str:
    """Where a camera's feature image goes: `suffix` before its ImageName's extension."""
    stem, ext = os.path.splitext(name)
    return stem + suffix + ext


def aov_images(a: dict) -> list:
    """The feature images rtg_cli --aov writes, as (suffix, (ny, nx, 3) float32): the normal as
    (n * 0.5 + 0.5) * 255, the albedo * 255 and the depth in all three channels."""
    half, full = np.float32(0.5), np.float32(255.0)
    return [("_normal", (a["normal"] * half + half) * full), ("_albedo", a["albedo"] * full),
            ("_depth", np.repeat(a["depth"][:, :, None], 3, axis=2))]


def _bvh(fn, handle, obj):
    npr, nn = C.c_int32(), C.c_int32()
    A.check(fn(handle, obj, C.byref(npr), C.byref(nn), None, None, None))
    perm = np.zeros(max(npr.value, 1), np.int32)
    nodes = np.zeros((max(nn.value, 1), 4), np.int32)
    boxes = np.zeros((max(nn.value, 1), 6), np.float32)
    A.check(fn(handle, obj, None, None, perm.ctypes.data_as(A.PI), nodes.ctypes.data_as(A.PI),
               boxes.ctypes.data_as(A.PF)))
    return perm[:npr.value], nodes[:nn.value], boxes[:nn.value]


class Frame:
    """One camera's resumable accumulator on the GPU (rtg_frame).  Any chunking of the samples
    resolves to the same bits; over the whole camera that is Renderer.render's image.

        with r.frame(0, moments=True) as f:
            f.add(16)
            while f.samples_done < total and f.error()["mean_sem"] > tol: f.add(16)
            img = f.resolve()
    """

    def __init__(self, renderer: Renderer, cam: Camera, first_sample: int, sample_count: int, moments: bool, opts,
                 order: int = 0):
        self.lib = renderer.lib
        self.renderer = renderer
        self.camera = cam
        self.opts = opts
        self.has_moments = bool(moments)
        self.handle = None
        fo = A.FrameOpts(int(first_sample), int(sample_count), int(self.has_moments), int(order))
        cd = cam.desc()
        h = C.c_void_p()
        A.check(self.lib.rtg_frame_create(renderer.handle, C.byref(cd), C.byref(opts), C.byref(fo), C.byref(h)),
                self.lib)
        self.handle = h
        self.rows = self.lib.rtg_shard_rows(cam.ny, opts.row_offset, opts.row_stride, opts.row_block)
        renderer._frames.append(self)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rtg_frame_destroy(self.handle)
            self.handle = None
            if self in self.renderer._frames:
                self.renderer._frames.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def add(self, n: int, stream: int = 0) -> int:
        """Trace the next n samples of every owned pixel; returns samples_done."""
        A.check(self.lib.rtg_frame_add_samples(self.handle, int(n), C.c_void_p(stream)), self.lib)
        return self.samples_done

    @property
    def samples_done(self) -> int:
        return int(self.lib.rtg_frame_samples_done(self.handle))

    def resolve(self) -> np.ndarray:
        rows = self.rows if self.opts.compact_rows else self.camera.ny
        out = np.empty((rows, self.camera.nx, 3), np.float32)
        A.check(self.lib.rtg_frame_resolve(self.handle, out.ctypes.data_as(A.PF)), self.lib)
        return out

    def resolve_device(self, out_ptr: int, stream: int = 0):
        A.check(self.lib.rtg_frame_resolve_device(self.handle, C.c_void_p(out_ptr), C.c_void_p(stream)), self.lib)

    def moments(self):
        """(mean, variance) of the samples' luminance per owned pixel, (rows_owned, nx) float32 each."""
        mean = np.empty((self.rows, self.camera.nx), np.float32)
        var = np.empty_like(mean)
        A.check(self.lib.rtg_frame_moments(self.handle, mean.ctypes.data_as(A.PF), var.ctypes.data_as(A.PF)), self.lib)
        return mean, var

    def error(self) -> dict:
        e = A.FrameError()
        A.check(self.lib.rtg_frame_error_stats(self.handle, C.byref(e)), self.lib)
        return {k: getattr(e, k) for k, _ in A.FrameError._fields_}

    def state(self) -> dict:
        """A checkpoint for restore(): samples_done, the raw sums and (with moments) mean / M2."""
        sums = np.zeros((self.rows, self.camera.nx, 3), np.float32)
        mom = np.zeros((self.rows, self.camera.nx, 2), np.float32) if self.has_moments else None
        A.check(self.lib.rtg_frame_get_state(self.handle, sums.ctypes.data_as(A.PF),
                                             None if mom is None else mom.ctypes.data_as(A.PF)), self.lib)
        st = {"samples_done": self.samples_done, "sums": sums, "moments": mom}
        if self.active < self.rows * self.camera.nx:
            st["counts"], st["retired"] = self.counts()
        return st

    def restore(self, state: dict):
        sums = np.ascontiguousarray(state["sums"], np.float32)
        mom = None if state.get("moments") is None else np.ascontiguousarray(state["moments"], np.float32)
        if sums.size != self.rows * self.camera.nx * 3 or (mom is not None and mom.size != self.rows * self.camera.nx * 2):
            raise ValueError("frame state of another size")
        A.check(self.lib.rtg_frame_set_state(self.handle, int(state["samples_done"]), sums.ctypes.data_as(A.PF),
                                             None if mom is None else mom.ctypes.data_as(A.PF)), self.lib)
        if state.get("retired") is not None:
            cnt = np.ascontiguousarray(state["counts"], np.int32)
            ret = np.ascontiguousarray(state["retired"], np.uint8)
            if cnt.size != self.rows * self.camera.nx or ret.size != cnt.size:
                raise ValueError("frame state of another size")
            A.check(self.lib.rtg_frame_set_retired(self.handle, cnt.ctypes.data_as(A.PI), ret.ctypes.data), self.lib)

    # ---- adaptive sampling: retired pixels keep their samples and are traced no further
    @property
    def active(self) -> int:
        """Owned pixels that add() still traces."""
        return int(self.lib.rtg_frame_active_pixels(self.handle))

    def retire(self, rel_tol: float = 0.0, abs_tol: float = 0.0, min_samples: int = 2) -> int:
        """Retire every active pixel whose standard error is at most max(abs_tol, rel_tol * its mean
        luminance), once samples_done >= max(min_samples, 2); returns the active pixels left."""
        a = A.FrameAdapt(float(rel_tol), float(abs_tol), int(min_samples), 0)
        n = C.c_int32()
        A.check(self.lib.rtg_frame_retire(self.handle, C.byref(a), C.byref(n)), self.lib)
        return n.value

    def retire_mask(self, mask) -> int:
        """Retire the active pixels where `mask` (owned-row shape) is set; returns the active pixels left."""
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        if m.size != self.rows * self.camera.nx:
            raise ValueError("mask of another size")
        n = C.c_int32()
        A.check(self.lib.rtg_frame_retire_mask(self.handle, m.ctypes.data, C.byref(n)), self.lib)
        return n.value

    def counts(self):
        """(counts, retired): samples held per owned pixel (int32) and the retired flags (bool)."""
        cnt = np.zeros((self.rows, self.camera.nx), np.int32)
        ret = np.zeros((self.rows, self.camera.nx), np.uint8)
        A.check(self.lib.rtg_frame_sample_counts(self.handle, cnt.ctypes.data_as(A.PI), ret.ctypes.data), self.lib)
        return cnt, ret.astype(bool)


# ---------------------------------------------------------------------------- feature buffers
def _renderer_aov(self, camera: Camera | int = 0, first_sample: int = 0, sample_count: int = 0, **kw) -> dict:
    """First-hit feature buffers of `camera` over samples first_sample .. first_sample + sample_count - 1
    (0 = through the last) of its primary rays (rtg_render_aov): `hits` (ny, nx) int32, the samples that
    hit; `depth` (ny, nx), `normal` and `albedo` (ny, nx, 3) float32, their in-order means over the hit
    samples; `object`, `prim`, `material` (ny, nx) int32 of the window's first sample (-1, -1, 0 for a
    miss).  `kw`: the render options (seed, row shards, compact_rows, traversal); layout as render()."""
    cam = self.scene.cameras[camera] if isinstance(camera, int) else camera
    o = self.opts(**kw)
    rows = (self.lib.rtg_shard_rows(cam.ny, o.row_offset, o.row_stride, o.row_block) if o.compact_rows
            else cam.ny)
    hits = np.empty((rows, cam.nx), np.int32)
    depth = np.empty((rows, cam.nx), np.float32)
    normal = np.empty((rows, cam.nx, 3), np.float32)
    albedo = np.empty((rows, cam.nx, 3), np.float32)
    ids = np.empty((rows, cam.nx, 3), np.int32)
    ao = A.AovOpts(int(first_sample), int(sample_count))
    bufs = A.AovBuffers(hits.ctypes.data_as(A.PI), depth.ctypes.data_as(A.PF), normal.ctypes.data_as(A.PF),
                        albedo.ctypes.data_as(A.PF), ids.ctypes.data_as(A.PI))
    cd = cam.desc()
    A.check(self.lib.rtg_render_aov(self.handle, C.byref(cd), C.byref(o), C.byref(ao), C.byref(bufs)), self.lib)
    return {"hits": hits, "depth": depth, "normal": normal, "albedo": albedo,
            "object": ids[:, :, 0].copy(), "prim": ids[:, :, 1].copy(), "material": ids[:, :, 2].copy()}


def _renderer_camera_rays(self, camera: Camera | int = 0, first_sample: int = 0, sample_count: int = 0,
                          seed: int = DEFAULT_SEED):
    """(origins, directions, times) of the camera's primary rays as the renderer forms them under `seed`
    (rtg_camera_rays): (ny, nx, count, 3) and (ny, nx, count) float32, sample first_sample + j at [y, x, j];
    reshaped to (-1, 3) / (-1) they are ready for Renderer.trace and the oracle's trace."""
    cam = self.scene.cameras[camera] if isinstance(camera, int) else camera
    count = int(sample_count) if sample_count > 0 else max(cam.num_samples - int(first_sample), 0)
    n = cam.ny * cam.nx * count
    rays = (A.Ray * max(n, 1))()
    cd = cam.desc()
    A.check(self.lib.rtg_camera_rays(self.handle, C.byref(cd), int(seed), int(first_sample), int(sample_count), rays),
            self.lib)
    buf = np.frombuffer(rays, dtype=np.float32, count=7 * max(n, 1)).reshape(-1, 7)[:n]
    shape = (cam.ny, cam.nx, count)
    return (buf[:, 0:3].reshape(*shape, 3).copy(), buf[:, 3:6].reshape(*shape, 3).copy(), buf[:, 6].reshape(shape).copy())


# (methods of Renderer, defined here so that the lines above them stay where they are)
Renderer.aov = _renderer_aov
Renderer.camera_rays = _renderer_camera_rays


# ---------------------------------------------------------------------------- denoiser
def denoise(img: np.ndarray, normal: np.ndarray, depth: np.ndarray, albedo=None, variance=None, iterations: int = 0,
            sigma_l: float = 0.0, sigma_z: float = 0.0, normal_power_log2: int = 0, device: int = 0) -> np.ndarray:
    """Edge-avoiding à-trous filter on the GPU (rtg_denoise): `img` (ny, nx, 3) guided by Renderer.aov's
    `normal` (ny, nx, 3) and `depth` (ny, nx); `albedo` (ny, nx, 3) demodulates, `variance` (ny, nx), the
    variance of each pixel's mean luminance, opens the luminance stop.  An option of 0 takes its default
    (5 iterations, sigma_l 4, sigma_z 1, normal power 2^6)."""
    lib = A.load_library()
    a = np.ascontiguousarray(img, np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("image must be (ny, nx, 3)")
    ny, nx = a.shape[:2]

    def guide(v, shape, what):
        if v is None:
            return None
        v = np.ascontiguousarray(v, np.float32)
        if v.shape != shape:
            raise ValueError(f"{what} must be {shape}")
        return v

    n = guide(normal, (ny, nx, 3), "normal")
    z = guide(depth, (ny, nx), "depth")
    al = guide(albedo, (ny, nx, 3), "albedo")
    var = guide(variance, (ny, nx), "variance")
    if n is None or z is None:
        raise ValueError("normal and depth are required")
    out = np.zeros_like(a)
    ptr = lambda v: None if v is None else v.ctypes.data_as(A.PF)
    di = A.DenoiseInputs(ptr(a), ptr(n), ptr(z), ptr(al), ptr(var))
    do = A.DenoiseOpts(int(iterations), float(sigma_l), float(sigma_z), int(normal_power_log2))
    A.check(lib.rtg_denoise(int(device), C.byref(di), nx, ny, C.byref(do), out.ctypes.data_as(A.PF)), lib)
    return out


def denoised_name(name: str) -> str:
    """Where a camera's denoised image goes: _denoised before its ImageName's extension."""
    return aov_name(name, "_denoised")


def _denoise_opts(iterations: int = 0, sigma_l: float = 0.0, sigma_z: float = 0.0, normal_power_log2: int = 0):
    return A.DenoiseOpts(int(iterations), float(sigma_l), float(sigma_z), int(normal_power_log2))


def _frame_denoise(self, demodulate: bool = True, resident: bool = False, **opts) -> np.ndarray:
    """The frame's resolve() filtered by rtg.denoise under the camera's first-hit guides (Renderer.aov over
    its whole sample range, the frame's seed and traversal).  With moments and at least two samples the
    luminance stop runs on moments()[1] / counts()[0], the variance of each pixel's mean (0 for a pixel with
    fewer than two samples).  `opts`: denoise's options.  Whole, uncompacted frames only.
    resident=True computes the same bits without leaving the device (rtg_frame_denoise): the
    guides are traced by the frame's first such call and kept, the filter's workspace stays with the frame."""
    if resident:
        out = np.empty((self.camera.ny, self.camera.nx, 3), np.float32)
        do = _denoise_opts(**opts)
        A.check(self.lib.rtg_frame_denoise(self.handle, C.byref(do), int(bool(demodulate)), out.ctypes.data_as(A.PF)),
                self.lib)
        return out
    o = self.opts
    if o.compact_rows or o.row_stride > 1 or self.rows != self.camera.ny or o.num_devices > 0 or bool(o.devices):
        raise ValueError("Frame.denoise needs a whole frame: not sharded, not compact")
    if self.samples_done < 1:
        raise ValueError("Frame.denoise on a frame without samples")
    img = self.resolve()
    g = self.renderer.aov(self.camera, seed=o.seed, traversal=o.traversal)
    var = None
    if self.has_moments and self.samples_done >= 2:
        cnt = self.counts()[0]
        var = (self.moments()[1] / np.maximum(cnt, 1).astype(np.float32)).astype(np.float32)
        var[cnt < 2] = 0
    return denoise(img, g["normal"], g["depth"], g["albedo"] if demodulate else None, var, device=self.renderer.device,
                   **opts)


def _frame_denoise_device(self, out_ptr: int, stream: int = 0, demodulate: bool = True, **opts):
    """denoise(resident=True) into caller-owned device memory (ny * nx * 3 floats, e.g. a torch tensor's
    data_ptr), enqueued behind `stream`; synchronous on return (rtg_frame_denoise_device)."""
    do = _denoise_opts(**opts)
    A.check(self.lib.rtg_frame_denoise_device(self.handle, C.byref(do), int(bool(demodulate)), C.c_void_p(out_ptr),
                                              C.c_void_p(stream)), self.lib)


def _frame_guides_device(self, rgb: int = 0, normal: int = 0, depth: int = 0, albedo: int = 0, variance: int = 0,
                         stream: int = 0):
    """Copy what the resident filter reads at the frame's current state into caller-owned device arrays
    (raw pointers, 0 = not wanted): rgb, normal, albedo (ny * nx * 3 floats), depth, variance (ny * nx)."""
    g = A.FrameGuides(*(C.c_void_p(p or None) for p in (rgb, normal, depth, albedo, variance)))
    A.check(self.lib.rtg_frame_guides_device(self.handle, C.byref(g), C.c_void_p(stream)), self.lib)


Frame.denoise = _frame_denoise
Frame.denoise_device = _frame_denoise_device
Frame.guides_device = _frame_guides_device


# ---------------------------------------------------------------------------- ray queries
def _renderer_occluded(self, origins, directions, tmax=None, times=None, traversal: int = 0) -> np.ndarray:
    """Occlusion query (rtg_trace_occluded): a bool per ray, True iff trace() reports a hit with t < tmax for
    it.  `tmax`: None (+inf), a scalar or one value per ray, in trace()'s `t` units; NaN, 0 or negative: False."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    n = len(o)
    rays = (A.Ray * max(n, 1))()
    buf = np.frombuffer(rays, dtype=np.float32, count=7 * max(n, 1)).reshape(-1, 7)
    buf[:n, 0:3], buf[:n, 3:6] = o, d
    buf[:n, 6] = 0 if times is None else np.asarray(times, np.float32)
    tm = None
    if tmax is not None:
        tm = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
    out = np.zeros(max(n, 1), np.uint8)
    A.check(self.lib.rtg_trace_occluded(self.handle, rays, None if tm is None else tm.ctypes.data_as(A.PF), n,
                                        out.ctypes.data_as(C.POINTER(C.c_uint8)), int(traversal)), self.lib)
    return out[:n] != 0


def _renderer_trace_device(self, rays_ptr: int, n: int, hits_ptr: int, stream: int = 0, traversal: int = 0):
    """trace() on caller-owned device arrays (rtg_trace_closest_device), enqueued on `stream`, synchronous on
    return.  The torch shapes that carry the C layouts: rays a contiguous float32 (n, 7) tensor (rtg_ray, 28 B:
    origin, direction, time), hits an int32 (n, 11) tensor (rtg_hit, 44 B: full, object, prim, material, then
    t, point, normal in columns 4..10, to be viewed as float32); pass their data_ptr().  hits_to_dict reads
    the host copy: hits_to_dict(hits.cpu().numpy(), n)."""
    A.check(self.lib.rtg_trace_closest_device(self.handle, C.c_void_p(rays_ptr or None), int(n),
                                              C.c_void_p(hits_ptr or None), int(traversal), C.c_void_p(stream)),
            self.lib)


def _renderer_occluded_device(self, rays_ptr: int, n: int, out_ptr: int, tmax_ptr: int = 0, stream: int = 0,
                              traversal: int = 0):
    """occluded() on caller-owned device arrays (rtg_trace_occluded_device): rays as for trace_device, `out` a
    uint8 (n,) tensor (1 = occluded), `tmax` a float32 (n,) tensor or 0 for +inf."""
    A.check(self.lib.rtg_trace_occluded_device(self.handle, C.c_void_p(rays_ptr or None), C.c_void_p(tmax_ptr or None),
                                               int(n), C.c_void_p(out_ptr or None), int(traversal),
                                               C.c_void_p(stream)), self.lib)


# ---------------------------------------------------------------------------- scene updates
def _renderer_update(self, scene: Scene):
    """Move the resident scene to `scene` in place (rtg_scene_update): transforms, blur vectors, material
    assignments and tables, lights and the scene scalars may differ from the scene this Renderer was built
    from; geometry, textures, object counts and intersection_test_eps may not (RtgError, RTG_ERR_UNSUPPORTED,
    naming the field).  Only the top level is rebuilt and uploaded: every later call gives the bits of a fresh
    Renderer(scene).  Frames of this Renderer must be closed first."""
    desc, keep = scene.to_desc(geometry=False)
    A.check(self.lib.rtg_scene_update(self.handle, C.byref(desc)), self.lib)
    self.scene = scene
    self._keep = keep


def _renderer_top_hash(self) -> int:
    """rtg_scene_top_hash: a 64-bit fingerprint of the scene's top level as built or last updated."""
    h = C.c_uint64()
    A.check(self.lib.rtg_scene_top_hash(self.handle, C.byref(h)), self.lib)
    return int(h.value)


Renderer.update = _renderer_update
Renderer.top_hash = _renderer_top_hash
Renderer.occluded = _renderer_occluded
Renderer.trace_device = _renderer_trace_device
Renderer.occluded_device = _renderer_occluded_device


# ---------------------------------------------------------------------------- caller-supplied primary rays
def _ray_image(nx: int, ny: int, num_samples: int, integrator: int, pt_flags: int):
    return A.RayImage(int(nx), int(ny), int(num_samples), int(integrator), int(pt_flags))


def _renderer_render_rays(self, origins, directions, times=None, integrator: int = 0, pt_flags: int = 0, **kw) -> np.ndarray:
    """Render caller-supplied primary rays (rtg_render_rays): `origins` and `directions` (ny, nx, ns, 3), `times`
    (ny, nx, ns) or None (0) -- the shapes camera_rays returns; sample s of pixel (x, y) at [y, x, s].  The
    integrator (0 the reference's, 1 the path tracer with `pt_flags`) runs over them with everything below
    level 0 as render() has it for a camera of that size and sample count: a camera's own rays under the same
    seed give render()'s bits.  Directions are used as given (supply unit vectors).  `kw`: the render options;
    returns (rows, nx, 3) float32 as render()."""
    o = np.asarray(origins, np.float32)
    d = np.asarray(directions, np.float32)
    if o.ndim != 4 or o.shape[3] != 3 or d.shape != o.shape:
        raise ValueError("origins and directions must both be (ny, nx, ns, 3)")
    ny, nx, ns = o.shape[:3]
    t = np.zeros((ny, nx, ns), np.float32) if times is None else np.asarray(times, np.float32)
    if t.shape != (ny, nx, ns):
        raise ValueError("times must be (ny, nx, ns)")
    rays = np.empty((ny, nx, ns, 7), np.float32)
    rays[..., 0:3], rays[..., 3:6], rays[..., 6] = o, d, t
    opt = self.opts(**kw)
    rows = (self.lib.rtg_shard_rows(ny, opt.row_offset, opt.row_stride, opt.row_block) if opt.compact_rows else ny)
    out = np.empty((rows, nx, 3), np.float32)
    im = _ray_image(nx, ny, ns, integrator, pt_flags)
    A.check(self.lib.rtg_render_rays(self.handle, C.byref(im), rays.ctypes.data, C.byref(opt), out.ctypes.data), self.lib)
    return out


def _renderer_render_rays_device(self, rays_ptr: int, nx: int, ny: int, num_samples: int, out_ptr: int, stream: int = 0,
                                 integrator: int = 0, pt_flags: int = 0, **kw):
    """render_rays() on caller-owned device arrays (rtg_render_rays_device), enqueued on `stream`, synchronous
    on return: rays a contiguous float32 (ny * nx * num_samples, 7) tensor as for trace_device, read in place;
    out a float32 (rows, nx, 3) tensor; pass their data_ptr()."""
    im = _ray_image(nx, ny, num_samples, integrator, pt_flags)
    opt = self.opts(**kw)
    A.check(self.lib.rtg_render_rays_device(self.handle, C.byref(im), C.c_void_p(rays_ptr or None), C.byref(opt),
                                            C.c_void_p(out_ptr or None), C.c_void_p(stream)), self.lib)


Renderer.render_rays = _renderer_render_rays
Renderer.render_rays_device = _renderer_render_rays_device
