"""Rendering caller-supplied primary rays (ABI 10 additions), the part that needs no GPU: the
two entry points are declared, mirrored and exported, the ABI version stays 10, rtg_ray_image is 32 bytes, and
the argument errors come in the documented order on a host-only scene -- with ray and output pointers that are
never dereferenced."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rtg import _abi as A
from rtg import scenegen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtg.h")
NEW = ["rtg_render_rays", "rtg_render_rays_device"]
OK, INVALID, NO_DEVICE, UNSUPPORTED = 0, -1, -2, -5


def test_new_functions_in_header_exports_and_library(lib):
    src = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True, check=True)
    for fn in NEW:
        assert re.search(r"^int32_t " + fn + r"\(", src, re.M), fn
        assert fn in A.EXPORTS, fn
        assert re.search(r"\sT\s" + fn + r"\b", out.stdout), fn
    assert A.RTG_ABI_VERSION == 10 and lib.rtg_abi_version() == 10
    assert re.search(r"^#define RTG_ABI_VERSION 10$", src, re.M)
    assert re.search(r"typedef struct rtg_ray_image \{\s*/\* 32 bytes \*/", src)
    assert C.sizeof(A.RayImage) == 32
    assert C.sizeof(A.Ray) == 28 and "28 B per ray" in src


@pytest.fixture(scope="module")
def host_scene(lib):
    """A host-only scene: no device is touched."""
    sc = scenegen.simple(8, 6)
    desc, keep = sc.to_desc()
    h = C.c_void_p()
    assert lib.rtg_scene_create(C.byref(desc), A.RTG_DEVICE_HOST_ONLY, C.byref(h)) == 0
    yield h
    lib.rtg_scene_destroy(h)
    del keep


def image(nx=8, ny=6, ns=2, integrator=0, pt_flags=0, pad=(0, 0, 0)):
    return A.RayImage(nx, ny, ns, integrator, pt_flags, (C.c_int32 * 3)(*pad))


def opts(**kw):
    o = A.RenderOpts()
    o.row_stride = o.row_block = 1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_argument_errors_in_order(lib, host_scene):
    h = host_scene
    sentinel = np.full((6, 8, 3), -7.0, np.float32)
    rays = np.zeros((6, 8, 2, 7), np.float32)       # all-zero directions: never looked at on a host-only scene
    wild = C.c_void_p(4096)                         # never dereferenced: every call is refused before any device work
    im, o = image(), opts()
    host = lambda s, i, r, op, out: lib.rtg_render_rays(s, i, r, op, out)
    dev = lambda s, i, r, op, out: lib.rtg_render_rays_device(s, i, r, op, out, None)
    for f, r, out in ((host, C.c_void_p(rays.ctypes.data), C.c_void_p(sentinel.ctypes.data)), (host, wild, wild),
                      (dev, wild, wild)):
        bi, bo = C.byref(im), C.byref(o)
        # 1. NULL arguments, each before everything else (here together with a bad image and bad options)
        worst_im, worst_o = C.byref(image(nx=0, pad=(1, 0, 0))), C.byref(opts(row_offset=5, num_devices=2))
        assert f(None, worst_im, r, worst_o, out) == INVALID and lib.rtg_last_error()
        assert f(h, None, r, worst_o, out) == INVALID
        assert f(h, worst_im, None, worst_o, out) == INVALID
        assert f(h, worst_im, r, worst_o, None) == INVALID
        # 2. the image, before the options
        for bad in (image(nx=0), image(ny=0), image(ns=0), image(ny=-3), image(pad=(0, 0, 1)), image(pad=(2, 0, 0)),
                    image(integrator=2), image(integrator=-1), image(pt_flags=8), image(pt_flags=-1)):
            assert f(h, C.byref(bad), r, C.byref(opts(num_devices=2)), out) == INVALID, list(bad.pad)
        # 3. the options, before the multi-device refusal
        for kw in (dict(row_offset=1), dict(row_offset=-1), dict(row_offset=2, row_stride=2), dict(tile_band=-1),
                   dict(segment_pixels=-1), dict(segment_nodes=-1), dict(schedule=3), dict(schedule=-1)):
            assert f(h, bi, r, C.byref(opts(num_devices=2, **kw)), out) == INVALID, kw
        # 4. several devices, before the host-only scene
        assert f(h, bi, r, C.byref(opts(num_devices=2)), out) == UNSUPPORTED
        assert b"one device" in lib.rtg_last_error()
        devs = (C.c_int32 * 1)(0)
        assert f(h, bi, r, C.byref(opts(devices=C.cast(devs, C.POINTER(C.c_int32)))), out) == UNSUPPORTED
        # 5. the host-only scene; NULL options are the defaults
        assert f(h, bi, r, bo, out) == NO_DEVICE
        assert b"host-only" in lib.rtg_last_error()
        assert f(h, bi, r, None, out) == NO_DEVICE
        assert f(h, C.byref(image(integrator=1, pt_flags=7)), r, C.byref(opts(num_devices=1, compact_rows=1)), out) == NO_DEVICE
    assert (sentinel == -7.0).all()
