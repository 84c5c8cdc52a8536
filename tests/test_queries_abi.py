"""Occlusion queries and ray queries on device arrays (ABI 10 additions), the part that needs
no GPU: the three entry points are declared, mirrored and exported, the ABI version stays 10, and argument
errors come in the documented order on a host-only scene (invalid arguments, then n == 0, then the device)."""
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
NEW = ["rtg_trace_occluded", "rtg_trace_closest_device", "rtg_trace_occluded_device"]
OK, INVALID, NO_DEVICE = 0, -1, -2
PU8 = C.POINTER(C.c_uint8)


def test_new_functions_in_header_exports_and_library(lib):
    src = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True, check=True)
    for fn in NEW:
        assert re.search(r"^int32_t " + fn + r"\(", src, re.M), fn
        assert fn in A.EXPORTS, fn
        assert re.search(r"\sT\s" + fn + r"\b", out.stdout), fn
    assert A.RTG_ABI_VERSION == 10 and lib.rtg_abi_version() == 10
    assert re.search(r"^#define RTG_ABI_VERSION 10$", src, re.M)
    assert "44 B per ray" in src                      # the header states the workspace per ray


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


def test_occluded_argument_errors(lib, host_scene):
    h = host_scene
    rays = (A.Ray * 4)()
    tmax = np.ones(4, np.float32)
    occ = np.full(4, 7, np.uint8)
    pt, po = tmax.ctypes.data_as(A.PF), occ.ctypes.data_as(PU8)
    f = lib.rtg_trace_occluded
    assert f(None, rays, pt, 4, po, 0) == INVALID and lib.rtg_last_error()
    assert f(None, rays, pt, 0, po, 0) == INVALID          # a null scene comes before n == 0
    assert f(h, rays, pt, -1, po, 0) == INVALID
    assert f(h, None, pt, 4, po, 0) == INVALID
    assert f(h, rays, pt, 4, None, 0) == INVALID
    assert f(h, None, None, 0, None, 0) == OK              # n == 0 comes before the device
    assert f(h, rays, pt, 0, po, 1) == OK
    assert f(h, rays, pt, 4, po, 0) == NO_DEVICE
    assert b"host-only" in lib.rtg_last_error()
    assert f(h, rays, None, 4, po, 1) == NO_DEVICE         # tmax may be NULL
    assert (occ == 7).all()


def test_device_forms_argument_errors(lib, host_scene):
    h = host_scene
    p = C.c_void_p(4096)          # never dereferenced: every call below is refused before any device work
    fc, fo = lib.rtg_trace_closest_device, lib.rtg_trace_occluded_device
    assert fc(None, p, 4, p, 0, None) == INVALID
    assert fc(None, p, 0, p, 0, None) == INVALID
    assert fc(h, p, -1, p, 0, None) == INVALID
    assert fc(h, None, 4, p, 0, None) == INVALID
    assert fc(h, p, 4, None, 0, None) == INVALID
    assert fc(h, None, 0, None, 0, None) == OK
    assert fc(h, p, 4, p, 0, None) == NO_DEVICE
    assert fo(None, p, p, 4, p, 0, None) == INVALID
    assert fo(None, p, p, 0, p, 0, None) == INVALID
    assert fo(h, p, p, -1, p, 0, None) == INVALID
    assert fo(h, None, p, 4, p, 0, None) == INVALID
    assert fo(h, p, p, 4, None, 0, None) == INVALID
    assert fo(h, None, None, 0, None, 0, None) == OK
    assert fo(h, p, None, 4, p, 0, None) == NO_DEVICE
    assert fo(h, p, p, 4, p, 1, None) == NO_DEVICE
    assert b"host-only" in lib.rtg_last_error()
