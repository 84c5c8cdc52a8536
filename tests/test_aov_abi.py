"""First-hit feature buffers and camera rays (ABI 10 additions), the part that needs no
GPU: the two entry points are declared, mirrored and exported, the new structs have the C layout, the
ABI version stays 10, argument errors are reported in the documented order on a host-only scene, and the
command line refuses --aov together with --devices or --progressive."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from rtg import _abi as A
from rtg import native, scenegen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtg.h")
NEW = ["rtg_render_aov", "rtg_camera_rays"]
INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -5


def test_new_functions_in_header_exports_and_library(lib):
    src = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True, check=True)
    for fn in NEW:
        assert re.search(r"^int32_t " + fn + r"\(", src, re.M), fn
        assert fn in A.EXPORTS, fn
        assert re.search(r"\sT\s" + fn + r"\b", out.stdout), fn
    assert A.RTG_ABI_VERSION == 10 and lib.rtg_abi_version() == 10
    assert re.search(r"^#define RTG_ABI_VERSION 10$", src, re.M)


def test_struct_layouts_match_c():
    body = 'printf("%zu %zu\\n", sizeof(rtg_aov_opts), sizeof(rtg_aov_buffers));'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        with open(c, "w") as fh:
            fh.write(f'#include <stdio.h>\n#include "{HEADER}"\nint main(void){{{body} return 0;}}\n')
        subprocess.run(["gcc", "-o", os.path.join(d, "s"), c], check=True)
        sizes = [int(x) for x in subprocess.run([os.path.join(d, "s")], capture_output=True, text=True).stdout.split()]
    assert sizes == [C.sizeof(A.AovOpts), C.sizeof(A.AovBuffers)] == [16, 40]
    assert [n for n, _ in A.AovOpts._fields_] == ["first_sample", "sample_count", "pad"]
    assert [n for n, _ in A.AovBuffers._fields_] == ["hits", "depth", "normal", "albedo", "ids"]


def test_host_library_exports_the_aov_loop():
    hdr = open(os.path.join(ROOT, "include", "rtg_host.h")).read()
    assert re.search(r"^extern int32_t rtgh_render_scene_aov\(", hdr, re.M)
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True)
    assert re.search(r"\sT\srtgh_render_scene_aov\b", out.stdout)
    assert native.load().rtgh_render_scene_aov.restype is C.c_int32


@pytest.fixture(scope="module")
def host_scene(lib):
    """A host-only scene (no device is touched) with a 4-sample camera."""
    sc = scenegen.simple(8, 6)
    sc.cameras[0].num_samples = 4
    desc, keep = sc.to_desc()
    h = C.c_void_p()
    assert lib.rtg_scene_create(C.byref(desc), A.RTG_DEVICE_HOST_ONLY, C.byref(h)) == 0
    yield h, sc.cameras[0].desc()
    lib.rtg_scene_destroy(h)
    del keep


def _buffers(n):
    depth = np.zeros(n, np.float32)
    return A.AovBuffers(None, depth.ctypes.data_as(A.PF), None, None, None), depth


def test_render_aov_argument_errors(lib, host_scene):
    h, cd = host_scene
    bufs, keep = _buffers(8 * 6)
    opts, ao = A.RenderOpts(), A.AovOpts()

    def call(scene=h, cam=cd, o=opts, a=ao, b=bufs):
        return lib.rtg_render_aov(scene, None if cam is None else C.byref(cam), None if o is None else C.byref(o),
                                  None if a is None else C.byref(a), None if b is None else C.byref(b))

    assert call(scene=None) == INVALID and lib.rtg_last_error()
    assert call(cam=None) == INVALID
    assert call(b=None) == INVALID
    assert call(b=A.AovBuffers()) == INVALID                      # every pointer NULL
    for first, count in ((-1, 0), (4, 0), (5, 0), (0, 5), (2, 3), (0, -1)):   # outside [0, 4]
        assert call(a=A.AovOpts(first, count)) == INVALID, (first, count)
    for pad in ((1, 0), (0, 1)):
        assert call(a=A.AovOpts(0, 0, (C.c_int32 * 2)(*pad))) == INVALID, pad
    two = A.RenderOpts()
    two.num_devices = 2
    assert call(o=two) == UNSUPPORTED
    listed = A.RenderOpts()
    arr = (C.c_int32 * 1)(0)
    listed.devices = C.cast(arr, C.POINTER(C.c_int32))
    assert call(o=listed) == UNSUPPORTED
    # valid arguments (windows inside the camera's samples, NULL option structs): only the device is missing
    for a in (ao, A.AovOpts(0, 4), A.AovOpts(3, 1), A.AovOpts(1, 2), None):
        assert call(a=a) == NO_DEVICE
    assert call(o=None) == NO_DEVICE
    assert b"host-only" in lib.rtg_last_error()
    assert not keep.any()


def test_camera_rays_argument_errors(lib, host_scene):
    h, cd = host_scene
    rays = (A.Ray * (8 * 6 * 4))()
    assert lib.rtg_camera_rays(None, C.byref(cd), 1, 0, 0, rays) == INVALID
    assert lib.rtg_camera_rays(h, None, 1, 0, 0, rays) == INVALID
    assert lib.rtg_camera_rays(h, C.byref(cd), 1, 0, 0, None) == INVALID
    for first, count in ((-1, 0), (4, 0), (0, 5), (2, 3), (0, -1)):
        assert lib.rtg_camera_rays(h, C.byref(cd), 1, first, count, rays) == INVALID, (first, count)
    assert lib.rtg_camera_rays(h, C.byref(cd), 1, 0, 0, rays) == NO_DEVICE
    assert lib.rtg_camera_rays(h, C.byref(cd), 1, 3, 1, rays) == NO_DEVICE


def test_cli_refuses_aov_with_devices_or_progressive(tmp_path):
    """Argument errors are reported before anything touches a scene file or a GPU."""
    for extra in (["--aov", "--progressive", "4"], ["--aov", "--devices", "2"], ["--devices", "2", "--aov"]):
        p = subprocess.run([native.CLI_PATH, str(tmp_path / "none.xml"), *extra], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and p.stderr.strip(), extra
