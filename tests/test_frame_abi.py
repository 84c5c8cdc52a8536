"""Progressive frames (rtg_frame, ABI 10), the part that needs no GPU: the new structs have the C
layouts, a host-only scene cannot carry a frame, and NULL arguments are refused.  (That the header,
the ctypes exports and the library's symbols agree on the new functions is tests/test_abi.py's.)"""
import ctypes as C
import os
import subprocess
import tempfile

import re

from rtg import _abi as A
from rtg import native, scenegen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtg.h")


def test_abi_version_is_10(lib):
    assert A.RTG_ABI_VERSION == 10 and lib.rtg_abi_version() == 10


def test_frame_struct_layouts_match_c():
    structs = ["rtg_frame_opts", "rtg_frame_error"]
    py = [A.FrameOpts, A.FrameError]
    body = "\n".join(f'printf("%zu\\n", sizeof({s}));' for s in structs)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        with open(c, "w") as fh:
            fh.write(f'#include <stdio.h>\n#include "{HEADER}"\nint main(void){{{body} return 0;}}\n')
        subprocess.run(["gcc", "-o", os.path.join(d, "s"), c], check=True)
        sizes = [int(x) for x in subprocess.run([os.path.join(d, "s")], capture_output=True, text=True).stdout.split()]
    assert sizes == [C.sizeof(p) for p in py]


def _host_scene(lib):
    sc = scenegen.simple(8, 8)
    desc, keep = sc.to_desc()
    h = C.c_void_p()
    assert lib.rtg_scene_create(C.byref(desc), A.RTG_DEVICE_HOST_ONLY, C.byref(h)) == A.RTG_OK
    return sc, h, keep


def test_host_only_scene_cannot_carry_a_frame(lib):
    sc, h, _keep = _host_scene(lib)
    cam = sc.cameras[0].desc()
    f = C.c_void_p(1)
    assert lib.rtg_frame_create(h, C.byref(cam), None, None, C.byref(f)) == -2
    assert b"host-only" in lib.rtg_last_error()
    assert not f.value                         # *out is cleared on failure
    assert lib.rtg_scene_destroy(h) == 0       # no frame was left behind


def test_null_arguments_are_invalid(lib):
    sc, h, _keep = _host_scene(lib)
    cam = sc.cameras[0].desc()
    f = C.c_void_p()
    assert lib.rtg_frame_create(None, C.byref(cam), None, None, C.byref(f)) == -1
    assert lib.rtg_frame_create(h, None, None, None, C.byref(f)) == -1
    assert lib.rtg_frame_create(h, C.byref(cam), None, None, None) == -1
    buf = (C.c_float * 4)()
    err = A.FrameError()
    for rc in (lib.rtg_frame_add_samples(None, 1, None), lib.rtg_frame_samples_done(None),
               lib.rtg_frame_resolve(None, buf), lib.rtg_frame_resolve_device(None, None, None),
               lib.rtg_frame_moments(None, buf, buf), lib.rtg_frame_error_stats(None, C.byref(err)),
               lib.rtg_frame_get_state(None, buf, buf), lib.rtg_frame_set_state(None, 0, buf, buf)):
        assert rc == -1
        assert lib.rtg_last_error()
    assert lib.rtg_frame_destroy(None) == 0    # like rtg_scene_destroy(NULL)
    assert lib.rtg_scene_destroy(h) == 0


def test_host_library_exports_the_progressive_loop():
    hdr = open(os.path.join(ROOT, "include", "rtg_host.h")).read()
    assert re.search(r"^extern int32_t rtgh_render_scene_progressive\(", hdr, re.M)
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True)
    assert re.search(r"\sT\srtgh_render_scene_progressive\b", out.stdout)
    assert native.load().rtgh_render_scene_progressive.restype is C.c_int32


def test_cli_refuses_progressive_with_devices(tmp_path):
    """Argument errors are reported before anything touches a scene file or a GPU."""
    for extra in (["--progressive", "4", "--devices", "2"], ["--progressive", "0"], ["--target-error", "0.1"]):
        p = subprocess.run([native.CLI_PATH, str(tmp_path / "none.xml"), *extra], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and p.stderr.strip(), extra
