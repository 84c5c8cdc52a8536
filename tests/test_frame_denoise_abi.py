"""Denoising a frame on the device (ABI 10 additions), the part that needs no GPU: the three
entry points are declared, mirrored and exported, rtg_frame_guides has the C layout, a NULL frame is refused
with a message, the host library carries the progressive-denoise loop, and the command line refuses
--denoise-rounds without --progressive or beside --adaptive, --devices, --aov or --denoise."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

from rtg import _abi as A
from rtg import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtg.h")
NEW = ["rtg_frame_denoise", "rtg_frame_denoise_device", "rtg_frame_guides_device"]
INVALID = -1


def test_new_functions_in_header_exports_and_library(lib):
    src = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True, check=True)
    for fn in NEW:
        assert re.search(r"^int32_t " + fn + r"\(", src, re.M), fn
        assert fn in A.EXPORTS, fn
        assert re.search(r"\sT\s" + fn + r"\b", out.stdout), fn
    assert A.RTG_ABI_VERSION == 10 and lib.rtg_abi_version() == 10
    assert re.search(r"^#define RTG_ABI_VERSION 10$", src, re.M)


def test_guides_struct_layout_matches_c():
    fields = ["rgb", "normal", "depth", "albedo", "variance"]
    body = 'printf("%zu", sizeof(rtg_frame_guides));' + "".join(
        f'printf(" %zu", offsetof(rtg_frame_guides, {f}));' for f in fields)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        with open(c, "w") as fh:
            fh.write(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{{body} return 0;}}\n')
        subprocess.run(["gcc", "-o", os.path.join(d, "s"), c], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "s")], capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(A.FrameGuides) == 40
    assert [n for n, _ in A.FrameGuides._fields_] == fields
    assert got[1:] == [getattr(A.FrameGuides, f).offset for f in fields] == [0, 8, 16, 24, 32]


def test_null_frame_is_invalid_with_a_message(lib):
    out = np.full(12, 7.0, np.float32)
    g = A.FrameGuides(out.ctypes.data, 0, 0, 0, 0)
    calls = {
        "rtg_frame_denoise": lambda f: lib.rtg_frame_denoise(f, None, 1, out.ctypes.data_as(A.PF)),
        "rtg_frame_denoise_device": lambda f: lib.rtg_frame_denoise_device(f, None, 1, C.c_void_p(out.ctypes.data), None),
        "rtg_frame_guides_device": lambda f: lib.rtg_frame_guides_device(f, C.byref(g), None),
    }
    assert sorted(calls) == sorted(NEW)
    for fn, call in calls.items():
        assert lib.rtg_sample_order_index(4, 7, 0) == INVALID        # another call's message is in place first
        before = lib.rtg_last_error()
        assert call(None) == INVALID, fn
        assert lib.rtg_last_error() and lib.rtg_last_error() != before, fn
    assert (out == 7.0).all()


def test_host_library_exports_the_progressive_denoise_loop():
    hdr = open(os.path.join(ROOT, "include", "rtg_host.h")).read()
    assert re.search(r"^extern int32_t rtgh_render_scene_progressive_denoise\(", hdr, re.M)
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True)
    assert re.search(r"\sT\srtgh_render_scene_progressive_denoise\b", out.stdout)
    fn = native.load().rtgh_render_scene_progressive_denoise
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 6
    # argument errors come before the scene file is looked at
    assert fn(b"/nonexistent/none.xml", 0, 1, None, 0, 0.0) == INVALID
    assert fn(b"/nonexistent/none.xml", 0, 1, None, 4, -1.0) == INVALID


def test_cli_refuses_denoise_rounds_alone_or_combined(tmp_path):
    """Argument errors are reported before anything touches a scene file or a GPU."""
    for extra in (["--denoise-rounds"], ["--denoise-rounds", "--target-error", "0.1"],
                  ["--progressive", "4", "--adaptive", "0.1", "--denoise-rounds"],
                  ["--progressive", "4", "--devices", "2", "--denoise-rounds"],
                  ["--progressive", "4", "--aov", "--denoise-rounds"],
                  ["--progressive", "4", "--denoise", "--denoise-rounds"],
                  ["--denoise-rounds", "--devices", "2"], ["--denoise-rounds", "--aov"], ["--denoise-rounds", "--denoise"],
                  ["--progressive", "0", "--denoise-rounds"],
                  ["--denoise", "--progressive", "4"]):               # the refusal that was there stays
        p = subprocess.run([native.CLI_PATH, str(tmp_path / "none.xml"), *extra], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and p.stderr.strip(), extra
