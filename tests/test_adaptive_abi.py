"""Adaptive sampling on progressive frames (ABI 10 additions), the part that needs no
GPU: the new entry points are declared, mirrored and exported, the new struct has the C layout, the
sample order is the bijection the header states and spreads its prefixes over the pixel, NULL frames
are refused, and the command line refuses --adaptive without --progressive."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import pytest

from rtg import _abi as A
from rtg import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtg.h")
NEW = ["rtg_sample_order_index", "rtg_frame_retire", "rtg_frame_retire_mask", "rtg_frame_active_pixels",
       "rtg_frame_sample_counts", "rtg_frame_set_retired"]


def test_new_functions_in_header_exports_and_library(lib):
    src = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True, check=True)
    for fn in NEW:
        assert re.search(r"^int32_t " + fn + r"\(", src, re.M), fn
        assert fn in A.EXPORTS, fn
        assert re.search(r"\sT\s" + fn + r"\b", out.stdout), fn
    assert A.RTG_ABI_VERSION == 10 and lib.rtg_abi_version() == 10


def test_struct_layouts_match_c():
    body = 'printf("%zu %zu\\n", sizeof(rtg_frame_adapt), sizeof(rtg_frame_opts));'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        with open(c, "w") as fh:
            fh.write(f'#include <stdio.h>\n#include "{HEADER}"\nint main(void){{{body} return 0;}}\n')
        subprocess.run(["gcc", "-o", os.path.join(d, "s"), c], check=True)
        sizes = [int(x) for x in subprocess.run([os.path.join(d, "s")], capture_output=True, text=True).stdout.split()]
    assert sizes == [C.sizeof(A.FrameAdapt), C.sizeof(A.FrameOpts)] == [16, 16]
    assert [n for n, _ in A.FrameOpts._fields_] == ["first_sample", "sample_count", "moments", "order"]


def _multiplier(n):
    """The header's integer rule, restated."""
    if n <= 2:
        return 1
    m = max((n * 618034 + 500000) // 1000000, 1)
    while math.gcd(m, n) != 1:
        m += 1
    return m


def test_order_0_is_the_identity(lib):
    for n in (1, 2, 7, 256):
        assert [lib.rtg_sample_order_index(n, 0, j) for j in range(n)] == list(range(n))
    assert lib.rtg_sample_order_index(100000, 0, 99999) == 99999


@pytest.mark.parametrize("n", list(range(1, 301)) + [1024, 32768])
def test_order_1_is_the_stated_bijection(lib, n):
    m = _multiplier(n)
    assert 1 <= m and (m < n or n == 1)
    got = [lib.rtg_sample_order_index(n, 1, j) for j in range(n)]
    assert got == [(j * m) % n for j in range(n)]
    assert sorted(got) == list(range(n))


@pytest.mark.parametrize("n", [36, 64, 100, 256, 1024])
def test_order_1_prefix_touches_all_quadrants(lib, n):
    g = math.isqrt(n)
    assert g * g == n

    def quadrants(order):
        q = set()
        for j in range(n // 4):
            k = lib.rtg_sample_order_index(n, order, j)
            q.add((2 * (k % g) // g, 2 * (k // g) // g))     # sample k sits in cell (k mod g, k / g)
        return q

    assert len(quadrants(1)) == 4
    assert len(quadrants(0)) == 2                            # index order: the first sub-pixel rows only


def test_order_index_refuses_bad_arguments(lib):
    for n, order, j in ((4, 0, 4), (4, 1, -1), (4, 1, 4), (0, 0, 0), (-3, 1, 0), (4, 2, 0), (4, -1, 0)):
        assert lib.rtg_sample_order_index(n, order, j) == -1, (n, order, j)
        assert lib.rtg_last_error()
    assert lib.rtg_sample_order_index(32769, 1, 0) == -5
    assert lib.rtg_sample_order_index(32768, 1, 32767) >= 0


def test_null_frames_are_invalid(lib):
    a = A.FrameAdapt(0.1, 0.0, 2, 0)
    n = C.c_int32()
    cnt = (C.c_int32 * 4)()
    ret = (C.c_uint8 * 4)()
    for rc in (lib.rtg_frame_retire(None, C.byref(a), C.byref(n)), lib.rtg_frame_retire_mask(None, ret, C.byref(n)),
               lib.rtg_frame_active_pixels(None), lib.rtg_frame_sample_counts(None, cnt, ret),
               lib.rtg_frame_set_retired(None, cnt, ret)):
        assert rc == -1
        assert lib.rtg_last_error()


def test_host_library_exports_the_adaptive_loop():
    hdr = open(os.path.join(ROOT, "include", "rtg_host.h")).read()
    assert re.search(r"^extern int32_t rtgh_render_scene_adaptive\(", hdr, re.M)
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True)
    assert re.search(r"\sT\srtgh_render_scene_adaptive\b", out.stdout)
    assert native.load().rtgh_render_scene_adaptive.restype is C.c_int32


def test_cli_refuses_adaptive_without_progressive(tmp_path):
    """Argument errors are reported before anything touches a scene file or a GPU."""
    for extra in (["--adaptive", "0.05"], ["--progressive", "4", "--adaptive", "-1"],
                  ["--progressive", "4", "--min-samples", "8"],
                  ["--progressive", "4", "--adaptive", "0.05", "--target-error", "0.1"]):
        p = subprocess.run([native.CLI_PATH, str(tmp_path / "none.xml"), *extra], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and p.stderr.strip(), extra
