"""The edge-avoiding denoiser (ABI 10 additions), the part that needs no GPU: the two entry
points are declared, mirrored and exported, the structs have the C layout, argument errors come in the
documented order before the device is touched, the command line refuses --denoise with --progressive,
--adaptive or --devices, and the numpy restatement (tests/denoise_ref.py) that the GPU tests compare
against has the properties a denoiser must have."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from denoise_ref import denoise_ref
from rtg import _abi as A
from rtg import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtg.h")
NEW = ["rtg_denoise", "rtg_denoise_device"]
INVALID, NO_DEVICE = -1, -2
NO_SUCH_DEVICE = 1 << 20        # valid arguments end here on every machine, with or without a GPU


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
    body = 'printf("%zu %zu\\n", sizeof(rtg_denoise_opts), sizeof(rtg_denoise_inputs));'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        with open(c, "w") as fh:
            fh.write(f'#include <stdio.h>\n#include "{HEADER}"\nint main(void){{{body} return 0;}}\n')
        subprocess.run(["gcc", "-o", os.path.join(d, "s"), c], check=True)
        sizes = [int(x) for x in subprocess.run([os.path.join(d, "s")], capture_output=True, text=True).stdout.split()]
    assert sizes == [C.sizeof(A.DenoiseOpts), C.sizeof(A.DenoiseInputs)] == [32, 40]
    assert [n for n, _ in A.DenoiseOpts._fields_] == ["iterations", "sigma_l", "sigma_z", "normal_power_log2", "pad"]
    assert [n for n, _ in A.DenoiseInputs._fields_] == ["rgb", "normal", "depth", "albedo", "variance"]


def test_host_library_exports_the_denoise_loop():
    hdr = open(os.path.join(ROOT, "include", "rtg_host.h")).read()
    assert re.search(r"^extern int32_t rtgh_render_scene_denoise\(", hdr, re.M)
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True)
    assert re.search(r"\sT\srtgh_render_scene_denoise\b", out.stdout)
    assert native.load().rtgh_render_scene_denoise.restype is C.c_int32


def test_argument_errors_in_order(lib):
    nx, ny = 8, 6
    rgb = np.ones((ny, nx, 3), np.float32)
    normal = np.zeros((ny, nx, 3), np.float32)
    depth = np.ones((ny, nx), np.float32)
    out = np.full((ny, nx, 3), 7.0, np.float32)
    pf = lambda a: a.ctypes.data_as(A.PF)

    def inputs(**kw):
        f = dict(rgb=pf(rgb), normal=pf(normal), depth=pf(depth), albedo=None, variance=None)
        f.update(kw)
        return A.DenoiseInputs(f["rgb"], f["normal"], f["depth"], f["albedo"], f["variance"])

    def call(fn, device=NO_SUCH_DEVICE, di=inputs(), w=nx, h=ny, o=A.DenoiseOpts(), dst=out):
        args = [device, None if di is None else C.byref(di), w, h, None if o is None else C.byref(o),
                None if dst is None else (pf(dst) if fn == "rtg_denoise" else C.c_void_p(dst.ctypes.data))]
        if fn == "rtg_denoise_device":
            args.append(None)
        return getattr(lib, fn)(*args)

    nan, inf = float("nan"), float("inf")
    for fn in NEW:
        # every INVALID comes before the device is looked at: the device index here exists nowhere
        assert call(fn, di=None) == INVALID and lib.rtg_last_error()
        for field in ("rgb", "normal", "depth"):
            assert call(fn, di=inputs(**{field: None})) == INVALID, field
        assert call(fn, dst=None) == INVALID
        for w, h in ((0, 6), (8, 0), (-1, 6), (8, -1), (1 << 16, 1 << 15)):     # the last: 2^31 pixels > 2^30
            assert call(fn, w=w, h=h) == INVALID, (w, h)
        for it in (-1, 9):
            assert call(fn, o=A.DenoiseOpts(it)) == INVALID, it
        for p in (-1, 11):
            assert call(fn, o=A.DenoiseOpts(0, 0, 0, p)) == INVALID, p
        for s in (-1.0, nan, inf, -inf):
            assert call(fn, o=A.DenoiseOpts(0, s, 0, 0)) == INVALID, s
            assert call(fn, o=A.DenoiseOpts(0, 0, s, 0)) == INVALID, s
        for k in range(4):
            pad = [0, 0, 0, 0]
            pad[k] = 1
            assert call(fn, o=A.DenoiseOpts(0, 0, 0, 0, (C.c_int32 * 4)(*pad))) == INVALID, k
        # an invalid argument wins over a missing device, a valid call reaches the device check
        assert call(fn, device=-1, o=A.DenoiseOpts(9)) == INVALID
        for o in (A.DenoiseOpts(), None, A.DenoiseOpts(1, 0.5, 3.0, 1), A.DenoiseOpts(8, 0, 0, 10)):
            assert call(fn, o=o) == NO_DEVICE
        assert call(fn, device=-1) == NO_DEVICE
        assert call(fn, w=1 << 15, h=1 << 15) == NO_DEVICE                        # 2^30 pixels: allowed
    assert (out == 7.0).all()


def test_cli_refuses_denoise_with_progressive_adaptive_or_devices(tmp_path):
    """Argument errors are reported before anything touches a scene file or a GPU."""
    for extra in (["--denoise", "--progressive", "4"], ["--denoise", "--adaptive", "0.1"], ["--denoise", "--devices", "2"],
                  ["--progressive", "4", "--adaptive", "0.1", "--denoise"], ["--devices", "2", "--aov", "--denoise"]):
        p = subprocess.run([native.CLI_PATH, str(tmp_path / "none.xml"), *extra], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and p.stderr.strip(), extra


# ---- the restatement itself: two half-planes with orthogonal normals, a gentle depth ramp, base colours plus
# N(0, 20^2) noise, the true variance of the luminance passed in
NY, NX, SIGMA = 48, 64, 20.0


@pytest.fixture(scope="module")
def planes():
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:NY, 0:NX]
    left = xx < NX // 2
    normal = np.where(left[..., None], np.float32([0, 0, 1]), np.float32([1, 0, 0])).astype(np.float32)
    depth = (5.0 + 0.01 * xx + 0.005 * yy).astype(np.float32)
    base = np.where(left[..., None], np.float32([180, 90, 60]), np.float32([50, 120, 200])).astype(np.float32)
    rgb = (base + rng.normal(0.0, SIGMA, base.shape)).astype(np.float32)
    var = np.full((NY, NX), SIGMA * SIGMA * (0.2126 ** 2 + 0.7152 ** 2 + 0.0722 ** 2), np.float32)
    return dict(left=left, normal=normal, depth=depth, base=base, rgb=rgb, var=var, rng=rng)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_ref_removes_noise(planes):
    p = planes
    out = denoise_ref(p["rgb"], p["normal"], p["depth"], variance=p["var"])
    rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - p["base"]) ** 2)))
    before, after = rms(p["rgb"]), rms(out)
    print(f"noise rms {before:.3f} -> {after:.3f}, ratio {before / after:.2f}")
    assert before / after >= 8.0


def test_ref_keeps_a_constant_image(planes):
    p = planes
    rgb = np.full((NY, NX, 3), 123.456, np.float32)
    for var in (None, p["var"]):
        out = denoise_ref(rgb, p["normal"], p["depth"], variance=var)
        rel = float(np.max(np.abs(out.astype(np.float64) - rgb) / rgb))
        print(f"constant image: max relative deviation {rel:.3g}")
        assert rel <= 1e-5       # 5 iterations x 28 roundings x 2^-24


def test_ref_normal_edge_isolates_bitwise_without_variance(planes):
    p = planes
    other = p["rgb"].copy()
    other[~p["left"]] = np.random.default_rng(4).uniform(0, 255, other[~p["left"]].shape).astype(np.float32)
    a = denoise_ref(p["rgb"], p["normal"], p["depth"])
    b = denoise_ref(other, p["normal"], p["depth"])
    assert np.array_equal(_bits(a)[p["left"]], _bits(b)[p["left"]])
    assert not np.array_equal(_bits(a)[~p["left"]], _bits(b)[~p["left"]])


def test_ref_invalid_pixels_pass_through_and_stay_out(planes):
    p = planes
    rgb, depth = p["rgb"].copy(), p["depth"].copy()
    depth[20:30, 20:30] = 0.0
    rgb[5, 40, 1] = np.nan
    bad = np.zeros((NY, NX), bool)
    bad[20:30, 20:30] = True
    bad[5, 40] = True
    for var in (None, p["var"]):
        out = denoise_ref(rgb, p["normal"], depth, variance=var)
        assert np.array_equal(_bits(out)[bad], _bits(rgb)[bad])
        assert np.isfinite(out[~bad]).all()
        assert not np.array_equal(_bits(out)[~bad], _bits(rgb)[~bad])


def test_ref_albedo_of_ones_changes_nothing(planes):
    p = planes
    ones = np.ones((NY, NX, 3), np.float32)
    a = denoise_ref(p["rgb"], p["normal"], p["depth"], variance=p["var"])
    b = denoise_ref(p["rgb"], p["normal"], p["depth"], albedo=ones, variance=p["var"])
    assert np.array_equal(_bits(a), _bits(b))
