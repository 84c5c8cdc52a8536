"""The edge-avoiding denoiser on the GPU (rtg_denoise) against its numpy restatement
(tests/denoise_ref.py): every comparison is array_equal on the int32 views."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import rtg
from denoise_ref import denoise_ref
from rtg import _abi as A
from rtg import native, scenegen
from rtg.render import denoised_name, ppm_p3_bytes
from rtg.scene import parse_xml, write_xml

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def guides(ny, nx, seed):
    """An image with a few normal clusters, a depth ramp plus steps, about 3 % invalid pixels (no depth, a
    NaN / inf colour or normal) and NaN, inf and negative variances sprinkled in."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ny, 0:nx]
    dirs = rng.normal(size=(4, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    cluster = ((xx // 11) + 2 * (yy // 9)) % 4
    normal = (dirs[cluster] + rng.normal(0, 0.05, (ny, nx, 3))).astype(np.float32)
    depth = (3.0 + 0.02 * xx + 0.013 * yy + 1.5 * ((xx // 17) % 2) + 0.7 * ((yy // 13) % 3)).astype(np.float32)
    albedo = rng.uniform(0.0, 1.0, (ny, nx, 3)).astype(np.float32)
    albedo[rng.random((ny, nx)) < 0.05] = 0.0                        # below the 1/256 floor
    rgb = (albedo * rng.uniform(20, 300, (ny, nx, 1)) + rng.normal(0, 15, (ny, nx, 3))).astype(np.float32)
    var = rng.uniform(0.0, 200.0, (ny, nx)).astype(np.float32)
    for value in (np.nan, np.inf, -1.0, 0.0):
        var[rng.random((ny, nx)) < 0.02] = value
    depth[rng.random((ny, nx)) < 0.01] = 0.0
    depth[rng.random((ny, nx)) < 0.005] = -2.0
    depth[rng.random((ny, nx)) < 0.005] = np.inf
    rgb[rng.random((ny, nx)) < 0.005, 1] = np.nan
    normal[rng.random((ny, nx)) < 0.005, 2] = -np.inf
    return dict(img=rgb, normal=normal, depth=depth, albedo=albedo, variance=var)


def check(g, **opts):
    got = rtg.denoise(g["img"], g["normal"], g["depth"], g.get("albedo"), g.get("variance"), **opts)
    ref = denoise_ref(g["img"], g["normal"], g["depth"], g.get("albedo"), g.get("variance"), **opts)
    diff = int(np.count_nonzero(_bits(got) != _bits(ref)))
    print(f"{g['img'].shape[:2]} {opts}: {diff} differing values of {ref.size}")
    assert np.array_equal(_bits(got), _bits(ref))
    return got


@pytest.mark.parametrize("ny,nx,opts", [(1, 1, {}), (3, 70, {}), (65, 33, {}), (37, 53, {}), (130, 97, dict(iterations=8))])
def test_shapes(gpu, ny, nx, opts):
    """Sizes below, at no multiple of and beyond the 32x8 block; with 8 iterations stride 128 exceeds the
    image, and both the LDS-tiled (strides 1, 2) and the direct kernels run."""
    check(guides(ny, nx, 100 + ny), **opts)


def test_tall_image(gpu):
    """More rows than 65535 blocks of 8 cover: the blocks are numbered in one grid dimension."""
    check(guides(65536 * 8 + 3, 2, 5), iterations=2)


@pytest.mark.parametrize("albedo", [False, True])
@pytest.mark.parametrize("variance", [False, True])
def test_optional_inputs(gpu, albedo, variance):
    g = guides(37, 53, 7)
    if not albedo:
        g["albedo"] = None
    if not variance:
        g["variance"] = None
    check(g)


@pytest.mark.parametrize("opts", [dict(iterations=1), dict(normal_power_log2=1), dict(normal_power_log2=10),
                                  dict(sigma_l=0.5, sigma_z=3.0)])
def test_options(gpu, opts):
    check(guides(37, 53, 7), **opts)


def test_device_entry_point_and_repeatability(gpu, lib):
    import torch

    g = guides(65, 33, 11)
    host = rtg.denoise(g["img"], g["normal"], g["depth"], g["albedo"], g["variance"], device=gpu)
    assert np.array_equal(_bits(host), _bits(rtg.denoise(g["img"], g["normal"], g["depth"], g["albedo"], g["variance"],
                                                         device=gpu)))
    dev = torch.device(f"cuda:{gpu}")
    t = {k: torch.from_numpy(v).to(dev) for k, v in g.items()}
    out = torch.full((65, 33, 3), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ptr = lambda k: C.cast(C.c_void_p(t[k].data_ptr()), A.PF)
    di = A.DenoiseInputs(ptr("img"), ptr("normal"), ptr("depth"), ptr("albedo"), ptr("variance"))
    for _ in range(2):
        A.check(lib.rtg_denoise_device(gpu, C.byref(di), 33, 65, None, C.c_void_p(out.data_ptr()), None), lib)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(host))


def _frame_reference(r, f, cam):
    cnt = f.counts()[0]
    var = (f.moments()[1] / np.maximum(cnt, 1).astype(np.float32)).astype(np.float32)
    var[cnt < 2] = 0
    a = r.aov(cam)
    return denoise_ref(f.resolve(), a["normal"], a["depth"], a["albedo"], var)


def test_real_frames(gpu):
    sc = scenegen.cornell_pt(64, 36, spp=16)
    with rtg.Renderer(sc, device=gpu) as r:
        before = r.render(0)
        with r.frame(0, moments=True) as f:
            f.add(16)
            img = f.resolve()
            out = f.denoise()
            assert np.array_equal(_bits(out), _bits(_frame_reference(r, f, 0)))
            assert not np.array_equal(_bits(out), _bits(img))
            assert np.array_equal(_bits(f.resolve()), _bits(img))
            # without demodulation and without moments the other inputs are dropped
            a = r.aov(0)
            var = (f.moments()[1] / np.float32(16)).astype(np.float32)
            assert np.array_equal(_bits(f.denoise(demodulate=False, iterations=2)),
                                  _bits(denoise_ref(img, a["normal"], a["depth"], None, var, iterations=2)))
        with r.frame(0) as f:
            f.add(16)
            assert np.array_equal(_bits(f.denoise()), _bits(denoise_ref(img, a["normal"], a["depth"], a["albedo"], None)))
        assert np.array_equal(_bits(r.render(0)), _bits(before))
    # adaptive: an order-1 frame of a 64-spp camera, pixels retired at different counts
    sc = scenegen.cornell_pt(64, 36, spp=64)
    with rtg.Renderer(sc, device=gpu) as r:
        before = r.render(0)
        with r.frame(0, moments=True, order=1) as f:
            f.add(8)
            left = f.retire(rel_tol=0.1, min_samples=4)
            f.add(8)
            cnt = f.counts()[0]
            print(f"adaptive: {left} of {cnt.size} pixels active, counts {cnt.min()}..{cnt.max()}")
            assert cnt.min() < cnt.max()
            img = f.resolve()
            assert np.array_equal(_bits(f.denoise()), _bits(_frame_reference(r, f, 0)))
            assert np.array_equal(_bits(f.resolve()), _bits(img))
        assert np.array_equal(_bits(r.render(0)), _bits(before))


def test_refusals(gpu):
    sc = scenegen.cornell_pt(32, 18, spp=4)
    with rtg.Renderer(sc, device=gpu) as r:
        with r.frame(0, moments=True, row_stride=2) as f:
            f.add(4)
            with pytest.raises(ValueError):
                f.denoise()
        with r.frame(0, moments=True, row_stride=2, compact_rows=1) as f:
            f.add(4)
            with pytest.raises(ValueError):
                f.denoise()
        with r.frame(0, moments=True) as f:
            with pytest.raises(ValueError):
                f.denoise()


def test_cli_denoise(gpu, tmp_path):
    sc = scenegen.cornell_pt(32, 24, spp=8)
    sc.cameras[0].image_name = "pt.png"
    xml = write_xml(sc, str(tmp_path / "pt.xml"))
    plain, den = tmp_path / "plain", tmp_path / "den"
    plain.mkdir()
    den.mkdir()
    for d, extra in ((plain, []), (den, ["--denoise", "--aov"])):
        p = subprocess.run([native.CLI_PATH, xml, "--out-dir", str(d), "--device", str(gpu), *extra], capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 0, p.stderr
    assert (den / "pt.png").read_bytes() == (plain / "pt.png").read_bytes()
    assert sorted(x.name for x in den.iterdir()) == ["pt.png", "pt_albedo.png", "pt_denoised.png", "pt_depth.png",
                                                     "pt_normal.png"]
    with rtg.Renderer(parse_xml(xml), device=gpu) as r:
        with r.frame(0, moments=True) as f:
            f.add(8)
            want = f.denoise()
    assert denoised_name("pt.png") == "pt_denoised.png"
    assert (den / "pt_denoised.png").read_bytes() == ppm_p3_bytes(want)
    # the Python host writes the same files
    py = tmp_path / "py"
    py.mkdir()
    rtg.render_scene(parse_xml(xml), out_dir=str(py), device=gpu, denoise=True)
    for name in ("pt.png", "pt_denoised.png"):
        assert (py / name).read_bytes() == (den / name).read_bytes(), name
