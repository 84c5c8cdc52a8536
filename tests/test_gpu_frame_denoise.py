"""Denoising a frame on the device (rtg_frame_denoise) against today's host path
(Frame.denoise()) and the numpy restatement (tests/denoise_ref.py) fed from the frame's public getters: every
comparison is array_equal on the int32 views."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import rtg
from denoise_ref import denoise_ref
from rtg import _abi as A
from rtg import native, scenegen
from rtg.scene import write_xml

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _variance(f):
    """The float32 formula of include/rtg.h from moments() and counts(); None where the frame has none."""
    if not (f.has_moments and f.samples_done >= 2):
        return None
    cnt = f.counts()[0]
    var = (f.moments()[1] / np.maximum(cnt, 1).astype(np.float32)).astype(np.float32)
    var[cnt < 2] = 0
    return var


def _reference(r, f, demodulate=True, **opts):
    a = r.aov(f.camera, seed=f.opts.seed, traversal=f.opts.traversal)
    return denoise_ref(f.resolve(), a["normal"], a["depth"], a["albedo"] if demodulate else None, _variance(f), **opts)


def _device_result(f, gpu, demodulate=True, **opts):
    """denoise_device into a torch tensor pre-filled with -1, on a stream of torch's that is not the default one."""
    import torch

    dev = torch.device(f"cuda:{gpu}")
    out = torch.full((f.camera.ny, f.camera.nx, 3), -1.0, dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    f.denoise_device(out.data_ptr(), stream=stream.cuda_stream, demodulate=demodulate, **opts)
    return out.cpu().numpy()


def check(r, f, gpu, demodulate=True, **opts):
    """The resident paths against the host path and the restatement; returns the image."""
    host = f.denoise(demodulate, **opts)
    ref = _reference(r, f, demodulate, **opts)
    res = f.denoise(demodulate, resident=True, **opts)
    dev = _device_result(f, gpu, demodulate, **opts)
    for name, got in (("resident", res), ("device", dev)):
        for what, want in (("host path", host), ("restatement", ref)):
            diff = int(np.count_nonzero(_bits(got) != _bits(want)))
            print(f"{host.shape[:2]} spp {f.samples_done} demod {demodulate} {opts}: {name} vs {what}: {diff} differing "
                  f"values of {want.size}")
            assert diff == 0, (name, what)
    return res


def test_stages(gpu):
    """One sample (no variance), four, all sixteen."""
    sc = scenegen.cornell_pt(64, 36, spp=16)
    with rtg.Renderer(sc, device=gpu) as r:
        with r.frame(0, moments=True) as f:
            seen = []
            for n in (1, 3, 12):
                f.add(n)
                img = f.resolve()
                out = check(r, f, gpu)
                assert not _same(out, img)
                assert _same(f.resolve(), img)
                seen.append(out)
            assert f.samples_done == 16
            assert not _same(seen[0], seen[1]) and not _same(seen[1], seen[2])


@pytest.mark.parametrize("nx,ny", [(37, 53), (1, 1)])
@pytest.mark.parametrize("demodulate", [True, False])
def test_sizes_off_the_block(gpu, nx, ny, demodulate):
    sc = scenegen.cornell_pt(nx, ny, spp=4)
    with rtg.Renderer(sc, device=gpu) as r:
        with r.frame(0, moments=True) as f:
            f.add(4)
            check(r, f, gpu, demodulate)


@pytest.mark.parametrize("demodulate", [True, False])
def test_textured_whitted_scene(gpu, demodulate):
    """Texture detail is in the albedo: the two settings must differ, each matching its own reference."""
    sc = scenegen.textured(37, 53, spp=4)
    with rtg.Renderer(sc, device=gpu) as r:
        with r.frame(0, moments=True) as f:
            f.add(4)
            out = check(r, f, gpu, demodulate)
            assert not _same(out, f.denoise(not demodulate, resident=True))


def test_without_moments(gpu):
    sc = scenegen.cornell_pt(37, 53, spp=4)
    with rtg.Renderer(sc, device=gpu) as r:
        with r.frame(0) as f:
            f.add(4)
            plain = check(r, f, gpu)
        with r.frame(0, moments=True) as f:
            f.add(4)
            assert not _same(check(r, f, gpu), plain)         # the luminance stop changes the result


@pytest.mark.parametrize("opts", [dict(iterations=1), dict(iterations=8), dict(sigma_l=0.5, sigma_z=3.0),
                                  dict(normal_power_log2=1)])
def test_options(gpu, opts):
    sc = scenegen.cornell_pt(37, 53, spp=4)
    with rtg.Renderer(sc, device=gpu) as r:
        with r.frame(0, moments=True) as f:
            f.add(4)
            out = check(r, f, gpu, **opts)
            assert not _same(out, f.denoise(resident=True))


def test_window_past_the_first_sample(gpu):
    sc = scenegen.cornell_pt(37, 53, spp=8)
    with rtg.Renderer(sc, device=gpu) as r:
        with r.frame(0, first_sample=3, sample_count=4, moments=True) as f:
            f.add(4)
            check(r, f, gpu)


def test_adaptive_frames(gpu):
    sc = scenegen.cornell_pt(64, 36, spp=64)
    with rtg.Renderer(sc, device=gpu) as r:
        # pixels retired between rounds hold 8 to 16 samples
        with r.frame(0, moments=True, order=1) as f:
            f.add(8)
            left = f.retire(rel_tol=0.1, min_samples=4)
            check(r, f, gpu)
            f.add(8)
            cnt = f.counts()[0]
            print(f"adaptive: {left} of {cnt.size} pixels active, counts {cnt.min()}..{cnt.max()}")
            assert 0 < left < cnt.size and cnt.min() == 8 and cnt.max() == 16
            check(r, f, gpu)
            check(r, f, gpu, demodulate=False, iterations=2)
        # a mask before the first sample: pixels without samples resolve to 0 and carry no variance
        mask = np.zeros((36, 64), np.uint8)
        mask[5:20, 10:40] = 1
        mask[0, 0] = mask[35, 63] = 1
        with r.frame(0, moments=True, order=1) as f:
            f.retire_mask(mask)
            f.add(1)
            check(r, f, gpu)                                   # one sample: no variance, some pixels none at all
            f.add(3)
            cnt = f.counts()[0]
            assert cnt.min() == 0 and cnt.max() == 4
            assert (f.resolve()[5:20, 10:40] == 0).all()
            check(r, f, gpu)
        # every pixel retired, and still so after further rounds that trace nothing
        with r.frame(0, moments=True) as f:
            f.add(4)
            assert f.retire_mask(np.ones((36, 64), np.uint8)) == 0
            a = check(r, f, gpu)
            f.add(4)
            assert f.samples_done == 8 and (f.counts()[0] == 4).all()
            assert _same(check(r, f, gpu), a)


def test_guides_device(gpu):
    import torch

    dev = torch.device(f"cuda:{gpu}")
    ny, nx = 53, 37
    sc = scenegen.cornell_pt(nx, ny, spp=8)
    shapes = dict(rgb=(ny, nx, 3), normal=(ny, nx, 3), depth=(ny, nx), albedo=(ny, nx, 3), variance=(ny, nx))
    with rtg.Renderer(sc, device=gpu) as r:
        a = r.aov(0)
        with r.frame(0, moments=True, order=1) as f:
            for rows, n in ((slice(0, 5), 1), (slice(5, 9), 3), (slice(9, 30), 2)):     # counts 0, 1, 4 and 6
                mask = np.zeros((ny, nx), np.uint8)
                mask[rows, 3:] = 1
                f.retire_mask(mask)
                f.add(n)
            cnt = f.counts()[0]
            assert sorted(set(cnt.reshape(-1).tolist())) == [0, 1, 4, 6]
            # the float32 formula, written out: two divides in this order
            m2 = f.state()["moments"][:, :, 1]
            n = cnt.astype(np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                var = np.where(cnt >= 2, (m2 / (n - np.float32(1))).astype(np.float32) / n, np.float32(0)).astype(np.float32)
            assert _same(var, _variance(f))
            want = dict(rgb=f.resolve(), normal=a["normal"], depth=a["depth"], albedo=a["albedo"], variance=var)
            stream = torch.cuda.Stream(dev)
            for name, shape in shapes.items():               # each array on its own
                t = torch.full(shape, -1.0, dtype=torch.float32, device=dev)
                torch.cuda.synchronize(dev)
                f.guides_device(**{name: t.data_ptr()}, stream=stream.cuda_stream)
                assert _same(t.cpu().numpy(), want[name]), name
            ts = {k: torch.full(s, -1.0, dtype=torch.float32, device=dev) for k, s in shapes.items()}
            torch.cuda.synchronize(dev)
            f.guides_device(**{k: t.data_ptr() for k, t in ts.items()})      # and all at once
            for name in shapes:
                assert _same(ts[name].cpu().numpy(), want[name]), name
            with pytest.raises(A.RtgError, match="RTG_ERR_INVALID"):
                f.guides_device()
        t = torch.full((ny, nx), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        with r.frame(0) as f:                                # no moments
            f.add(4)
            with pytest.raises(A.RtgError, match="RTG_ERR_INVALID"):
                f.guides_device(variance=t.data_ptr())
        with r.frame(0, moments=True) as f:                  # one sample
            f.add(1)
            with pytest.raises(A.RtgError, match="RTG_ERR_INVALID"):
                f.guides_device(variance=t.data_ptr())
            f.guides_device(depth=t.data_ptr())
            assert _same(t.cpu().numpy(), a["depth"])


def test_cache_and_stats(gpu):
    sc = scenegen.cornell_pt(40, 24, spp=16)
    with rtg.Renderer(sc, device=gpu) as r:
        with r.frame(0, moments=True) as f:
            f.add(4)
            first = f.denoise(resident=True)
            st = r.stats()
            assert st["primary_rays"] == st["total_rays"] == 40 * 24 * 16 and st["devices"] == 1
            assert _same(f.denoise(resident=True), first)     # two calls at one state
            assert r.stats() == st
            f.add(4)
            after_add = r.stats()
            assert after_add["primary_rays"] == 40 * 24 * 4
            second = f.denoise(resident=True)
            assert r.stats() == after_add                      # the cache is filled: nothing traced, stats untouched
            assert not _same(second, first)
            assert _same(second, f.denoise())


def test_nothing_disturbed(gpu):
    sc = scenegen.cornell_pt(40, 24, spp=16)
    with rtg.Renderer(sc, device=gpu) as r:
        before = r.render(0)
        with r.frame(0, moments=True) as f:
            f.add(8)
            img, mom, cnt = f.resolve(), f.moments(), f.counts()
            out = f.denoise(resident=True)
            _device_result(f, gpu, demodulate=False, iterations=2)
            assert _same(f.resolve(), img)
            assert all(_same(x, y) for x, y in zip(f.moments(), mom))
            assert all(np.array_equal(x, y) for x, y in zip(f.counts(), cnt))
            assert _same(r.render(0), before)
            st = f.state()
            with r.frame(0, moments=True) as g:               # a checkpoint restored elsewhere filters to the same bits
                g.restore(st)
                assert _same(g.denoise(resident=True), out)
            f.add(8)
            assert _same(f.resolve(), before)                  # continued to its last sample: Renderer.render
            assert _same(f.denoise(resident=True), f.denoise())
        assert _same(r.render(0), before)


def test_refusals(gpu):
    UNSUPPORTED, INVALID = "RTG_ERR_UNSUPPORTED", "RTG_ERR_INVALID"
    sc = scenegen.cornell_pt(32, 18, spp=4)
    out = np.full((18, 32, 3), 7.0, np.float32)
    with rtg.Renderer(sc, device=gpu) as r:
        for kw in (dict(row_stride=2), dict(row_stride=2, compact_rows=1), dict(compact_rows=1)):
            with r.frame(0, moments=True, **kw) as f:
                with pytest.raises(A.RtgError, match=INVALID):               # no samples: ahead of the shard refusal
                    f.denoise(resident=True)
                f.add(4)
                with pytest.raises(A.RtgError, match=UNSUPPORTED):
                    f.denoise(resident=True)
                with pytest.raises(A.RtgError, match=UNSUPPORTED):
                    f.denoise_device(1)                                       # (never written to)
                with pytest.raises(A.RtgError, match=UNSUPPORTED):
                    f.guides_device(rgb=1)
                with pytest.raises(A.RtgError, match=INVALID + ".*iterations"):   # bad options: ahead of it too
                    f.denoise(resident=True, iterations=9)
        with r.frame(0, moments=True) as f:
            with pytest.raises(A.RtgError, match=INVALID + ".*no samples"):
                f.denoise(resident=True)
            with pytest.raises(A.RtgError, match=INVALID + ".*no samples"):
                f.guides_device(rgb=1)
            f.add(1)
            for bad in (dict(iterations=-1), dict(iterations=9), dict(normal_power_log2=11), dict(sigma_l=-1.0),
                        dict(sigma_z=float("nan"))):
                with pytest.raises(A.RtgError, match=INVALID + ".*denoise"):
                    f.denoise(resident=True, **bad)
            assert f.lib.rtg_frame_denoise(f.handle, None, 1, None) == -1
            assert f.lib.rtg_frame_denoise_device(f.handle, None, 1, None, None) == -1
            assert f.lib.rtg_frame_guides_device(f.handle, None, None) == -1
            do = A.DenoiseOpts(0, 0, 0, 0, (C.c_int32 * 4)(0, 0, 1, 0))
            assert f.lib.rtg_frame_denoise(f.handle, C.byref(do), 1, out.ctypes.data_as(A.PF)) == -1
    assert (out == 7.0).all()


def test_lifetime(gpu):
    sc = scenegen.cornell_pt(32, 18, spp=8)
    r = rtg.Renderer(sc, device=gpu)
    f, g = r.frame(0, moments=True), r.frame(0, moments=True, seed=7)
    f.add(2)
    g.add(4)
    outs = []
    for _ in range(2):                                     # two frames of one scene, alternately
        outs.append((f.denoise(resident=True), g.denoise(resident=True)))
    assert _same(outs[0][0], outs[1][0]) and _same(outs[0][1], outs[1][1])
    assert not _same(outs[0][0], outs[0][1])
    assert _same(outs[0][0], f.denoise()) and _same(outs[0][1], g.denoise())
    f.add(2)
    assert _same(f.denoise(resident=True), f.denoise())
    assert _same(g.denoise(resident=True), outs[0][1])
    f.close()                                              # a frame that has denoised goes, then the scene
    assert _same(g.denoise(resident=True), outs[0][1])
    g.close()
    r.close()
    assert r.handle is None


def test_cli_denoise_rounds(gpu, tmp_path):
    sc = scenegen.cornell_pt(32, 24, spp=16)
    sc.cameras[0].image_name = "pt.png"
    xml = write_xml(sc, str(tmp_path / "pt.xml"))
    runs = {"plain": [], "den": ["--denoise"], "prog": ["--progressive", "4"],
            "rounds": ["--progressive", "4", "--denoise-rounds"]}
    out = {}
    for name, extra in runs.items():
        d = tmp_path / name
        d.mkdir()
        p = subprocess.run([native.CLI_PATH, xml, "--out-dir", str(d), "--device", str(gpu), *extra], capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        out[name] = p.stdout.replace(str(d), "<dir>")
    files = lambda name: sorted(x.name for x in (tmp_path / name).iterdir())
    assert files("rounds") == ["pt.png", "pt_denoised.png"] and files("prog") == ["pt.png"]
    assert (tmp_path / "rounds" / "pt_denoised.png").read_bytes() == (tmp_path / "den" / "pt_denoised.png").read_bytes()
    assert (tmp_path / "rounds" / "pt.png").read_bytes() == (tmp_path / "plain" / "pt.png").read_bytes()
    assert out["rounds"] == out["prog"] and out["prog"].count("spp, mean_sem") == 4
    # the library function behind the flag, stopped early by a target error: the file of the round it stopped at
    d = tmp_path / "lib"
    d.mkdir()
    lib = native.load()
    assert lib.rtgh_render_scene_progressive_denoise(xml.encode(), gpu, rtg.render.DEFAULT_SEED, str(d).encode(), 4, 1e9) == 0
    with rtg.Renderer(sc, device=gpu) as r:
        with r.frame(0, moments=True) as f:
            f.add(4)
            assert (d / "pt_denoised.png").read_bytes() == rtg.render.ppm_p3_bytes(f.denoise())
