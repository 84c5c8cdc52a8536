"""Progressive frames (rtg_frame): a device-resident accumulator that takes a camera's
samples in chunks.  Sample k of a pixel is the same ray tree whichever call traces it, and the
per-pixel sum continues in sample order (Scene::MultiSample, src/Scene.cpp:386-411), so any chunking
resolves to the bits of the one-shot render -- on both schedules, with any batch size, on row shards,
interleaved with other renders, and across a checkpoint.  With moments the frame also keeps Welford's
running mean and M2 of the samples' luminance, from which the error figures are reduced."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import pyoracle
import rtg
from rtg import _abi as A
from rtg import native, scenegen
from rtg.scene import parse_xml, write_xml

pytestmark = pytest.mark.gpu

SCENES = {
    "cornell_pt": lambda: scenegen.cornell_pt(32, 18, spp=16),                # path tracer, every flag, stream by default
    "glass_nest": lambda: scenegen.glass_nest(32, 24, spp=4, max_depth=6),    # Whitted, two children per level
    "cornell": lambda: scenegen.cornell(36, 27, spp=4),                       # DoF, blur, area light
    "multilight": lambda: scenegen.multilight(40, 30),                        # 1 spp: SingleSample (mode 2)
}
SCHEDULES = {"passes": A.SCHEDULE_PASSES, "stream": A.SCHEDULE_STREAM}
F32 = np.float32


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _chunkings(n):
    return ((n,), (1,) * n, (3, 5, n - 8) if n >= 9 else (1, n - 1) if n >= 2 else (1,))


def _rays(st):
    return np.array([st["primary_rays"], st["secondary_rays"], st["shadow_rays"]], np.int64)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    o = pyoracle.Oracle(SCENES[name]())
    ref, _, _, _ = o.render(0)
    o.close()
    return ref


@functools.lru_cache(maxsize=None)
def _samples(name):
    """(c_k for every sample k of camera 0, from one-sample windows; the one-shot render)."""
    sc = SCENES[name]()
    n = sc.cameras[0].num_samples
    with rtg.Renderer(sc, device=0) as r:
        cs = []
        for k in range(n):
            with r.frame(0, first_sample=k, sample_count=1) as f:
                assert f.add(1) == 1
                cs.append(f.resolve())
        return cs, r.render(0)


def _prefix_mean(cs, j):
    a = np.zeros_like(cs[0])
    for k in range(j):
        a = a + cs[k]
    return a / F32(j)


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_any_chunking_equals_the_one_shot_frame(gpu, name, sched):
    sc = SCENES[name]()
    n = sc.cameras[0].num_samples
    with rtg.Renderer(sc, device=gpu) as r:
        for batch, streams in ((0, 0), (300, 1), (1000, 3)):
            kw = dict(schedule=SCHEDULES[sched], max_batch_rays=batch, streams=streams)
            if sched == "stream":
                kw["segment_nodes"] = 4200
            ref = r.render(0, **kw)
            rays0 = _rays(r.stats())
            for chunks in _chunkings(n):
                with r.frame(0, **kw) as f:
                    rays = np.zeros(3, np.int64)
                    for c in chunks:
                        f.add(c)
                        rays += _rays(r.stats())
                    assert f.samples_done == n
                    assert _same(f.resolve(), ref), (name, sched, batch, streams, chunks)
                    assert (rays == rays0).all(), (name, sched, batch, streams, chunks)
            if name in ("cornell_pt", "glass_nest"):
                assert _same(np.nan_to_num(ref), np.nan_to_num(_oracle(name)))


@pytest.mark.parametrize("name", ["cornell_pt", "cornell"])
def test_windows_are_the_same_samples(gpu, name):
    cs, ref = _samples(name)
    n = len(cs)
    assert _same(_prefix_mean(cs, n), ref)
    with rtg.Renderer(SCENES[name](), device=gpu) as r, r.frame(0) as f:
        done = 0
        for j in sorted({1, min(5, n), n}):        # prefixes of 1, 5 and n samples (n where n < 5)
            f.add(j - done)
            done = j
            assert _same(f.resolve(), _prefix_mean(cs, j)), (name, j)


@pytest.mark.parametrize("compact", [0, 1])
def test_shard_frames(gpu, compact):
    sc = SCENES["cornell_pt"]()
    kw = dict(row_offset=1, row_stride=3, row_block=4, compact_rows=compact)
    with rtg.Renderer(sc, device=gpu) as r:
        ref = r.render(0, **kw)
        with r.frame(0, **kw) as f:
            for c in (3, 5, 8):
                f.add(c)
            img = f.resolve()
    assert img.shape == ref.shape and _same(img, ref)
    assert np.any(ref != 0)


def test_frames_and_renders_interleave(gpu):
    sc = SCENES["cornell_pt"]()
    with rtg.Renderer(sc, device=gpu) as r:
        ra, rb, rc = r.render(0, seed=11), r.render(0, seed=22), r.render(0)
        with r.frame(0, seed=11) as fa, r.frame(0, seed=22) as fb:
            fa.add(3)
            assert _same(r.render(0), rc)
            fb.add(5)
            fa.add(13)
            assert _same(r.render(0), rc)
            fb.add(11)
            assert _same(fa.resolve(), ra) and _same(fb.resolve(), rb)
    assert not _same(ra, rb)


def _lum64(c):
    c = c.astype(np.float64)
    y = (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]
    return np.where(np.isfinite(y) & (y > 0), y, 0.0)


def test_moments_and_error_figures(gpu):
    cs, _ = _samples("cornell_pt")
    n = len(cs)
    assert n == 16
    Y = np.stack([_lum64(c) for c in cs])                   # (n, ny, nx) float64
    ymax = Y.max(axis=0)
    mean64, var64 = Y.mean(axis=0), Y.var(axis=0, ddof=1)
    # the bound below must be tight enough to tell / n from / (n - 1): on the float64 reference alone
    lit = ymax > 0
    spread = float(np.median(var64[lit] / ymax[lit] ** 2))
    print(f"median var64 / max Y^2 over {int(lit.sum())} lit pixels: {spread:.4g}")
    assert spread > 1e-2
    maps = []
    with rtg.Renderer(SCENES["cornell_pt"](), device=gpu) as r:
        for chunks in _chunkings(n):
            with r.frame(0, moments=True) as f:
                for c in chunks:
                    f.add(c)
                mean, var = f.moments()
                e1, e2 = f.error(), f.error()
            maps.append((mean, var))
            em, ev = np.abs(mean - mean64), np.abs(var - var64)
            print(f"chunks {chunks[:3]}..: max |mean - mean64| / bound = {np.max(em / np.maximum(4 * n * 2.0**-24 * ymax, 1e-300)):.4g}, "
                  f"max |var - var64| / bound = {np.max(ev / np.maximum(16 * n * 2.0**-24 * ymax**2, 1e-300)):.4g}")
            assert np.all(em <= 4 * n * 2.0 ** -24 * ymax)
            assert np.all(ev <= 16 * n * 2.0 ** -24 * ymax ** 2)
            sem = np.sqrt(var.astype(np.float64) / n)
            assert e1 == e2
            assert e1["samples_done"] == n and e1["pixels"] == mean.size
            assert abs(e1["max_sem"] - sem.max()) <= 1e-12 * sem.max()
            assert abs(e1["mean_sem"] - sem.mean()) <= 1e-9 * sem.mean()
            lum = mean.astype(np.float64).mean()
            assert abs(e1["mean_luminance"] - lum) <= 1e-9 * lum
        for mean, var in maps[1:]:
            assert _same(mean, maps[0][0]) and _same(var, maps[0][1])


def test_one_sample_has_no_variance(gpu):
    sc = SCENES["multilight"]()
    with rtg.Renderer(sc, device=gpu) as r, r.frame(0, moments=True) as f:
        f.add(1)
        mean, var = f.moments()
        img = f.resolve()
        e = f.error()
    assert np.all(var == 0) and e["max_sem"] == 0.0 and e["mean_sem"] == 0.0
    assert np.allclose(mean, _lum64(img), rtol=1e-6, atol=0)


def test_state_moves_to_another_scene(gpu):
    sc = SCENES["cornell_pt"]()
    with rtg.Renderer(sc, device=gpu) as r1, rtg.Renderer(SCENES["cornell_pt"](), device=gpu) as r2:
        with r1.frame(0, moments=True) as whole, r1.frame(0, moments=True) as part:
            whole.add(16)
            part.add(5)
            st = part.state()
            assert st["samples_done"] == 5
            with r2.frame(0, moments=True) as cont:
                cont.restore(st)
                assert cont.samples_done == 5
                assert _same(cont.resolve(), part.resolve())
                cont.add(11)
                assert _same(cont.resolve(), whole.resolve())
                (m1, v1), (m2, v2) = cont.moments(), whole.moments()
                assert _same(m1, m2) and _same(v1, v2)


def test_errors(gpu, lib):
    sc = SCENES["cornell"]()
    n = sc.cameras[0].num_samples
    cd = sc.cameras[0].desc()

    def refused(rc, code=-1):
        assert rc == code, (rc, lib.rtg_last_error())
        assert lib.rtg_last_error()

    with rtg.Renderer(sc, device=gpu) as r:
        def create(fo=None, **kw):
            o = r.opts(**kw)
            h = C.c_void_p()
            rc = lib.rtg_frame_create(r.handle, C.byref(cd), C.byref(o), None if fo is None else C.byref(fo), C.byref(h))
            return rc, h

        # the multi-GPU fan-out of frames is out of scope
        refused(create(num_devices=2)[0], -5)
        refused(create(devices=[gpu])[0], -5)
        # windows outside [0, num_samples)
        for first, count in ((-1, 0), (n, 0), (2, n - 1), (0, n + 1), (0, -1)):
            refused(create(A.FrameOpts(first, count, 0, 0))[0])
        buf = np.zeros((sc.cameras[0].ny, sc.cameras[0].nx, 3), F32)
        pf = buf.ctypes.data_as(A.PF)
        err = A.FrameError()
        rc, h = create(A.FrameOpts(1, 2, 1, 0))                      # samples 1 and 2, with moments
        assert rc == 0
        # nothing accumulated yet
        refused(lib.rtg_frame_resolve(h, pf))
        refused(lib.rtg_frame_moments(h, pf, None))
        refused(lib.rtg_frame_error_stats(h, C.byref(err)))
        # counts
        for c in (0, -3, 3):
            refused(lib.rtg_frame_add_samples(h, c, None))
        assert lib.rtg_frame_add_samples(h, 2, None) == 0
        refused(lib.rtg_frame_add_samples(h, 1, None))              # the window is used up
        refused(lib.rtg_frame_set_state(h, 3, pf, pf))
        refused(lib.rtg_frame_set_state(h, -1, pf, pf))
        assert lib.rtg_frame_samples_done(h) == 2
        assert lib.rtg_frame_error_stats(h, C.byref(err)) == 0 and err.samples_done == 2
        # no moments on a frame created without them
        rc, h2 = create()
        assert rc == 0 and lib.rtg_frame_add_samples(h2, n, None) == 0
        refused(lib.rtg_frame_moments(h2, pf, None))
        refused(lib.rtg_frame_error_stats(h2, C.byref(err)))
        # a scene with live frames stays, and stays usable
        refused(lib.rtg_scene_destroy(r.handle))
        assert lib.rtg_frame_set_state(h2, 0, None, None) == 0
        assert lib.rtg_frame_add_samples(h2, n, None) == 0
        assert lib.rtg_frame_resolve(h2, pf) == 0
        assert _same(buf, r.render(0))
        assert lib.rtg_frame_destroy(h) == 0 and lib.rtg_frame_destroy(h2) == 0


def test_cli_progressive(gpu, tmp_path):
    sc = scenegen.cornell_pt(32, 24, spp=16)
    sc.cameras[0].image_name = "prog.exr"
    sc.cameras[0].tonemap = (0.18, 1.0, 1.0, 2.2)
    xml = write_xml(sc, str(tmp_path / "prog.xml"))
    dirs = {k: tmp_path / k for k in ("plain", "full", "early", "py")}
    for d in dirs.values():
        d.mkdir()

    def cli(out, *extra):
        return subprocess.run([native.CLI_PATH, xml, "--out-dir", str(out), "--device", str(gpu), *extra],
                              capture_output=True, text=True, timeout=120)

    p = cli(dirs["plain"])
    assert p.returncode == 0, p.stderr
    p = cli(dirs["full"], "--progressive", "4")
    assert p.returncode == 0, p.stderr
    rounds = [ln for ln in p.stdout.splitlines() if " spp, mean_sem " in ln]
    assert [ln.split(": ")[1].split(" spp")[0] for ln in rounds] == ["4/16", "8/16", "12/16", "16/16"]
    for name in ("prog.exr", "prog.png"):
        assert (dirs["full"] / name).read_bytes() == (dirs["plain"] / name).read_bytes(), name
    # a target any frame meets: one round, whose files are those of a 4-sample frame
    p = cli(dirs["early"], "--progressive", "4", "--target-error", "1e30")
    assert p.returncode == 0, p.stderr
    assert len([ln for ln in p.stdout.splitlines() if " spp, mean_sem " in ln]) == 1
    with rtg.Renderer(parse_xml(xml), device=gpu) as r, r.frame(0) as f:
        f.add(4)
        img = f.resolve()
    rtg.save_image(str(dirs["py"] / "prog.exr"), img)
    rtg.save_image(str(dirs["py"] / "prog.png"), rtg.tonemap(img, *sc.cameras[0].tonemap, device=gpu))
    for name in ("prog.exr", "prog.png"):
        assert (dirs["early"] / name).read_bytes() == (dirs["py"] / name).read_bytes(), name
    p = cli(dirs["early"], "--progressive", "4", "--devices", "2")
    assert p.returncode == 2 and "--devices" in p.stderr
