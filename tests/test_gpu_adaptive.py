"""Adaptive sampling on progressive frames: retired pixels keep their samples and are
traced no further, the others go on; sample order 1 spreads every prefix over the pixel.

The yardstick is the uniform frame, never the code under test: per-sample images come from one-sample
windows in index order (test_gpu_frame._samples, which that file pins to the one-shot render and the
oracle) and are summed in numpy float32 in the order and up to the count each pixel must hold.  Every
comparison of images, moments and retired sets is exact."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import rtg
from rtg import _abi as A
from rtg import native, scenegen
from rtg.scene import parse_xml, write_xml
from test_gpu_frame import SCENES, SCHEDULES, _same, _samples

pytestmark = pytest.mark.gpu

F32 = np.float32
BIG = lambda: scenegen.simple(300, 260)        # 78,000 pixels at 1 spp: 305 blocks of scan partials (two rounds)


def _order(lib, n, order):
    return [lib.rtg_sample_order_index(n, order, j) for j in range(n)]


def _sum_mean(cs, idx):
    """What a frame holds after the samples idx, in that order: the float32 sum, divided when there are several."""
    a = np.zeros_like(cs[0])
    for k in idx:
        a = a + cs[k]
    return a / F32(len(idx)) if len(idx) > 1 else a


def _expected(cs, idx, counts):
    """Per pixel, the mean of the first counts[p] samples in the order idx (0 where a pixel holds none)."""
    out = np.zeros_like(cs[0])
    for c in np.unique(counts):
        if c > 0:
            sel = counts == c
            out[sel] = _sum_mean(cs, idx[:c])[sel]
    return out


def _masks(ny, nx):
    """Active sets (True = traced) for the region-of-interest renders."""
    rng = np.random.default_rng(795)
    flat = rng.permutation(ny * nx)
    out = {}
    m = np.zeros((ny, nx), bool); m[0, 0] = True; out["first"] = m
    m = np.zeros((ny, nx), bool); m[-1, -1] = True; out["last"] = m
    yy, xx = np.mgrid[0:ny, 0:nx]
    out["checker"] = (yy + xx) % 2 == 0
    m = np.zeros((ny, nx), bool); m[5:ny - 3, 6:nx - 5] = True; out["rect"] = m     # straddles the 8x8 tiles and 8-row bands
    for k in (63, 64, 65):
        m = np.zeros(ny * nx, bool); m[flat[:k]] = True; out[f"n{k}"] = m.reshape(ny, nx)
    return out


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("name", ["cornell_pt", "glass_nest", "cornell"])
def test_region_of_interest_at_zero_samples(gpu, name, sched):
    sc = SCENES[name]()
    cam = sc.cameras[0]
    n = cam.num_samples
    with rtg.Renderer(sc, device=gpu) as r:
        for band in (0, 1):                                  # default bands, and bands one tile high
            kw = dict(schedule=SCHEDULES[sched], tile_band=band)
            ref = r.render(0, **kw)
            for mname, act in _masks(cam.ny, cam.nx).items():
                if band == 1 and mname not in ("rect", "n65"):
                    continue
                with r.frame(0, **kw) as f:
                    assert f.active == act.size
                    assert f.retire_mask(~act) == int(act.sum()) == f.active
                    f.add(n)
                    assert r.stats()["primary_rays"] == int(act.sum()) * n, (name, sched, mname)
                    img = f.resolve()
                    cnt, ret = f.counts()
                assert _same(img, np.where(act[..., None], ref, F32(0))), (name, sched, band, mname)
                assert np.array_equal(ret, ~act) and np.array_equal(cnt, np.where(act, n, 0))


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
def test_region_of_interest_over_65536_pixels(gpu, sched):
    sc = BIG()
    cam = sc.cameras[0]
    assert cam.num_samples == 1 and cam.nx * cam.ny == 78000
    rng = np.random.default_rng(2026)
    with rtg.Renderer(sc, device=gpu) as r:
        ref = r.render(0, schedule=SCHEDULES[sched])
        for act in (rng.random((cam.ny, cam.nx)) < 0.3, _masks(cam.ny, cam.nx)["last"]):
            with r.frame(0, schedule=SCHEDULES[sched]) as f:
                assert f.retire_mask(~act) == int(act.sum())
                f.add(1)
                assert r.stats()["primary_rays"] == int(act.sum())
                assert _same(f.resolve(), np.where(act[..., None], ref, F32(0)))
    assert np.any(ref != 0)


def _two_masks(ny, nx):
    rng = np.random.default_rng(14)
    a = rng.random((ny, nx)) < 0.35
    b = rng.random((ny, nx)) < 0.5          # overlaps a: those pixels stay retired with their first count
    return a, b


def _staged(r, lib, name, stages, order=0, moments=False, between=None, **kw):
    """add s0, retire A, add s1, retire B, add s2; checks rays and counts on the way.
    Returns (image, counts, frame moments or None)."""
    cam = r.scene.cameras[0]
    ma, mb = _two_masks(cam.ny, cam.nx)
    npix = ma.size
    s0, s1, s2 = stages
    with r.frame(0, moments=moments, order=order, **kw) as f:
        f.add(s0)
        assert r.stats()["primary_rays"] == npix * s0
        left = f.retire_mask(ma)
        assert left == int((~ma).sum())
        if between:
            between()
        f.add(s1)
        assert r.stats()["primary_rays"] == left * s1
        left = f.retire_mask(mb)
        assert left == int((~ma & ~mb).sum()) == f.active
        if between:
            between()
        f.add(s2)
        assert r.stats()["primary_rays"] == left * s2
        assert f.samples_done == s0 + s1 + s2
        cnt, ret = f.counts()
        want = np.where(ma, s0, np.where(mb, s0 + s1, s0 + s1 + s2))
        assert np.array_equal(cnt, want) and np.array_equal(ret, ma | mb)
        return f.resolve(), cnt, (f.moments() + (f.error(),) if moments else None)


STAGES = {"cornell_pt": (4, 4, 8), "glass_nest": (1, 1, 2), "cornell": (1, 1, 2)}


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("name", sorted(STAGES))
def test_staged_retirement(gpu, lib, name, sched):
    cs, _ = _samples(name)
    n = len(cs)
    with rtg.Renderer(SCENES[name](), device=gpu) as r:
        img, cnt, _ = _staged(r, lib, name, STAGES[name], schedule=SCHEDULES[sched])
    assert sum(STAGES[name]) == n and len(np.unique(cnt)) == 3
    assert _same(img, _expected(cs, list(range(n)), cnt)), (name, sched)


def _uniform_moments(r, counts, order, **kw):
    """(mean, variance) maps of uniform frames stopped at each of `counts`."""
    out = {}
    with r.frame(0, moments=True, order=order, **kw) as f:
        done = 0
        for c in sorted(counts):
            f.add(c - done)
            done = c
            out[c] = f.moments()
    return out


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
def test_staged_moments_and_error_stats(gpu, lib, sched):
    name = "cornell_pt"
    kw = dict(schedule=SCHEDULES[sched])
    with rtg.Renderer(SCENES[name](), device=gpu) as r:
        img, cnt, (mean, var, err) = _staged(r, lib, name, STAGES[name], moments=True, **kw)
        uni = _uniform_moments(r, (4, 8, 16), 0, **kw)
    for c, (um, uv) in uni.items():
        sel = cnt == c
        assert sel.any()
        assert _same(mean[sel], um[sel]) and _same(var[sel], uv[sel]), c
    # the error figures with each pixel's own n, against numpy as test_gpu_frame compares the uniform ones
    sem = np.sqrt(var.astype(np.float64) / cnt)
    assert err["samples_done"] == 16 and err["pixels"] == mean.size
    assert abs(err["max_sem"] - sem.max()) <= 1e-12 * sem.max()
    assert abs(err["mean_sem"] - sem.mean()) <= 1e-9 * sem.mean()
    lum = mean.astype(np.float64).mean()
    assert abs(err["mean_luminance"] - lum) <= 1e-9 * lum
    assert sem.max() > 0


def _decide(state, n, rel_tol, abs_tol):
    """rtg_frame_retire's criterion restated in float64 (include/rtg.h)."""
    mean = state["moments"][..., 0]
    var = state["moments"][..., 1] / F32(n - 1)                       # float32, as rtg_frame_moments returns it
    thr = np.maximum(np.float64(F32(abs_tol)), np.float64(F32(rel_tol)) * mean.astype(np.float64))
    return var.astype(np.float64) / np.float64(n) <= thr * thr


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
def test_builtin_criterion(gpu, sched):
    n = 8
    with rtg.Renderer(SCENES["cornell_pt"](), device=gpu) as r:
        with r.frame(0, moments=True, schedule=SCHEDULES[sched]) as f:
            f.add(n)
            st = f.state()
            npix = st["sums"].shape[0] * st["sums"].shape[1]
            sem = np.sqrt((st["moments"][..., 1] / F32(n - 1)).astype(np.float64) / n)
            abs_tol = float(F32(np.median(sem)))
            want = _decide(st, n, 0.0, abs_tol)
            print(f"median sem {abs_tol:.6g}: {int(want.sum())} of {npix} pixels pass on the uniform frame")
            assert 0 < want.sum() < npix
            # too few samples for the caller's taste: nothing retires
            assert f.retire(abs_tol=1e30, min_samples=n + 1) == npix
            assert not f.counts()[1].any()
            left = f.retire(abs_tol=abs_tol)
            cnt, ret = f.counts()
            assert np.array_equal(ret, want) and left == npix - int(want.sum()) == f.active
            assert np.all(cnt == n)
            # a relative tolerance on top: the retired set only grows, by exactly the pixels that pass it
            rel = 0.25
            more = _decide(st, n, rel, 0.0)
            left = f.retire(rel_tol=rel)
            assert np.array_equal(f.counts()[1], want | more) and left == npix - int((want | more).sum())
            f.add(8)
            assert r.stats()["primary_rays"] == left * 8
            assert np.array_equal(f.counts()[0], np.where(want | more, 8, 16))


@pytest.mark.parametrize("compact", [0, 1])
def test_shards(gpu, compact):
    sc = SCENES["cornell_pt"]()
    cam = sc.cameras[0]
    kw = dict(row_offset=1, row_stride=3, row_block=4, compact_rows=compact)
    owned = [y for y in range(cam.ny) if (y // 4) % 3 == 1]
    rng = np.random.default_rng(5)
    mask = rng.random((len(owned), cam.nx)) < 0.4                     # owned-row shape
    with rtg.Renderer(sc, device=gpu) as r:
        with r.frame(0, **kw) as u:
            u.add(4)
            u4 = u.resolve()
            u.add(12)
            u16 = u.resolve()
        assert _same(u16, r.render(0, **kw))
        with r.frame(0, **kw) as f:
            assert f.rows == len(owned)
            f.add(4)
            assert f.retire_mask(mask) == int((~mask).sum())
            f.add(12)
            assert r.stats()["primary_rays"] == int((~mask).sum()) * 12
            img = f.resolve()
            cnt, _ = f.counts()
        with r.frame(0, **kw) as g:                                  # and a region of interest from the start
            g.retire_mask(mask)
            g.add(16)
            roi = g.resolve()
    full = np.zeros((u16.shape[0], cam.nx), bool)
    if compact:
        full[:] = mask
    else:
        full[owned] = mask
    assert np.array_equal(cnt, np.where(mask, 4, 16))
    assert _same(img, np.where(full[..., None], u4, u16))
    assert _same(roi, np.where(full[..., None], F32(0), u16))
    assert np.any(u16 != 0)


def test_checkpoint_moves_to_another_scene(gpu, lib):
    name = "cornell_pt"
    ma, mb = _two_masks(18, 32)
    with rtg.Renderer(SCENES[name](), device=gpu) as r1, rtg.Renderer(SCENES[name](), device=gpu) as r2:
        with r1.frame(0, moments=True, order=1) as whole, r1.frame(0, moments=True, order=1) as part:
            for f in (whole, part):
                f.add(4); f.retire_mask(ma); f.add(4); f.retire_mask(mb)
            whole.add(8)
            st = part.state()
            assert st["samples_done"] == 8 and np.array_equal(st["retired"], ma | mb)
            with r2.frame(0, moments=True, order=1) as cont:
                cont.restore(st)
                assert cont.samples_done == 8 and cont.active == part.active
                assert _same(cont.resolve(), part.resolve())
                cont.add(8)
                assert r2.stats()["primary_rays"] == part.active * 8
                assert _same(cont.resolve(), whole.resolve())
                (m1, v1), (m2, v2) = cont.moments(), whole.moments()
                assert _same(m1, m2) and _same(v1, v2)
                assert all(np.array_equal(a, b) for a, b in zip(cont.counts(), whole.counts()))
                # restoring the plain state makes every pixel active again
                cont.restore({k: st[k] for k in ("samples_done", "sums", "moments")})
                assert cont.active == ma.size and not cont.counts()[1].any()


def test_all_retired_traces_nothing(gpu):
    with rtg.Renderer(SCENES["cornell_pt"](), device=gpu) as r, r.frame(0) as f:
        f.add(4)
        assert f.retire_mask(np.ones((18, 32), bool)) == 0 and f.active == 0
        img = f.resolve()
        assert f.add(4) == 8
        st = r.stats()
        assert st["primary_rays"] == 0 and st["total_rays"] == 0
        assert _same(f.resolve(), img)
        assert np.all(f.counts()[0] == 4)


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("name", ["cornell_pt", "cornell"])
def test_order_1_sums_the_same_samples_in_its_order(gpu, lib, name, sched):
    cs, _ = _samples(name)
    n = len(cs)
    idx = _order(lib, n, 1)
    assert sorted(idx) == list(range(n)) and (n <= 2 or idx != list(range(n)))
    with rtg.Renderer(SCENES[name](), device=gpu) as r, r.frame(0, order=1, schedule=SCHEDULES[sched]) as f:
        done = 0
        for j in sorted({1, min(5, n), n}):
            f.add(j - done)
            done = j
            assert _same(f.resolve(), _sum_mean(cs, idx[:j])), (name, sched, j)
        # a window of positions: first_sample counts positions too
        with r.frame(0, order=1, first_sample=1, sample_count=2, schedule=SCHEDULES[sched]) as w:
            w.add(2)
            assert _same(w.resolve(), _sum_mean(cs, idx[1:3]))


def test_order_1_with_staged_retirement(gpu, lib):
    name = "cornell_pt"
    cs, _ = _samples(name)
    idx = _order(lib, len(cs), 1)
    with rtg.Renderer(SCENES[name](), device=gpu) as r:
        img, cnt, (mean, var, _) = _staged(r, lib, name, STAGES[name], order=1, moments=True)
        uni = _uniform_moments(r, (4, 8, 16), 1)
    assert _same(img, _expected(cs, idx, cnt))
    for c, (um, uv) in uni.items():
        sel = cnt == c
        assert _same(mean[sel], um[sel]) and _same(var[sel], uv[sel]), c


def test_renders_interleave_with_adaptive_adds(gpu, lib):
    name = "cornell_pt"
    cs, ref = _samples(name)
    with rtg.Renderer(SCENES[name](), device=gpu) as r:
        def between():
            assert _same(r.render(0), ref)
        img, cnt, _ = _staged(r, lib, name, STAGES[name], between=between)
    assert _same(img, _expected(cs, list(range(len(cs))), cnt))


def test_errors(gpu, lib):
    sc = SCENES["cornell"]()
    cam = sc.cameras[0]
    npix = cam.nx * cam.ny
    with rtg.Renderer(sc, device=gpu) as r:
        with pytest.raises(rtg.RtgError):
            r.frame(0, order=2)
        with r.frame(0) as plain, r.frame(0, moments=True) as f:
            plain.add(2)
            with pytest.raises(rtg.RtgError):
                plain.retire(abs_tol=1.0)                        # no moments
            with pytest.raises(rtg.RtgError):
                f.retire(abs_tol=1.0)                            # no samples yet
            f.add(2)
            for bad in (dict(rel_tol=-1.0), dict(abs_tol=float("nan")), dict(rel_tol=float("inf"))):
                with pytest.raises(rtg.RtgError):
                    f.retire(**bad)
            assert f.active == npix
            cnt = np.full(npix, 2, np.int32)
            ret = np.zeros(npix, np.uint8)
            pi, pr = cnt.ctypes.data_as(A.PI), ret.ctypes.data
            cnt[3] = 1                                           # an active pixel must hold samples_done
            assert lib.rtg_frame_set_retired(f.handle, pi, pr) == -1
            ret[3] = 1
            cnt[5] = 3                                           # more than samples_done
            assert lib.rtg_frame_set_retired(f.handle, pi, pr) == -1
            cnt[5] = 2
            assert lib.rtg_frame_set_retired(f.handle, pi, pr) == 0 and f.active == npix - 1
            assert lib.rtg_frame_sample_counts(f.handle, None, None) == 0
        big = scenegen.cornell(8, 6, spp=32769)
        with rtg.Renderer(big, device=gpu) as rb:
            o = rb.opts()
            cd = big.cameras[0].desc()
            h = C.c_void_p()
            fo = A.FrameOpts(0, 0, 0, 1)
            assert lib.rtg_frame_create(rb.handle, C.byref(cd), C.byref(o), C.byref(fo), C.byref(h)) == -5


def test_cli_adaptive(gpu, tmp_path):
    sc = scenegen.cornell_pt(32, 24, spp=16)
    sc.cameras[0].image_name = "adapt.exr"
    xml = write_xml(sc, str(tmp_path / "adapt.xml"))
    out = tmp_path / "cli"
    out.mkdir()
    p = subprocess.run([native.CLI_PATH, xml, "--out-dir", str(out), "--device", str(gpu), "--progressive", "4",
                        "--adaptive", "0.1", "--min-samples", "8"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    rounds = [ln for ln in p.stdout.splitlines() if " spp, mean_sem " in ln]
    active = [int(ln.rsplit(", active ", 1)[1]) for ln in rounds]
    with rtg.Renderer(parse_xml(xml), device=gpu) as r, r.frame(0, moments=True, order=1) as f:
        want = []
        while f.samples_done < 16 and f.active > 0:
            f.add(4)
            want.append(f.retire(rel_tol=0.1, min_samples=8))
        img = f.resolve()
    assert active == want and want[0] == 32 * 24 and 0 < want[-1] < want[0]
    rtg.save_image(str(tmp_path / "adapt.exr"), img)
    assert (out / "adapt.exr").read_bytes() == (tmp_path / "adapt.exr").read_bytes()
