"""The primary-ray generators of rtg.rays: shapes, dtypes, unit directions, and the float32
results against float64 closed forms written out here.  Tolerance 1e-6: a float32 rounding of a value of
magnitude <= 4 is at most 2.4e-7 away from it."""
import numpy as np
import pytest

import rtg
from rtg import rays

TOL = 1e-6


def check_layout(o, d, t, nx, ny, spp):
    assert o.shape == (ny, nx, spp, 3) and d.shape == (ny, nx, spp, 3) and t.shape == (ny, nx, spp)
    assert o.dtype == np.float32 and d.dtype == np.float32 and t.dtype == np.float32
    assert o.flags.c_contiguous and d.flags.c_contiguous and t.flags.c_contiguous
    assert not t.any()
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1.0).max() <= TOL


def test_exported():
    assert rtg.equirect_rays is rays.equirect_rays and rtg.ortho_rays is rays.ortho_rays
    assert "equirect_rays" in rtg.__all__ and "ortho_rays" in rtg.__all__


@pytest.mark.parametrize("forward,up", [((0, 0, -1), (0, 1, 0)), ((1, 0, 0), (0, 0, 1)), ((1, 2, -2), (0.5, 1, 0.25))])
def test_equirect_pixel_centres(forward, up):
    nx, ny = 33, 17                                   # odd: a centre column and a centre row exist
    pos = (1.5, -2.0, 0.25)
    o, d, t = rays.equirect_rays(pos, nx, ny, forward=forward, up=up)
    check_layout(o, d, t, nx, ny, 1)
    assert np.abs(o.astype(np.float64) - np.asarray(pos)).max() <= TOL
    u = np.asarray(up, np.float64) / np.linalg.norm(up)
    f = np.asarray(forward, np.float64)
    f = f - f.dot(u) * u
    f /= np.linalg.norm(f)
    r = np.cross(f, u)
    D = d[:, :, 0].astype(np.float64)
    # the centre pixel looks along forward; the centre column has no sideways component
    assert np.abs(D[ny // 2, nx // 2] - f).max() <= TOL
    assert np.abs(D[:, nx // 2] @ r).max() <= TOL
    # the top row tends to up, the bottom row to -up: half a pixel of polar angle away
    assert np.abs(D[0] @ u - np.cos(0.5 * np.pi / ny)).max() <= TOL
    assert np.abs(D[-1] @ u + np.cos(0.5 * np.pi / ny)).max() <= TOL
    # every row at its polar angle, every column at its azimuth, adjacent columns 2 pi / nx apart
    theta = (np.arange(ny) + 0.5) * np.pi / ny
    assert np.abs(D @ u - np.cos(theta)[:, None]).max() <= TOL
    az = np.arctan2(D @ r, D @ f)
    want = ((np.arange(nx) + 0.5) / nx - 0.5) * 2 * np.pi
    mid = slice(1, ny - 1)                            # (near the poles the azimuth of a float32 vector is ill-conditioned)
    assert np.abs(az[mid] - want[None, :]).max() <= TOL / np.sin(theta[1])
    step = np.diff(az[ny // 2])
    assert np.abs(step - 2 * np.pi / nx).max() <= 2 * TOL
    # the closed form itself
    full = (np.sin(theta)[:, None, None] * (np.cos(want)[None, :, None] * f + np.sin(want)[None, :, None] * r)
            + np.cos(theta)[:, None, None] * u)
    assert np.abs(D - full).max() <= TOL


def test_ortho_pixel_centres():
    nx, ny, w, h = 12, 7, 3.0, 1.75
    pos, gaze, up = (0.5, 1.0, -2.0), (1.0, -1.0, -2.0), (0.0, 1.0, 0.0)
    o, d, t = rays.ortho_rays(pos, gaze, up, w, h, nx, ny)
    check_layout(o, d, t, nx, ny, 1)
    g = np.asarray(gaze, np.float64) / np.linalg.norm(gaze)
    assert np.abs(d.astype(np.float64) - g).max() <= TOL
    assert (d == d[0, 0, 0]).all()
    r = np.cross(g, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    u2 = np.cross(r, g)
    rel = o[:, :, 0].astype(np.float64) - np.asarray(pos)
    assert np.abs(rel @ g).max() <= TOL                                  # the plane through `position`
    x, y = rel @ r, rel @ u2
    assert np.abs(x - ((np.arange(nx) + 0.5) / nx - 0.5)[None, :] * w).max() <= TOL
    assert np.abs(y - (0.5 - (np.arange(ny) + 0.5) / ny)[:, None] * h).max() <= TOL
    assert np.abs(np.diff(x, axis=1) - w / nx).max() <= 2 * TOL and np.abs(np.diff(y, axis=0) + h / ny).max() <= 2 * TOL
    assert abs((x.max() - x.min()) - (w - w / nx)) <= 2 * TOL and abs((y.max() - y.min()) - (h - h / ny)) <= 2 * TOL


@pytest.mark.parametrize("spp", [2, 3, 4, 7])
def test_jitter_is_stratified_and_seeded(spp):
    nx, ny = 9, 5
    g = int(np.ceil(np.sqrt(spp)))
    a = rays.ortho_rays((0, 0, 0), (0, 0, -1), (0, 1, 0), nx, ny, nx, ny, spp=spp, seed=11)
    b = rays.ortho_rays((0, 0, 0), (0, 0, -1), (0, 1, 0), nx, ny, nx, ny, spp=spp, seed=11)
    c = rays.ortho_rays((0, 0, 0), (0, 0, -1), (0, 1, 0), nx, ny, nx, ny, spp=spp, seed=12)
    check_layout(*a, nx, ny, spp)
    for p, q in zip(a, b):
        assert np.array_equal(p.view(np.int32), q.view(np.int32))
    assert not np.array_equal(a[0], c[0])
    # one film unit per pixel here: the sample's offset inside its pixel lies in its cell of the g x g grid
    fx = a[0][..., 0].astype(np.float64) + nx / 2 - np.arange(nx)[None, :, None]
    fy = ny / 2 - a[0][..., 1].astype(np.float64) - np.arange(ny)[:, None, None]
    s = np.arange(spp)
    assert (fx >= (s % g) / g - TOL).all() and (fx <= (s % g + 1) / g + TOL).all()
    assert (fy >= (s // g) / g - TOL).all() and (fy <= (s // g + 1) / g + TOL).all()
    assert len(np.unique(fx)) > nx * ny                                  # jittered, not the cell centres
    e = rays.equirect_rays((0, 0, 0), nx, ny, spp=spp, seed=11)
    e2 = rays.equirect_rays((0, 0, 0), nx, ny, spp=spp, seed=11)
    check_layout(*e, nx, ny, spp)
    assert np.array_equal(e[1].view(np.int32), e2[1].view(np.int32))


def test_one_sample_draws_nothing():
    a = rays.equirect_rays((0, 0, 0), 8, 4, seed=1)
    b = rays.equirect_rays((0, 0, 0), 8, 4, seed=2)
    assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def test_bad_arguments():
    with pytest.raises(ValueError):
        rays.equirect_rays((0, 0, 0), 0, 4)
    with pytest.raises(ValueError):
        rays.equirect_rays((0, 0, 0), 8, 4, forward=(0, 2, 0))           # parallel to up
    with pytest.raises(ValueError):
        rays.ortho_rays((0, 0, 0), (0, 0, 0), (0, 1, 0), 1, 1, 4, 4)
    with pytest.raises(ValueError):
        rays.ortho_rays((0, 0, 0), (0, 1, 0), (0, 1, 0), 1, 1, 4, 4)
