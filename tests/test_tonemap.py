"""hw5 Photographic tone mapping (pages/Page5.md:47-53 describes a global
operator, src/ has no code).  CPU: the oracle's restatement against closed forms; GPU:
rtg_tonemap against the oracle."""
import numpy as np
import pytest

import pyoracle
import rtg


def _gray(v, h=6, w=9):
    return np.full((h, w, 3), v, np.float32)


def test_constant_gray_maps_to_white():
    """A uniform gray image: L = key * Y / (Y + 1e-5) ~ key = Lwhite (burn 0), so Ld = 1."""
    out = pyoracle.tonemap(_gray(3.0), key=0.18, burn=0.0, gamma=2.2)
    assert np.allclose(out, 255.0, atol=1e-3)


def test_reinhard_curve_without_white_point():
    """burn 100 picks the darkest pixel as Lwhite (0 here): Ld = L / (1 + L), gamma 1."""
    img = np.zeros((4, 4, 3), np.float32)
    img[0, 0] = 10.0
    img[1, 1] = 2.0
    out = pyoracle.tonemap(img, key=0.5, burn=100.0, saturation=1.0, gamma=1.0)
    n = 16
    lw = np.exp((np.log(1e-5 + 10.0) + np.log(1e-5 + 2.0) + 14 * np.log(1e-5)) / n)
    for y, v in ((0, 10.0), (1, 2.0)):
        L = np.float32(0.5 / lw) * np.float32(v)
        assert abs(out[y, y, 0] - 255.0 * min(1.0, L / (1 + L))) < 1e-3
    assert out[2, 2].max() == 0.0


def test_saturation_and_monotonicity():
    rng = np.random.default_rng(5)
    img = (rng.random((20, 30, 3)) ** 3 * 50).astype(np.float32)
    out = pyoracle.tonemap(img, key=0.18, burn=2.0, saturation=0.5)
    assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= 255
    y = (0.2126 * img[..., 0] + 0.7152 * img[..., 1]) + 0.0722 * img[..., 2]
    g = pyoracle.tonemap(np.repeat(y[..., None], 3, 2).astype(np.float32), key=0.18, burn=2.0)
    order = np.argsort(y.ravel())
    assert (np.diff(g[..., 0].ravel()[order]) >= -1e-3).all()      # monotone in luminance


def _tonemap_f64(img, key, burn, saturation, gamma):
    """DESIGN.md §11 in float64 numpy: luminance, log-average, burn rank, curve, saturation, gamma.  The image
    and the four parameters are rounded to float32 first, as the ABI hands them on."""
    c = np.asarray(np.asarray(img, np.float32), np.float64).reshape(-1, 3)
    key, burn, saturation, gamma = (float(np.float32(v)) for v in (key, burn, saturation, gamma))
    y = (0.2126 * c[:, 0] + 0.7152 * c[:, 1]) + 0.0722 * c[:, 2]
    lw = np.exp(np.mean(np.log(1e-5 + y)))
    lum = (key / lw) * y
    rank = int(np.floor((y.size - 1) * (1.0 - burn / 100.0)))
    white = np.sort(lum)[rank]
    ld = lum * (1.0 + lum / white ** 2) / (1.0 + lum)
    out = 255.0 * np.clip(ld[:, None] * (c / y[:, None]) ** saturation, 0.0, 1.0) ** (1.0 / gamma)
    return out.reshape(np.shape(img)), rank, np.sort(lum)


def _edge_image(n, burn):
    """n strictly positive pixels in one row whose luminance at the burn rank is repeated: the pixel of that rank
    is copied over its two neighbours in the sorted order (the two below it where none lies above)."""
    rng = np.random.default_rng(1000 * n + int(burn))
    img = (rng.random((1, n, 3)) ** 4 * 1000 + 0.01).astype(np.float32)
    _, rank, _ = _tonemap_f64(img, 0.18, burn, 1.0, 2.2)
    c = img[0].astype(np.float64)
    order = np.argsort((0.2126 * c[:, 0] + 0.7152 * c[:, 1]) + 0.0722 * c[:, 2], kind="stable")
    ties = [r for r in ((rank + 1, rank + 2) if rank + 2 < n else (rank - 1, rank - 2)) if 0 <= r < n]
    for r in ties:
        img[0, order[r]] = img[0, order[rank]]
    return img


EDGE_CASES = [(n, burn) for n in (1, 255, 256, 257, 65537) for burn in (0.0, 50.0, 100.0)]
# 1 pixel; either side of the 256-thread block; more partial sums than k_tm_scale has threads


def _edge_reference(n, burn, cache={}):
    if (n, burn) not in cache:
        img = _edge_image(n, burn)
        ref, rank, lum = _tonemap_f64(img, 0.18, burn, 0.7, 2.2)
        if n >= 255:            # the rank's luminance is repeated, and the frame is not all black or all white
            assert np.count_nonzero(lum == lum[rank]) >= 3
            if burn < 100.0:
                assert ref.min() < 128 < ref.max()
            else:               # Lwhite is the darkest pixel: Ld >= 1 everywhere, only the channel ratios show
                assert (ref.max(axis=-1) == 255.0).all()
        cache[(n, burn)] = (img, ref)
    return cache[(n, burn)]


@pytest.mark.parametrize("n,burn", EDGE_CASES)
def test_oracle_tonemap_matches_float64(n, burn):
    img, ref = _edge_reference(n, burn)
    got = pyoracle.tonemap(img, key=0.18, burn=burn, saturation=0.7, gamma=2.2)
    assert np.isfinite(got).all()
    assert np.abs(got.astype(np.float64) - ref).max() < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("n,burn", EDGE_CASES)
def test_gpu_tonemap_matches_float64(gpu, n, burn):
    img, ref = _edge_reference(n, burn)
    got = rtg.tonemap(img, key=0.18, burn=burn, saturation=0.7, gamma=2.2, device=gpu)
    assert np.isfinite(got).all()
    assert np.abs(got.astype(np.float64) - ref).max() < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("shape,burn,sat,gamma", [((1080, 1920), 1.0, 1.0, 2.2), ((37, 53), 0.0, 0.7, 1.8),
                                                  ((64, 64), 100.0, 1.2, 2.4)])
def test_gpu_tonemap_matches_oracle(gpu, shape, burn, sat, gamma):
    rng = np.random.default_rng(7)
    img = (rng.random(shape + (3,)) ** 4 * 1000).astype(np.float32)
    img[0, :5] = [[0, 0, 0], [np.nan, 1, 1], [np.inf, 0, 0], [-5, 2, 2], [1e30, 1e30, 1e30]]
    got = rtg.tonemap(img, key=0.18, burn=burn, saturation=sat, gamma=gamma, device=gpu)
    ref = pyoracle.tonemap(img, key=0.18, burn=burn, saturation=sat, gamma=gamma)
    assert np.isfinite(got).all()
    assert np.abs(got.astype(np.float64) - ref).max() < 1e-3
