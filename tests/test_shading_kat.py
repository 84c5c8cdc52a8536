"""Known answers of the Whitted shading arithmetic: the oracle's 4x3 frames against float64 closed forms written
from the reference's text (tests/shading_ref.py), on scenes of horizontal planes (tests/shading_cases.py).
The parity tests compare the GPU with the oracle; both restate src/Light.cpp and src/Scene.cpp by the same
reading, so a swapped rs / rp, a wrong normaliser or a dropped 1 - F would sit in both.  Here each light term,
BRDF, Fresnel term, Beer factor and recursion weight has to equal the formula itself.

Bound: |oracle - closed form| <= 1e-5 x (the pixel's largest closed-form channel), per channel: about 170
float32 roundings for a chain of a few dozen operations plus a pow, which multiplies its base's error by the
exponent (50 at the most).  Worst deviation seen per family, as a share of the pixel's largest channel:

    point 6.2e-7, directional 2.8e-7, spot 3.1e-6 (the falloff's difference of cosines), area 1.8e-6,
    environment 1.2e-6, area + spot 1.1e-6, grazing cut 1.8e-7, shadow 5.0e-7, mirror / conductor 4.3e-7,
    glass slab 1.1e-6, four samples 2.3e-7.
"""
import numpy as np
import pytest

import pyoracle
import shading_cases as S


def _oracle(sc):
    o = pyoracle.Oracle(sc)
    try:
        return o.render(0, seed=S.SEED)[0]
    finally:
        o.close()


def _check(sc, what):
    img, ref = S.reference(sc, pyoracle.rng_uniform)
    S.assert_lit(sc, img, pyoracle.rng_uniform, what)
    S.assert_close(_oracle(sc), img, what)
    return img, ref


def test_winding_gives_the_normals():
    """add_rect's two windings, seen by the oracle's own intersection: the floor's normal is +y, the ceiling's -y."""
    o = pyoracle.Oracle(S.reflector("mirror", 2))
    h = o.trace([[0.1, 0, -0.2], [0.1, 0, -0.2]], [[0.1, -1, 0.05], [0.05, 1, 0.1]])
    o.close()
    assert h["full"].tolist() == [1, 1] and h["object"].tolist() == [0, 1]
    assert h["normal"].tolist() == [[0, 1, 0], [0, -1, 0]]
    assert np.allclose(h["point"][:, 1], [-1, 4], atol=1e-6)


@pytest.mark.parametrize("exponent", S.EXPONENTS, ids=lambda p: f"p{p}")
@pytest.mark.parametrize("brdf", list(S.BRDFS))
@pytest.mark.parametrize("kind", S.LIGHTS)
def test_direct(kind, brdf, exponent):
    _check(S.direct(kind, brdf, exponent), f"{kind}-{brdf}-p{exponent}")


def test_area_and_spot_together():
    _check(S.direct("area", "none", 8, extra=("spot",)), "area+spot")


@pytest.mark.parametrize("brdf", ["op", "obp", "mp", "mbp"])
def test_grazing_light_cut(brdf):
    """cos theta_i = 0.0005: the "original" forms return 0 for that light, the modified ones do not."""
    sc = S.grazing(brdf)
    img, _ = _check(sc, f"grazing-{brdf}")
    one = S.reference(S.direct("directional", brdf, 8), pyoracle.rng_uniform)[0]
    if brdf in ("op", "obp"):
        assert np.array_equal(img, one)
    else:
        assert ((img - one).max(axis=-1) > 0.05 * one.max(axis=-1)).all()


def test_spot_zones():
    sc = S.direct("spot", "none", 8)
    _, ref = _check(sc, "spot zones")
    zones = S.spot_zones(ref)
    assert min(zones) >= 2, zones


def test_shadow():
    sc = S.shadow()
    _, ref = _check(sc, "shadow")
    lit, dark, least = S.shadow_census(ref)
    assert lit >= 3 and dark >= 3 and least > 0.05, (lit, dark, least)


@pytest.mark.parametrize("kind", ["mirror", "conductor"])
def test_reflector(kind):
    """Depth 2: the floor's own shading plus the weighted shading of the ceiling it reflects."""
    sc = S.reflector(kind, 2)
    img, _ = _check(sc, f"{kind}-d2")
    flat = S.reference(S.reflector(kind, 0), pyoracle.rng_uniform)[0]
    assert ((img - flat).max(axis=-1) > 0.01 * flat.max(axis=-1)).all()        # the reflection carries weight


@pytest.mark.parametrize("kind", ["mirror", "conductor"])
def test_depth_zero_is_basic_shading(kind):
    sc = S.reflector(kind, 0)
    img, _ = _check(sc, f"{kind}-d0")
    plain = S.reflector(kind, 0)
    plain.materials[0].type = S.A.MAT_NORMAL
    assert np.array_equal(img, S.reference(plain, pyoracle.rng_uniform)[0])
    assert np.array_equal(S.bits(_oracle(sc)), S.bits(_oracle(plain)))


@pytest.mark.parametrize("depth", [1, 2, 4, 6], ids=lambda d: f"d{d}")
@pytest.mark.parametrize("absorption", [(0.0, 0.0, 0.0), (0.3, 0.6, 0.9)], ids=["clear", "absorbing"])
def test_glass_slab(absorption, depth):
    sc = S.slab(absorption, depth)
    _, ref = _check(sc, f"slab-{absorption}-d{depth}")
    S.assert_slab(ref, any(absorption))


def test_four_samples():
    """The only case through sample accumulation: the mean of four closed-form samples."""
    _check(S.multisample(), "multisample")
