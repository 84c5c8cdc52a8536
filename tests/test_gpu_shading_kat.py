"""Renderer.render against the float64 closed forms of tests/shading_ref.py, directly and not through the
oracle: the scenes, the bound (1e-5 of the pixel's largest closed-form channel) and the vacuity conditions of
tests/test_shading_kat.py.  Each frame must also equal the oracle's bit for bit, as in the other parity tests,
so a later divergence says which side moved.

derive_view (csrc/rtg_host.cpp) and launch_shade_t (csrc/rtg_device.hip) pick one of six k_shade instantiations
from a scene's content; every parameter id names in brackets the one its scenes reach, and the matrix reaches
all six.  The recursive cases go through k_resolve / k_resolve2; the slab at depth 6 has more than two levels."""
import numpy as np
import pytest

import pyoracle
import rtg
import shading_cases as S

pytestmark = pytest.mark.gpu

TLAS_ON = 2


def _check(sc, what, variant, **build):
    assert S.variant(sc) == variant, f"{what}: reaches {S.variant(sc)}"
    img, ref = S.reference(sc, pyoracle.rng_uniform)
    S.assert_lit(sc, img, pyoracle.rng_uniform, what)
    with rtg.Renderer(sc, device=0, **build) as r:
        got = r.render(0, seed=S.SEED)
        stats = r.build_stats()
    S.assert_close(got, img, what)
    o = pyoracle.Oracle(sc)
    want = o.render(0, seed=S.SEED)[0]
    o.close()
    assert np.array_equal(S.bits(got), S.bits(want)), f"{what}: GPU and oracle differ"
    return ref, stats


def _direct_groups():
    """One light type, with or without a BRDF, one exponent: 1 or 8 scenes a case."""
    heavy = {"spot", "environment"}
    for kind in S.LIGHTS:
        plain = {"point": "simple", "directional": "simple", "spot": "simple+spot", "area": "full",
                 "environment": "full+heavy"}[kind]
        brdf = "full+tex+heavy" if kind in heavy else "full+tex"
        for p in S.EXPONENTS:
            yield pytest.param(kind, ("none",), p, plain, id=f"{kind}-nobrdf-p{p}[{plain}]")
            yield pytest.param(kind, tuple(b for b in S.BRDFS if b != "none"), p, brdf, id=f"{kind}-brdfs-p{p}[{brdf}]")


@pytest.mark.parametrize("kind,brdfs,exponent,variant", list(_direct_groups()))
def test_direct(gpu, kind, brdfs, exponent, variant):
    for b in brdfs:
        _check(S.direct(kind, b, exponent), f"{kind}-{b}-p{exponent}", variant)


@pytest.mark.parametrize("variant", ["full+heavy"])
def test_area_and_spot_together(gpu, variant):
    """The heavy variant without an environment map."""
    _check(S.direct("area", "none", 8, extra=("spot",)), "area+spot", variant)


@pytest.mark.parametrize("variant", ["full+tex"])
def test_grazing_light_cut(gpu, variant):
    for b in ("op", "obp", "mp", "mbp"):
        _check(S.grazing(b), f"grazing-{b}", variant)


@pytest.mark.parametrize("variant", ["simple+spot"])
def test_spot_zones(gpu, variant):
    ref, _ = _check(S.direct("spot", "none", 8), "spot zones", variant)
    assert min(S.spot_zones(ref)) >= 2


@pytest.mark.parametrize("variant", ["simple"])
def test_shadow(gpu, variant):
    ref, _ = _check(S.shadow(), "shadow", variant)
    lit, dark, least = S.shadow_census(ref)
    assert lit >= 3 and dark >= 3 and least > 0.05, (lit, dark, least)


@pytest.mark.parametrize("variant", ["simple"])
@pytest.mark.parametrize("kind", ["mirror", "conductor"])
def test_reflector(gpu, kind, variant):
    """Depth 2, and depth 0, which must equal basic shading."""
    _check(S.reflector(kind, 2), f"{kind}-d2", variant)
    _check(S.reflector(kind, 0), f"{kind}-d0", variant)


@pytest.mark.parametrize("variant", ["simple"])
def test_mirror_through_the_top_level_bvh(gpu, variant):
    """The mirror case with the top-level BVH forced on (rtg_build_opts.tlas)."""
    _, stats = _check(S.reflector("mirror", 2), "mirror-d2 tlas", variant, tlas=TLAS_ON)
    assert stats["tlas_nodes"] > 0


@pytest.mark.parametrize("variant", ["simple"])
@pytest.mark.parametrize("absorption", [(0.0, 0.0, 0.0), (0.3, 0.6, 0.9)], ids=["clear", "absorbing"])
def test_glass_slab(gpu, absorption, variant):
    """Depths 1, 2, 4 and 6."""
    for depth in (1, 2, 4, 6):
        ref, _ = _check(S.slab(absorption, depth), f"slab-{absorption}-d{depth}", variant)
        S.assert_slab(ref, any(absorption))


@pytest.mark.parametrize("variant", ["full"])
def test_four_samples(gpu, variant):
    """The only case through sample accumulation."""
    _check(S.multisample(), "multisample", variant)
