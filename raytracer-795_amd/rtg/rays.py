"""Primary-ray generators for Renderer.render_rays (rtg_render_rays).

Each returns (origins, directions, times): float32 arrays of shape (ny, nx, spp, 3), (ny, nx, spp, 3) and
(ny, nx, spp) -- sample s of pixel (x, y) at [y, x, s], row 0 at the top -- with unit directions and times 0.
Plain numpy: the closed forms are evaluated in float64 and rounded once to float32.

Sample positions inside a pixel: with spp == 1 the pixel centre, and nothing is drawn; otherwise sample s
lies in cell (s % g, s // g) of the g x g grid, g = ceil(sqrt(spp)), jittered inside the cell by
numpy.random.Generator(PCG64(seed)) -- one (ny, nx, spp, 2) draw, so a seed fixes every ray.
"""
from __future__ import annotations

import math

import numpy as np


def _unit(v, what: str) -> np.ndarray:
    v = np.asarray(v, np.float64).reshape(3)
    n = float(np.linalg.norm(v))
    if not np.isfinite(n) or n == 0.0:
        raise ValueError(f"{what} must be a finite non-zero vector")
    return v / n


def _film(nx: int, ny: int, spp: int, seed: int):
    """(u, v), each (ny, nx, spp) float64 in [0, 1): the samples' film coordinates, u to the right, v downwards."""
    nx, ny, spp = int(nx), int(ny), int(spp)
    if nx < 1 or ny < 1 or spp < 1:
        raise ValueError("nx, ny and spp must be at least 1")
    if spp == 1:
        fx = np.full((ny, nx, 1), 0.5)
        fy = fx
    else:
        g = math.isqrt(spp - 1) + 1                  # ceil(sqrt(spp))
        xi = np.random.Generator(np.random.PCG64(seed)).random((ny, nx, spp, 2))
        s = np.arange(spp)
        fx = ((s % g) + xi[..., 0]) / g
        fy = ((s // g) + xi[..., 1]) / g
    x = np.arange(nx, dtype=np.float64)[None, :, None]
    y = np.arange(ny, dtype=np.float64)[:, None, None]
    return (x + fx) / nx, (y + fy) / ny


def _frame(forward, up):
    """Orthonormal (forward, right, up): `forward` kept, `up` made perpendicular to it."""
    f = _unit(forward, "forward / gaze")
    r = np.cross(f, _unit(up, "up"))
    if float(np.linalg.norm(r)) < 1e-12:
        raise ValueError("up must not be parallel to forward / gaze")
    r = r / np.linalg.norm(r)
    return f, r, np.cross(r, f)


def equirect_rays(position, nx: int, ny: int, spp: int = 1, forward=(0, 0, -1), up=(0, 1, 0), seed: int = 0):
    """A latitude-longitude panorama from `position`: film u in [0, 1) is the azimuth (u - 1/2) * 2 pi about `up`,
    0 at `forward` and growing to the right; film v in [0, 1) is the polar angle v * pi from `up` (the top row
    tends to `up`, the bottom row to -up).  `forward` is made perpendicular to `up`."""
    u, v = _film(nx, ny, spp, seed)
    upn = _unit(up, "up")
    fw = _unit(forward, "forward")
    fw = fw - np.dot(fw, upn) * upn
    if float(np.linalg.norm(fw)) < 1e-12:
        raise ValueError("forward must not be parallel to up")
    f, r, _ = _frame(fw, upn)
    phi = (u - 0.5) * (2.0 * math.pi)
    theta = v * math.pi
    st = np.sin(theta)
    d = (st * np.cos(phi))[..., None] * f + (st * np.sin(phi))[..., None] * r + np.cos(theta)[..., None] * upn
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(np.asarray(position, np.float64).reshape(3), d.shape)
    return (np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), np.zeros(d.shape[:3], np.float32))


def ortho_rays(position, gaze, up, width: float, height: float, nx: int, ny: int, spp: int = 1, seed: int = 0):
    """An orthographic view: every ray runs along the normalised `gaze`; the origins cover the `width` x
    `height` rectangle centred on `position`, perpendicular to `gaze`, film u to the right and film v
    downwards (`up` made perpendicular to `gaze`)."""
    u, v = _film(nx, ny, spp, seed)
    f, r, u2 = _frame(gaze, up)
    o = (np.asarray(position, np.float64).reshape(3) + ((u - 0.5) * float(width))[..., None] * r
         + ((0.5 - v) * float(height))[..., None] * u2)
    d = np.broadcast_to(f, o.shape)
    return (np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), np.zeros(o.shape[:3], np.float32))
