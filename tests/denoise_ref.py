"""numpy float32 restatement of the edge-avoiding denoiser (rtg_denoise): the same operations
in the same order on whole arrays, so it decides bit for bit what the kernels decide.  (A helper of
tests/test_denoise_abi.py and tests/test_gpu_denoise.py, not a test.)"""
import numpy as np

F = np.float32
H = [F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625)]


def _lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def _shift(a, dy, dx):
    """out[y, x] = a[y + dy, x + dx] where that lies in the image, else 0 / False."""
    ny, nx = a.shape[:2]
    out = np.zeros_like(a)
    y0, y1, x0, x1 = max(0, -dy), min(ny, ny - dy), max(0, -dx), min(nx, nx - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def _slope(z, valid, dy, dx):
    hi, lo = _shift(valid, dy, dx), _shift(valid, -dy, -dx)
    a = np.abs(_shift(z, dy, dx) - z)
    b = np.abs(z - _shift(z, -dy, -dx))
    return np.where(hi & lo, np.minimum(a, b), np.where(hi, a, np.where(lo, b, F(0)))).astype(F)


def denoise_ref(rgb, normal, depth, albedo=None, variance=None, iterations=0, sigma_l=0.0, sigma_z=0.0,
                normal_power_log2=0):
    rgb = np.ascontiguousarray(rgb, F)
    normal = np.ascontiguousarray(normal, F)
    depth = np.ascontiguousarray(depth, F)
    iterations = iterations or 5
    sigma_l = F(sigma_l or 4.0)
    sigma_z = F(sigma_z or 1.0)
    npow = normal_power_log2 or 6
    with np.errstate(all="ignore"):
        valid = np.isfinite(depth) & (depth > 0) & np.isfinite(rgb).all(axis=2) & np.isfinite(normal).all(axis=2)
        v = np.zeros_like(depth) if variance is None else np.ascontiguousarray(variance, F)
        v = np.where(np.isfinite(v) & (v >= 0), v, F(0)).astype(F)
        am = None
        s = rgb
        if albedo is not None:
            albedo = np.ascontiguousarray(albedo, F)
            am = np.where(albedo > F(1.0 / 256.0), albedo, F(1.0 / 256.0)).astype(F)
            s = rgb / am
            ya = _lum(am)
            v = v / (ya * ya)
        s = np.where(valid[..., None], s, F(0)).astype(F)
        v = np.where(valid, v, F(0)).astype(F)
        z = np.where(valid, depth, F(0)).astype(F)
        n = np.where(valid[..., None], normal, F(0)).astype(F)
        gx = _slope(z, valid, 0, 1)
        gy = _slope(z, valid, 1, 0)

        for it in range(iterations):
            d = 1 << it
            den_l = yp = None
            if variance is not None:
                sv = np.zeros_like(v)
                sw = np.zeros_like(v)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        wt = F(0.5 if dy == 0 else 0.25) * F(0.5 if dx == 0 else 0.25)
                        m = _shift(valid, dy, dx)
                        sv = np.where(m, sv + wt * _shift(v, dy, dx), sv)
                        sw = np.where(m, sw + wt, sw)
                den_l = sigma_l * np.sqrt(sv / sw) + F(1e-3)
                yp = _lum(s)
            W = np.zeros_like(v)
            acc_s = np.zeros_like(s)
            acc_v = np.zeros_like(v)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if dx == 0 and dy == 0:
                        m, sq, vq = valid, s, v
                        w = np.full_like(v, H[2] * H[2])
                    else:
                        m = _shift(valid, d * dy, d * dx)
                        if not m.any():
                            continue
                        nq, zq = _shift(n, d * dy, d * dx), _shift(z, d * dy, d * dx)
                        sq, vq = _shift(s, d * dy, d * dx), _shift(v, d * dy, d * dx)
                        dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                        wn = np.where(dot > 0, dot, F(0)).astype(F)
                        for _ in range(npow):
                            wn = wn * wn
                        den_z = sigma_z * (gx * F(abs(d * dx)) + gy * F(abs(d * dy))) + F(1e-3) * z
                        x = np.abs(zq - z) / den_z
                        if variance is not None:
                            x = x + np.abs(_lum(sq) - yp) / den_l
                        u = F(1) + F(0.25) * x
                        u2 = u * u
                        w = ((H[dy + 2] * H[dx + 2]) * wn) / (u2 * u2)
                        w = np.where(np.isfinite(w), w, F(0)).astype(F)
                    W = np.where(m, W + w, W)
                    acc_s = np.where(m[..., None], acc_s + w[..., None] * sq, acc_s)
                    acc_v = np.where(m, acc_v + (w * w) * vq, acc_v)
            s = np.where(valid[..., None], acc_s / W[..., None], F(0)).astype(F)
            v = np.where(valid, acc_v / (W * W), F(0)).astype(F)
        out = s * am if am is not None else s
        out = np.where(valid[..., None], out, rgb).astype(F)
    assert out.dtype == F
    return out
