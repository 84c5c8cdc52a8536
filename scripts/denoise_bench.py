#!/usr/bin/env python3
"""Measurements of the edge-avoiding denoiser (results: profiles/denoise.json).

    python scripts/denoise_bench.py cost    OUT.json   # rtg_denoise_device at 1920x1080, per kernel, per variant
    python scripts/denoise_bench.py quality OUT.json   # cornell_pt at 1080p: noisy against denoised, and the times

cost: one process, the arms (every pass direct / stride 1 in LDS / strides 1 and 2 in LDS, chosen with the
RTG_DENOISE_LDS dev knob) alternating, one warm-up round then `--reps` timed; the total by events around the
call on the null stream, the per-kernel split from the library's own events (RTG_DENOISE_TIMING), the
per-call allocation as host wall time minus event time, and in the same rounds a device-to-device copy of
the bytes one pass must move."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer-795_amd"))

import rtg  # noqa: E402
from rtg import _abi as A  # noqa: E402
from rtg import scenegen  # noqa: E402


def stats(v):
    v = sorted(float(x) for x in v)
    return {"median": v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]), "min": v[0],
            "max": v[-1], "n": len(v)}


class Stderr:
    """The process's stderr (the library's fprintf included) into a file for the duration."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def cost(args):
    import torch

    lib = rtg.load_library()
    nx, ny, iters = 1920, 1080, 5
    n = nx * ny
    # guides of a real frame, tiled up from a small render would repeat; a path-traced Cornell box at 1080p, 16 spp
    sc = scenegen.cornell_pt(nx, ny, spp=16)
    with rtg.Renderer(sc, device=0) as r:
        with r.frame(0, moments=True) as f:
            f.add(16)
            img = f.resolve()
            var = (f.moments()[1] / np.float32(16)).astype(np.float32)
        g = r.aov(0)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
         for k, v in dict(rgb=img, normal=g["normal"], depth=g["depth"], albedo=g["albedo"], variance=var).items()}
    out = torch.empty((ny, nx, 3), dtype=torch.float32, device=dev)
    ptr = lambda k: C.cast(C.c_void_p(t[k].data_ptr()), A.PF)
    di = A.DenoiseInputs(ptr("rgb"), ptr("normal"), ptr("depth"), ptr("albedo"), ptr("variance"))
    do = A.DenoiseOpts(iters)
    # what one pass must move: 40 B read (G, S, the slopes) + 16 B written per pixel.  A copy of 28 B per pixel
    # reads and writes 56 B per pixel in all; a copy of 56 B per pixel is given beside it.
    src28, dst28 = (torch.empty(28 * n, dtype=torch.uint8, device=dev) for _ in range(2))
    src56, dst56 = (torch.empty(56 * n, dtype=torch.uint8, device=dev) for _ in range(2))
    src28.fill_(1)
    src56.fill_(1)
    arms = {"direct": "0", "lds_d1": "1", "lds_d1_d2": "2"}
    rows = {a: {"event_ms": [], "wall_ms": [], "kernels_ms": []} for a in arms}
    copies = {"copy_28B_per_pixel_ms": [], "copy_56B_per_pixel_ms": []}
    os.environ["RTG_DENOISE_TIMING"] = "1"
    ref_bits = None
    for rep in range(args.reps + 1):
        for arm, knob in arms.items():
            os.environ["RTG_DENOISE_LDS"] = knob
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            with Stderr() as err:
                w0 = time.perf_counter()
                e0.record()
                rc = lib.rtg_denoise_device(0, C.byref(di), nx, ny, C.byref(do), C.c_void_p(out.data_ptr()), None)
                e1.record()
                torch.cuda.synchronize()
                w1 = time.perf_counter()
            A.check(rc, lib)
            bits = out.cpu().numpy().view(np.int32)
            if ref_bits is None:
                ref_bits = bits
            assert np.array_equal(bits, ref_bits), "the variants disagree"
            if rep == 0:
                continue
            line = [ln for ln in err.text.splitlines() if "denoise" in ln and "ms:" in ln][-1]
            rows[arm]["kernels_ms"].append([float(x) for x in line.split("ms:")[1].split()])
            rows[arm]["event_ms"].append(e0.elapsed_time(e1))
            rows[arm]["wall_ms"].append((w1 - w0) * 1e3)
        for key, (s, d) in (("copy_28B_per_pixel_ms", (src28, dst28)), ("copy_56B_per_pixel_ms", (src56, dst56))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            d.copy_(s)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                copies[key].append(e0.elapsed_time(e1))
    res = {"image": [nx, ny], "iterations": iters, "reps": args.reps, "arms": {}, "copies": {k: stats(v) for k, v in copies.items()}}
    y28 = res["copies"]["copy_28B_per_pixel_ms"]["median"]
    for arm, r_ in rows.items():
        k = np.array(r_["kernels_ms"])          # prepare, pass 0..iters-1, finish
        names = ["prepare"] + [f"pass_d{1 << i}" for i in range(iters)] + ["finish"]
        res["arms"][arm] = {
            "event_ms": stats(r_["event_ms"]), "wall_ms": stats(r_["wall_ms"]),
            "alloc_and_launch_ms (wall - event)": stats(np.array(r_["wall_ms"]) - np.array(r_["event_ms"])),
            "kernels_ms": {nm: stats(k[:, i]) for i, nm in enumerate(names)},
            "pass_over_copy_28B": {nm: float(np.median(k[:, i]) / y28) for i, nm in enumerate(names) if nm.startswith("pass")},
        }
    return res


def quality(args):
    nx, ny = 1920, 1080
    res = {"image": [nx, ny], "scene": "scenegen.cornell_pt(1920, 1080, spp=N), one scene per sample count",
           "truth_spp": 1024, "rows": []}
    clamp = lambda a: np.clip(a.astype(np.float64), 0.0, 255.0)
    rms = lambda a, b: float(np.sqrt(np.mean((clamp(a) - clamp(b)) ** 2)))

    def where(a, b):
        """How concentrated the squared error is: the share of it in the worst 0.1 % and 1 % of the pixels, the
        rms without the worst 1 %, and the share in each cell of a 6 x 8 grid over the image (rows first)."""
        e2 = ((clamp(a) - clamp(b)) ** 2).sum(axis=2)
        srt = np.sort(e2.ravel())[::-1]
        k1, k01 = len(srt) // 100, len(srt) // 1000
        grid = e2.reshape(6, ny // 6, 8, nx // 8).sum(axis=(1, 3)) / e2.sum()
        return {"energy_share_worst_0.1_percent": float(srt[:k01].sum() / srt.sum()),
                "energy_share_worst_1_percent": float(srt[:k1].sum() / srt.sum()),
                "rms_without_worst_1_percent": float(np.sqrt(srt[k1:].sum() / (len(srt) - k1) / 3)),
                "energy_percent_grid_6x8": np.round(grid * 100, 1).tolist()}
    with rtg.Renderer(scenegen.cornell_pt(nx, ny, spp=1024), device=0) as r:
        with r.frame(0, sample_count=4, moments=True) as f:      # warm-up of the kernels and the allocator
            f.add(4)
        t0 = time.perf_counter()
        with r.frame(0) as f:
            f.add(1024)
            truth = f.resolve()
        res["truth_render_wall_ms"] = (time.perf_counter() - t0) * 1e3
    for spp in (16, 64, 256):
        row = {"spp": spp, "render_wall_ms": [], "denoise_wall_ms": [], "denoise_demodulate_off_wall_ms": []}
        with rtg.Renderer(scenegen.cornell_pt(nx, ny, spp=spp), device=0) as r:
            for rep in range(args.reps + 1):
                with r.frame(0, moments=True) as f:
                    t0 = time.perf_counter()
                    f.add(spp)
                    img = f.resolve()
                    t1 = time.perf_counter()
                    den = f.denoise()
                    t2 = time.perf_counter()
                    raw = f.denoise(demodulate=False)
                    t3 = time.perf_counter()
                    if rep == 0:                                  # the same filter without the luminance stop
                        g = r.aov(0)
                        novar = rtg.denoise(img, g["normal"], g["depth"], g["albedo"], None)
                if rep == 0:
                    continue                                      # one warm-up
                row["render_wall_ms"].append((t1 - t0) * 1e3)
                row["denoise_wall_ms"].append((t2 - t1) * 1e3)
                row["denoise_demodulate_off_wall_ms"].append((t3 - t2) * 1e3)
        for k in ("render_wall_ms", "denoise_wall_ms", "denoise_demodulate_off_wall_ms"):
            row[k] = stats(row[k])
        row["rms_clamped_noisy"] = rms(img, truth)
        row["rms_clamped_denoised"] = rms(den, truth)
        row["rms_clamped_denoised_demodulate_off"] = rms(raw, truth)
        row["rms_clamped_denoised_no_variance"] = rms(novar, truth)
        row["where_noisy"] = where(img, truth)
        row["where_denoised"] = where(den, truth)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["cost", "quality"])
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    res = cost(args) if args.what == "cost" else quality(args)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
