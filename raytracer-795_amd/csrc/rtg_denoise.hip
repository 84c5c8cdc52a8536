// rtg_denoise.hip — an edge-avoiding à-trous wavelet filter for frames (rtg_denoise), guided
// by rtg_render_aov's first-hit depth, normal and albedo and by the frames' per-pixel variance (§14).
//
// Float32 throughout, + - * / sqrt min max abs only, every sum inside one lane in a fixed order, no atomics:
// under this library's build flags (no contraction, correctly rounded divide and sqrt) tests/denoise_ref.py
// decides identically, bit for bit.
//   k_dn_prepare   validity, albedo demodulation, depth slopes, two 16-byte records per pixel:
//                  G = (n.x, n.y, n.z, z) and S = (s.r, s.g, s.b, v); an invalid pixel holds z = 0
//   k_dn_atrous    one 5x5 B3-spline pass with tap stride d, S -> S'; one lane per pixel, 32x8 blocks.
//                  <d, 0>: a (32 + 4d) x (8 + 4d) tile of both records staged in LDS (d = 1, 2);
//                  <0, 0>: every tap two 16-byte global loads (any stride)
//   k_dn_finish    remodulation; invalid pixels copy their input through
//   k_frame_inputs a frame's sums, counts and M2 -> the resolved rgb and the variance of the mean (§21)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "rtg_internal.h"

namespace rtg {
namespace {

constexpr int kDnBx = 32, kDnBy = 8;
constexpr float kDnAlbedoMin = 1.0f / 256.0f;

__device__ __forceinline__ float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ bool dn_finite(float x) { return fabsf(x) <= 3.402823466e38f; }     // false for NaN
__device__ __forceinline__ float dn_amod(float a) { return a > kDnAlbedoMin ? a : kDnAlbedoMin; }  // NaN -> the floor

// Blocks are numbered row by row in grid.x alone (grid.y would cap the image height at 65535 blocks of 8 rows).
__device__ __forceinline__ void dn_block(int nx, int& bx, int& by) {
    const unsigned gx = (unsigned)(nx + kDnBx - 1) / kDnBx;
    by = (int)(blockIdx.x / gx);
    bx = (int)(blockIdx.x - (unsigned)by * gx);
}

__device__ __forceinline__ bool dn_valid(const float* __restrict__ rgb, const float* __restrict__ normal,
                                         const float* __restrict__ depth, size_t i) {
    const float z = depth[i];
    if (!(dn_finite(z) && z > 0.0f)) return false;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; c++) ok = ok && dn_finite(rgb[3 * i + c]) && dn_finite(normal[3 * i + c]);
    return ok;
}

// min(|z(+1) - z|, |z - z(-1)|) over the valid in-image neighbours (index step `step`), 0 without one
__device__ __forceinline__ float dn_slope(const float* __restrict__ rgb, const float* __restrict__ normal,
                                          const float* __restrict__ depth, size_t i, float z, bool has_lo, bool has_hi,
                                          size_t step) {
    const bool lo = has_lo && dn_valid(rgb, normal, depth, i - step);
    const bool hi = has_hi && dn_valid(rgb, normal, depth, i + step);
    const float a = hi ? fabsf(depth[i + step] - z) : 0.0f;
    const float b = lo ? fabsf(z - depth[i - step]) : 0.0f;
    return hi && lo ? fminf(a, b) : hi ? a : b;
}

__global__ void __launch_bounds__(kDnBx * kDnBy)
k_dn_prepare(const float* __restrict__ rgb, const float* __restrict__ normal, const float* __restrict__ depth,
             const float* __restrict__ albedo, const float* __restrict__ variance, int nx, int ny,
             float4* __restrict__ G, float4* __restrict__ S, float2* __restrict__ slope) {
    int bx, by;
    dn_block(nx, bx, by);
    const int x = bx * kDnBx + threadIdx.x, y = by * kDnBy + threadIdx.y;
    if (x >= nx || y >= ny) return;
    const size_t i = (size_t)y * nx + x;
    if (!dn_valid(rgb, normal, depth, i)) {
        G[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        S[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        slope[i] = make_float2(0.0f, 0.0f);
        return;
    }
    const float z = depth[i];
    float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
    float v = variance ? variance[i] : 0.0f;
    if (!(dn_finite(v) && v >= 0.0f)) v = 0.0f;
    if (albedo) {
        const float ar = dn_amod(albedo[3 * i]), ag = dn_amod(albedo[3 * i + 1]), ab = dn_amod(albedo[3 * i + 2]);
        r = r / ar;
        g = g / ag;
        b = b / ab;
        const float ya = dn_lum(ar, ag, ab);
        v = v / (ya * ya);
    }
    G[i] = make_float4(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], z);
    S[i] = make_float4(r, g, b, v);
    slope[i] = make_float2(dn_slope(rgb, normal, depth, i, z, x > 0, x + 1 < nx, 1),
                           dn_slope(rgb, normal, depth, i, z, y > 0, y + 1 < ny, (size_t)nx));
}

struct DnParams {
    int nx, ny, d;
    float sigma_l, sigma_z;
    int npow;       // the normal stop is squared this many times
};

// One tap's weight; hh = h[dy+2] * h[dx+2], ax / ay = (float)|d*dx|, (float)|d*dy|.
template <bool kVar>
__device__ __forceinline__ float dn_weight(const float4& gp, const float4& gq, const float4& sq, float yp, float hh,
                                           float ax, float ay, const float2& sl, float den_l, const DnParams& P) {
    const float dot = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
    float wn = dot > 0.0f ? dot : 0.0f;
    for (int k = 0; k < P.npow; k++) wn = wn * wn;
    const float den_z = P.sigma_z * (sl.x * ax + sl.y * ay) + 1e-3f * gp.w;
    float xx = fabsf(gq.w - gp.w) / den_z;
    if (kVar) xx = xx + fabsf(dn_lum(sq.x, sq.y, sq.z) - yp) / den_l;
    const float u = 1.0f + 0.25f * xx;
    const float u2 = u * u;
    const float w = (hh * wn) / (u2 * u2);
    return dn_finite(w) ? w : 0.0f;
}

__device__ __forceinline__ float dn_h(int k) { return k == 2 ? 0.375f : (k == 1 || k == 3) ? 0.25f : 0.0625f; }

// kD > 0: the LDS-tiled pass for tap stride kD; kD == 0: the direct pass for stride P.d.
template <int kD, bool kVar>
__global__ void __launch_bounds__(kDnBx * kDnBy)
k_dn_atrous(const float4* __restrict__ G, const float4* __restrict__ Sin, const float2* __restrict__ slope,
            float4* __restrict__ Sout, DnParams P) {
    constexpr int kHalo = kD > 0 ? 2 * kD : 1;
    constexpr int kTw = kD > 0 ? kDnBx + 2 * kHalo : 1, kTh = kD > 0 ? kDnBy + 2 * kHalo : 1;
    // 16-byte records, 32 lanes of a row side by side: every 16-lane group of a 16-byte LDS read and every
    // 8-lane group of a 16-byte LDS write covers each bank once whatever the row length, so rows carry no pad
    __shared__ float4 tg[kTh][kTw];
    __shared__ float4 ts[kTh][kTw];
    const int nx = P.nx, ny = P.ny;
    int bx, by;
    dn_block(nx, bx, by);
    const int x = bx * kDnBx + threadIdx.x, y = by * kDnBy + threadIdx.y;
    if (kD > 0) {
        const int x0 = bx * kDnBx - kHalo, y0 = by * kDnBy - kHalo;
        for (int t = threadIdx.y * kDnBx + threadIdx.x; t < kTw * kTh; t += kDnBx * kDnBy) {
            const int ty = t / kTw, tx = t - ty * kTw;
            const int qx = x0 + tx, qy = y0 + ty;
            float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f), s = g;      // beyond the image: z = 0, no surface
            if (qx >= 0 && qx < nx && qy >= 0 && qy < ny) {
                const size_t q = (size_t)qy * nx + qx;
                g = G[q];
                s = Sin[q];
            }
            tg[ty][tx] = g;
            ts[ty][tx] = s;
        }
        __syncthreads();
    }
    if (x >= nx || y >= ny) return;
    const size_t p = (size_t)y * nx + x;
    const int lx = threadIdx.x + kHalo, ly = threadIdx.y + kHalo;
    const float4 gp = kD > 0 ? tg[ly][lx] : G[p];
    if (!(gp.w > 0.0f)) return;
    const float4 sp = kD > 0 ? ts[ly][lx] : Sin[p];
    const float2 sl = slope[p];
    const int d = kD > 0 ? kD : P.d;

    float den_l = 0.0f, yp = 0.0f;
    if (kVar) {
        float sv = 0.0f, sw = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const float wt = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
                float zq, vq;
                if (kD > 0) {
                    zq = tg[ly + dy][lx + dx].w;
                    vq = ts[ly + dy][lx + dx].w;
                } else {
                    const int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= nx || qy < 0 || qy >= ny) continue;
                    const size_t q = (size_t)qy * nx + qx;
                    zq = G[q].w;
                    vq = Sin[q].w;
                }
                if (!(zq > 0.0f)) continue;
                sv += wt * vq;
                sw += wt;
            }
        }
        den_l = P.sigma_l * sqrtf(sv / sw) + 1e-3f;
        yp = dn_lum(sp.x, sp.y, sp.z);
    }

    float W = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, av = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            float4 gq, sq;
            float w;
            if (dx == 0 && dy == 0) {
                sq = sp;
                w = 0.375f * 0.375f;
            } else {
                if (kD > 0) {
                    gq = tg[ly + kD * dy][lx + kD * dx];
                    if (!(gq.w > 0.0f)) continue;
                    sq = ts[ly + kD * dy][lx + kD * dx];
                } else {
                    const int qx = x + d * dx, qy = y + d * dy;
                    if (qx < 0 || qx >= nx || qy < 0 || qy >= ny) continue;
                    const size_t q = (size_t)qy * nx + qx;
                    gq = G[q];
                    if (!(gq.w > 0.0f)) continue;
                    sq = Sin[q];
                }
                const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
                w = dn_weight<kVar>(gp, gq, sq, yp, dn_h(dy + 2) * dn_h(dx + 2), (float)(d * adx), (float)(d * ady), sl,
                                    den_l, P);
            }
            W += w;
            ar += w * sq.x;
            ag += w * sq.y;
            ab += w * sq.z;
            av += (w * w) * sq.w;
        }
    }
    Sout[p] = make_float4(ar / W, ag / W, ab / W, av / (W * W));
}

__global__ void __launch_bounds__(kDnBx * kDnBy)
k_dn_finish(const float* __restrict__ rgb, const float* __restrict__ albedo, const float4* __restrict__ G,
            const float4* __restrict__ S, int nx, int ny, float* __restrict__ out) {
    int bx, by;
    dn_block(nx, bx, by);
    const int x = bx * kDnBx + threadIdx.x, y = by * kDnBy + threadIdx.y;
    if (x >= nx || y >= ny) return;
    const size_t i = (size_t)y * nx + x;
    if (!(G[i].w > 0.0f)) {
#pragma unroll
        for (int c = 0; c < 3; c++) out[3 * i + c] = rgb[3 * i + c];
        return;
    }
    const float4 s = S[i];
    float r = s.x, g = s.y, b = s.z;
    if (albedo) {
        r = r * dn_amod(albedo[3 * i]);
        g = g * dn_amod(albedo[3 * i + 1]);
        b = b * dn_amod(albedo[3 * i + 2]);
    }
    out[3 * i] = r;
    out[3 * i + 1] = g;
    out[3 * i + 2] = b;
}

// rtg_frame_denoise's per-call inputs, one lane per pixel of a whole, uncompacted frame (its
// owned-row order is image order): rgb as k_finalize / k_finalize_counts resolve it -- the sum over the pixel's
// own count, divided only when that exceeds 1, 0 without samples -- and, with kVar, the variance of the mean
// luminance (M2 / (float)(n - 1)) / (float)n, +0 for n < 2.  The 12-byte sums travel as three dwords in one
// access (they are 4-byte aligned), mean / M2 as one 8-byte load.
struct DnRgb { float r, g, b; };
template <bool kAdapt, bool kVar>
__global__ void __launch_bounds__(256)
k_frame_inputs(const DnRgb* __restrict__ acc, const unsigned* __restrict__ cnt, const float2* __restrict__ mom, int npix,
               int done, DnRgb* __restrict__ rgb, float* __restrict__ variance) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    int n = done;
    if (kAdapt) {
        const unsigned c = cnt[i];
        if (c & kRetiredBit) n = (int)(c & ~kRetiredBit);
    }
    DnRgb s = acc[i];
    if (n < 1) s = DnRgb{0.0f, 0.0f, 0.0f};
    if (n > 1) {
        const float fn = (float)n;
        s.r = s.r / fn; s.g = s.g / fn; s.b = s.b / fn;
    }
    rgb[i] = s;
    if (kVar) variance[i] = n >= 2 ? (mom[i].y / (float)(n - 1)) / (float)n : 0.0f;
}

template <class T>
struct DnBuf {
    T* p = nullptr;
    ~DnBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, sizeof(T) * (n ? n : 1)); }
};

struct DnEvents {       // RTG_DENOISE_TIMING (dev knob): the per-kernel split on stderr
    static constexpr int kMax = 12;
    hipEvent_t e[kMax] = {};
    int n = 0;
    bool on = false;
    ~DnEvents() { for (int i = 0; i < kMax; i++) if (e[i]) (void)hipEventDestroy(e[i]); }
    void mark(hipStream_t st) {
        if (on && n < kMax && hipEventCreate(&e[n]) == hipSuccess) { (void)hipEventRecord(e[n], st); n++; }
    }
};

template <int kD>
void dn_launch(bool var, dim3 grid, dim3 block, hipStream_t st, const float4* G, const float4* Sin, const float2* slope,
               float4* Sout, const DnParams& P) {
    if (var) hipLaunchKernelGGL((k_dn_atrous<kD, true>), grid, block, 0, st, G, Sin, slope, Sout, P);
    else hipLaunchKernelGGL((k_dn_atrous<kD, false>), grid, block, 0, st, G, Sin, slope, Sout, P);
}

}  // namespace

// Strides up to this run the LDS-tiled pass (measured on the MI355X: DESIGN.md §18, profiles/denoise.json).
constexpr int kDnLdsMaxStride = 2;

// the 56 B per pixel of workspace, one block (a hipMalloc costs more than a pass): G, S, S', slopes
size_t denoise_workspace_bytes(int nx, int ny) {
    const size_t n = (size_t)nx * ny;
    return sizeof(float4) * (3 * n + (n + 1) / 2);
}

int denoise_device(const rtg_denoise_inputs& in, int nx, int ny, const rtg_denoise_opts& o, float* out, hipStream_t st,
                   std::string& err) {
    DnBuf<char> ws;
    const hipError_t e = ws.alloc(denoise_workspace_bytes(nx, ny));
    if (e != hipSuccess) {
        err = std::string("denoise hipMalloc: ") + hipGetErrorString(e);
        return -1;
    }
    return denoise_device_ws(in, nx, ny, o, out, ws.p, st, err);
}

int denoise_device_ws(const rtg_denoise_inputs& in, int nx, int ny, const rtg_denoise_opts& o, float* out, void* workspace,
                      hipStream_t st, std::string& err) {
    const size_t n = (size_t)nx * ny;
    hipError_t e;
    float4* const ws = static_cast<float4*>(workspace);
    float4 *G = ws, *a = ws + n, *b = ws + 2 * n;
    float2* slope = (float2*)(ws + 3 * n);
    int lds_max = kDnLdsMaxStride;
    if (const char* s = getenv("RTG_DENOISE_LDS")) lds_max = atoi(s);      // dev knob: 0 = every pass direct
    DnEvents ev;
    ev.on = getenv("RTG_DENOISE_TIMING") != nullptr;
    const dim3 block(kDnBx, kDnBy), grid((unsigned)((nx + kDnBx - 1) / kDnBx) * (unsigned)((ny + kDnBy - 1) / kDnBy));
    ev.mark(st);
    hipLaunchKernelGGL(k_dn_prepare, grid, block, 0, st, in.rgb, in.normal, in.depth, in.albedo, in.variance, nx, ny, G, a,
                       slope);
    ev.mark(st);
    DnParams P{nx, ny, 1, o.sigma_l, o.sigma_z, o.normal_power_log2};
    const bool var = in.variance != nullptr;
    for (int i = 0; i < o.iterations; i++) {
        P.d = 1 << i;
        if (P.d == 1 && lds_max >= 1) dn_launch<1>(var, grid, block, st, G, a, slope, b, P);
        else if (P.d == 2 && lds_max >= 2) dn_launch<2>(var, grid, block, st, G, a, slope, b, P);
        else dn_launch<0>(var, grid, block, st, G, a, slope, b, P);
        ev.mark(st);
        float4* t = a; a = b; b = t;
    }
    hipLaunchKernelGGL(k_dn_finish, grid, block, 0, st, in.rgb, in.albedo, G, a, nx, ny, out);
    ev.mark(st);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess) {
        err = std::string("denoise: ") + hipGetErrorString(e);
        return -1;
    }
    if (ev.on) {
        fprintf(stderr, "[rtg] denoise %dx%d kernels (prepare, passes, finish) ms:", nx, ny);
        for (int i = 1; i < ev.n; i++) {
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, ev.e[i - 1], ev.e[i]);
            fprintf(stderr, " %.4f", ms);
        }
        fprintf(stderr, "\n");
    }
    return 0;
}

void launch_frame_inputs(const float* acc, const unsigned* cnt, const float* mom, int npix, int done, float* rgb,
                         float* variance, hipStream_t st) {
    if (npix <= 0) return;
    const dim3 grid((unsigned)((npix + 255) / 256)), block(256);
    const DnRgb* a = reinterpret_cast<const DnRgb*>(acc);
    const float2* m = reinterpret_cast<const float2*>(mom);
    DnRgb* o = reinterpret_cast<DnRgb*>(rgb);
    DnEvents ev;
    ev.on = getenv("RTG_DENOISE_TIMING") != nullptr;
    ev.mark(st);
    if (cnt && variance) hipLaunchKernelGGL((k_frame_inputs<true, true>), grid, block, 0, st, a, cnt, m, npix, done, o, variance);
    else if (cnt) hipLaunchKernelGGL((k_frame_inputs<true, false>), grid, block, 0, st, a, cnt, m, npix, done, o, variance);
    else if (variance) hipLaunchKernelGGL((k_frame_inputs<false, true>), grid, block, 0, st, a, cnt, m, npix, done, o, variance);
    else hipLaunchKernelGGL((k_frame_inputs<false, false>), grid, block, 0, st, a, cnt, m, npix, done, o, variance);
    ev.mark(st);
    if (ev.on && ev.n == 2 && hipEventSynchronize(ev.e[1]) == hipSuccess) {     // (the dev knob alone waits here)
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, ev.e[0], ev.e[1]);
        fprintf(stderr, "[rtg] frame inputs %d pixels (adaptive %d, variance %d) ms: %.4f\n", npix, cnt != nullptr,
                variance != nullptr, ms);
    }
}

}  // namespace rtg
