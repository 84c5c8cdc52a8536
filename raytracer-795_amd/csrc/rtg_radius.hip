// rtg_radius.hip — the bounding-sphere radius of a transformed mesh entry on the device.
//
// rtg_scene_update re-derives the top level of a built scene.  The only per-triangle work in that is the
// radius of an entry's bounding sphere (entry_bounding_sphere, rtg_host.cpp): the largest squared distance of
// any triangle corner, through the model matrix, from the sphere's centre.  A device scene does not keep the
// records of its large meshes on the host -- they are in d_tris -- so the maximum is taken here, with the
// host's own function (tri_radius2, rtg_internal.h): double arithmetic without contraction and a "NaN wins"
// maximum, which does not depend on the order of its operands, so the result is the host pass's bit for bit.
//
// Reduction: a grid-stride loop per thread, __shfl_down over the wave's 64 lanes, the block's four waves
// through LDS, one partial per block; a second one-block launch folds the partials (the launch boundary
// orders the two: no flag, no atomic).
#include <algorithm>

#include "rtg_internal.h"

namespace rtg {

namespace {

__device__ __forceinline__ double wave_fold(double v) {
    for (int off = 32; off > 0; off >>= 1) v = radius2_fold(v, __shfl_down(v, off, 64));
    return v;   // lane 0 holds the wave's maximum
}

// the block's maximum, valid in thread 0
__device__ __forceinline__ double block_fold(double v) {
    __shared__ double s_w[kRadiusBlock / 64];
    v = wave_fold(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kRadiusBlock / 64; w++) v = radius2_fold(v, s_w[w]);
    return v;
}

// part[block] = the largest tri_radius2 over the block's share of tris[0, n)
__global__ __launch_bounds__(kRadiusBlock) void k_entry_radius2(const TriGeom* __restrict__ tris, int n, RadiusXf X,
                                                               double* __restrict__ part) {
    double mx2 = 0.0;
    const long long stride = (long long)gridDim.x * kRadiusBlock;
    for (long long k = (long long)blockIdx.x * kRadiusBlock + threadIdx.x; k < n; k += stride)
        mx2 = tri_radius2(tris[k], X, mx2);
    mx2 = block_fold(mx2);
    if (threadIdx.x == 0) part[blockIdx.x] = mx2;
}

// out[0] = the fold of part[0, nblocks); one block
__global__ __launch_bounds__(kRadiusBlock) void k_radius2_final(const double* __restrict__ part, int nblocks,
                                                               double* __restrict__ out) {
    double mx2 = 0.0;
    for (int k = threadIdx.x; k < nblocks; k += kRadiusBlock) mx2 = radius2_fold(mx2, part[k]);
    mx2 = block_fold(mx2);
    if (threadIdx.x == 0) out[0] = mx2;
}

struct EventPair {
    hipEvent_t e[2] = {};
    ~EventPair() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

}  // namespace

int entry_radius2_device(const TriGeom* tris, int n, const RadiusXf& X, double* part, double* r2, float* ms,
                         std::string& err) {
    auto bad = [&](const char* what, hipError_t e) {
        err = std::string(what) + ": " + hipGetErrorString(e);
        return RTG_ERR_HIP;
    };
    if (!tris || !part || !r2 || n < 1) { err = "entry radius: bad arguments"; return RTG_ERR_INVALID; }
    const int nblocks = std::min((n + kRadiusBlock - 1) / kRadiusBlock, kRadiusMaxBlocks);
    EventPair ev;
    hipError_t e;
    if (ms) {
        for (hipEvent_t& x : ev.e)
            if ((e = hipEventCreate(&x)) != hipSuccess) return bad("hipEventCreate", e);
        if ((e = hipEventRecord(ev.e[0], nullptr)) != hipSuccess) return bad("hipEventRecord", e);
    }
    hipLaunchKernelGGL(k_entry_radius2, dim3(nblocks), dim3(kRadiusBlock), 0, nullptr, tris, n, X, part);
    hipLaunchKernelGGL(k_radius2_final, dim3(1), dim3(kRadiusBlock), 0, nullptr, part, nblocks, part + kRadiusMaxBlocks);
    if ((e = hipGetLastError()) != hipSuccess) return bad("entry radius launch", e);
    if (ms && (e = hipEventRecord(ev.e[1], nullptr)) != hipSuccess) return bad("hipEventRecord", e);
    if ((e = hipMemcpy(r2, part + kRadiusMaxBlocks, sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess)
        return bad("entry radius read-back", e);
    if (ms) {
        if ((e = hipEventSynchronize(ev.e[1])) != hipSuccess) return bad("hipEventSynchronize", e);
        if ((e = hipEventElapsedTime(ms, ev.e[0], ev.e[1])) != hipSuccess) return bad("hipEventElapsedTime", e);
    }
    return RTG_OK;
}

}  // namespace rtg
