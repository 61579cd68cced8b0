// film.hip -- per-pixel second moment, noise estimate and render-until-converged
// (no counterpart in the reference, which renders a fixed ITER samples).
//
// Every pixel receives one contribution c = sqrt(color) per iteration.  With
// moments on, every pipeline (a single one too) writes c to its contribution
// buffer and k_merge_m2 adds c to the image and c * c to the moment buffer in
// one pass, in iteration order: both sums are bit-reproducible and the same for
// every pipeline count.  The noise estimate reads the two sums.
//
// The estimate uses the raw-moment form var = Q/n - (S/n)^2 in float32, which
// cancels: the variance has a floor of about 1e-7 * mean^2.  It is an estimate
// to stop a render by, not a statistic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/pathtracer_amd.h"
#include "renderer.h"

namespace pt {

#define PT_HIP(call)                                   \
    do {                                               \
        hipError_t _e = (call);                        \
        if (_e != hipSuccess) return fail(_e, #call);  \
    } while (0)

constexpr int kTile = PT_NOISE_TILE;
constexpr int kTileWG = kTile * kTile;      // one lane per pixel of a tile: 4 waves
static_assert(kTileWG == 256, "k_noise_tiles reduces four waves");

// image += c, m2 += c * c for one iteration's contributions c, n = W*H*3 floats,
// one read of c.  Memory bound (2 streams read-modify-write, 1 read): VEC moves
// 16 bytes per lane and needs 16-byte aligned image and m2 (contrib is the
// renderer's own allocation); caller-bound buffers with less alignment take the
// scalar variant.  c * c is rounded before the add (-ffp-contract=off).
template <bool VEC>
__global__ __launch_bounds__(256) void k_merge_m2(float* __restrict__ image, float* __restrict__ m2,
                                                  const float* __restrict__ contrib, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const size_t n4 = n >> 2;
        if (i < n4) {
            const float4 c = reinterpret_cast<const float4*>(contrib)[i];
            float4 s = reinterpret_cast<float4*>(image)[i];
            float4 q = reinterpret_cast<float4*>(m2)[i];
            s.x += c.x; s.y += c.y; s.z += c.z; s.w += c.w;
            q.x += c.x * c.x; q.y += c.y * c.y; q.z += c.z * c.z; q.w += c.w * c.w;
            reinterpret_cast<float4*>(image)[i] = s;
            reinterpret_cast<float4*>(m2)[i] = q;
        }
        if (i < (n & 3)) {                  // the last n % 4 floats
            const size_t j = (n4 << 2) + i;
            const float c = contrib[j];
            image[j] += c;
            m2[j] += c * c;
        }
    } else if (i < n) {
        const float c = contrib[i];
        image[i] += c;
        m2[i] += c * c;
    }
}

// One pixel's relative error: the standard error of the mean of each channel,
// summed, over the summed channel means (float32, in exactly this order).
__device__ inline float pixel_err(const float* __restrict__ S, const float* __restrict__ Q, size_t px, float nf) {
    float e[3], m[3];
    for (int k = 0; k < 3; k++) {
        m[k] = S[3 * px + k] / nf;
        const float q = Q[3 * px + k] / nf;
        float v = q - m[k] * m[k];
        v = v > 0.0f ? v : 0.0f;
        e[k] = sqrtf(v / (nf - 1.0f));
    }
    return ((e[0] + e[1]) + e[2]) / (((m[0] + m[1]) + m[2]) + 0.01f);
}

// Sum over a wave, then over the workgroup's waves through LDS, in a fixed order
// (no atomics): the result is in thread 0 and repeats bit for bit.
template <int WAVES>
__device__ inline double block_sum(double v, double* s_part) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) s_part[wid] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < WAVES; w++) t += s_part[w];
    return t;
}

// One workgroup per 16 x 16 tile (edge tiles are partial), one lane per pixel.
__global__ __launch_bounds__(kTileWG) void k_noise_tiles(const float* __restrict__ S, const float* __restrict__ Q,
                                                         int W, int H, int tiles_x, float nf,
                                                         double* __restrict__ tile_sum, float* __restrict__ tile_err) {
    __shared__ double s_part[kTileWG / 64];
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int x = tx * kTile + (threadIdx.x % kTile), y = ty * kTile + (threadIdx.x / kTile);
    double err = 0.0;
    if (x < W && y < H) err = (double)pixel_err(S, Q, (size_t)y * W + x, nf);
    const double t = block_sum<kTileWG / 64>(err, s_part);
    if (threadIdx.x == 0) {
        const int rw = W - tx * kTile, rh = H - ty * kTile;
        const int pw = rw < kTile ? rw : kTile, ph = rh < kTile ? rh : kTile;
        tile_sum[blockIdx.x] = t;
        tile_err[blockIdx.x] = (float)(t / (double)(pw * ph));
    }
}

// One workgroup over the tile sums: out_mean = sum / (W*H), out_max = largest tile_err.
__global__ __launch_bounds__(256) void k_noise_final(const double* __restrict__ tile_sum, const float* __restrict__ tile_err,
                                                     int ntiles, double npix, double* __restrict__ out_mean,
                                                     float* __restrict__ out_max) {
    __shared__ double s_part[4];
    __shared__ float s_max[4];
    double s = 0.0;
    float mx = 0.0f;                        // tile errors are >= 0
    for (int i = threadIdx.x; i < ntiles; i += 256) {
        s += tile_sum[i];
        mx = fmaxf(mx, tile_err[i]);
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_down(mx, off, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    const double t = block_sum<4>(s, s_part);     // its barrier also publishes s_max
    if (threadIdx.x == 0) {
        *out_mean = t / npix;
        *out_max = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
int Renderer::enableMoments(float* device_m2) {
    if (allocated) { last_error = "enable_moments must precede allocateOnGPU"; return -1; }
    moments_on = true;
    ext_m2 = device_m2;
    return 0;
}

// allocateOnGPU: the moment buffer (unless the caller owns it) and the noise
// reduction's tile buffers.
int Renderer::allocMoments() {
    const size_t n3 = (size_t)cfg.width * cfg.height * 3;
    if (ext_m2) {
        m2 = ext_m2;
    } else {
        void* d = nullptr;
        PT_HIP(hipMalloc(&d, n3 * sizeof(float)));
        allocs.push_back(d);
        m2 = (float*)d;
    }
    const size_t nt = (size_t)noiseTilesX() * noiseTilesY();
    void* d = nullptr;
    PT_HIP(hipMalloc(&d, (nt + 1) * sizeof(double)));          // tile sums, then the mean
    allocs.push_back(d);
    noise_sum = (double*)d;
    PT_HIP(hipMalloc(&d, (nt + 1) * sizeof(float)));           // tile errors, then the largest
    allocs.push_back(d);
    noise_err = (float*)d;
    return 0;
}

// image += c, m2 += c * c on pipeline stream st (renderLoop, where k_merge runs
// when moments are off)
int Renderer::launchMergeM2(const KParams& k, hipStream_t st) {
    const size_t n3 = (size_t)cfg.width * cfg.height * 3;
    const bool vec = (((uintptr_t)k.image | (uintptr_t)m2) & 15) == 0;
    if (vec) {
        const size_t n4 = n3 >> 2;
        hipLaunchKernelGGL(k_merge_m2<true>, dim3((unsigned)std::max<size_t>(1, (n4 + 255) / 256)), dim3(256), 0, st,
                           k.image, m2, k.contrib, n3);
    } else {
        hipLaunchKernelGGL(k_merge_m2<false>, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, st,
                           k.image, m2, k.contrib, n3);
    }
    PT_HIP(hipGetLastError());
    return 0;
}

int Renderer::readMoments(float* host_m2) {
    if (!allocated) { last_error = "not allocated"; return -1; }
    if (!moments_on) { last_error = "moments not enabled"; return -1; }
    PT_HIP(hipMemcpyAsync(host_m2, m2, (size_t)cfg.width * cfg.height * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
    PT_HIP(hipStreamSynchronize(stream));
    return checkFaults();
}

int Renderer::noise(int samples, double* mean_err, float* max_tile_err, float* tile_err_host) {
    if (!allocated) { last_error = "not allocated"; return -1; }
    if (!moments_on) { last_error = "moments not enabled"; return -1; }
    if (samples <= 0) samples = samples_accumulated;
    if (samples < 2) { last_error = "need at least 2 samples"; return -1; }
    const int tx = noiseTilesX(), ty = noiseTilesY(), nt = tx * ty;
    hipLaunchKernelGGL(k_noise_tiles, dim3((unsigned)nt), dim3(kTileWG), 0, stream, kp.image, m2, cfg.width, cfg.height,
                       tx, (float)samples, noise_sum, noise_err);
    PT_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_noise_final, dim3(1), dim3(256), 0, stream, noise_sum, noise_err, nt,
                       (double)cfg.width * (double)cfg.height, noise_sum + nt, noise_err + nt);
    PT_HIP(hipGetLastError());
    double mean = 0.0;
    float mx = 0.0f;
    PT_HIP(hipMemcpyAsync(&mean, noise_sum + nt, sizeof mean, hipMemcpyDeviceToHost, stream));
    PT_HIP(hipMemcpyAsync(&mx, noise_err + nt, sizeof mx, hipMemcpyDeviceToHost, stream));
    if (tile_err_host)
        PT_HIP(hipMemcpyAsync(tile_err_host, noise_err, (size_t)nt * sizeof(float), hipMemcpyDeviceToHost, stream));
    PT_HIP(hipStreamSynchronize(stream));
    if (checkFaults() != 0) return -1;
    if (mean_err) *mean_err = mean;
    if (max_tile_err) *max_tile_err = mx;
    return 0;
}

// Chunks of check_every iterations; after each chunk that brings this call's
// count to max(min_iters, 2) or more, the estimate over every sample in the
// accumulator is compared with target.  1 converged, 0 max_iters reached.
int Renderer::renderUntil(int first_iter, int min_iters, int max_iters, int check_every, double target,
                          int* iters_done, double* mean_err) {
    if (!allocated) { last_error = "not allocated"; return -1; }
    if (!moments_on) { last_error = "moments not enabled"; return -1; }
    if (first_iter < 0 || max_iters < 1) { last_error = "bad iteration range"; return -1; }
    if (check_every <= 0) check_every = 32;
    const int min_check = std::max(min_iters, 2);
    int done = 0, converged = 0;
    double mean = -1.0;                      // no estimate yet
    bool fresh = false;                      // mean belongs to the current sample count
    while (done < max_iters && !converged) {
        const int n = std::min(check_every, max_iters - done);
        if (renderLoop(first_iter + done, n) != 0) return -1;
        done += n;
        fresh = false;
        if (done >= min_check) {
            if (noise(0, &mean, nullptr, nullptr) != 0) return -1;
            fresh = true;
            converged = mean <= target;
        }
    }
    if (!fresh) {                            // min_iters beyond max_iters: report the estimate all the same
        if (samples_accumulated >= 2) {
            if (noise(0, &mean, nullptr, nullptr) != 0) return -1;
        } else if (synchronize() != 0) {
            return -1;
        }
    }
    if (iters_done) *iters_done = done;
    if (mean_err) *mean_err = mean;
    return converged;
}

}  // namespace pt
