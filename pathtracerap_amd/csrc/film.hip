// film.hip -- per-pixel second moment, noise estimate, render-until-converged, the
// variance-guided edge-avoiding denoiser, and the host side of tile-masked sampling
// with its per-tile estimate, mean and adaptive loop, and the merge and the denoiser prep
// of the sampled first-hit guides (no counterpart in the reference,
// which renders a fixed ITER samples and writes the raw mean); and the host side of
// environment lighting with its lookup test hook (pt_env.h), at the end.
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
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

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

// k_noise_tiles with a sample count per tile (adaptive sampling): nf = (float)counts[tile],
// the same pixel_err and the same fixed-order sum.  A tile with fewer than 2 samples has
// no estimate: error +inf, and 0 in the sum the frame mean is made of.
__global__ __launch_bounds__(kTileWG) void k_noise_tiles_counts(const float* __restrict__ S, const float* __restrict__ Q,
                                                                int W, int H, int tiles_x, const int* __restrict__ counts,
                                                                double* __restrict__ tile_sum, float* __restrict__ tile_err) {
    __shared__ double s_part[kTileWG / 64];
    const int cnt = counts[blockIdx.x];
    if (cnt < 2) {                          // the whole workgroup leaves, before the barrier
        if (threadIdx.x == 0) {
            tile_sum[blockIdx.x] = 0.0;
            tile_err[blockIdx.x] = INFINITY;
        }
        return;
    }
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int x = tx * kTile + (threadIdx.x % kTile), y = ty * kTile + (threadIdx.x / kTile);
    double err = 0.0;
    if (x < W && y < H) err = (double)pixel_err(S, Q, (size_t)y * W + x, (float)cnt);
    const double t = block_sum<kTileWG / 64>(err, s_part);
    if (threadIdx.x == 0) {
        const int rw = W - tx * kTile, rh = H - ty * kTile;
        const int pw = rw < kTile ? rw : kTile, ph = rh < kTile ? rh : kTile;
        tile_sum[blockIdx.x] = t;
        tile_err[blockIdx.x] = (float)(t / (double)(pw * ph));
    }
}

// Float i of the W*H*3 sums over its tile's sample count (0 where the tile has none).
__device__ inline float mean_by_count(float s, size_t i, int W, int tiles_x, const int* __restrict__ counts) {
    const size_t px = i / 3;
    const int y = (int)(px / (size_t)W), x = (int)(px - (size_t)y * W);
    const int c = counts[(y / kTile) * tiles_x + (x / kTile)];
    return c > 0 ? s / (float)c : 0.0f;
}

// out = S / (float)counts[tile], n = W*H*3 floats.  Memory bound (one stream read, one
// written): VEC moves 16 bytes per lane and needs 16-byte aligned S and out; buffers
// with less alignment take the scalar variant, as in k_merge_m2.
template <bool VEC>
__global__ __launch_bounds__(256) void k_mean_counts(const float* __restrict__ S, float* __restrict__ out, size_t n, int W,
                                                     int tiles_x, const int* __restrict__ counts) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const size_t n4 = n >> 2;
        if (i < n4) {
            const float4 s = reinterpret_cast<const float4*>(S)[i];
            float4 m;
            m.x = mean_by_count(s.x, 4 * i, W, tiles_x, counts);
            m.y = mean_by_count(s.y, 4 * i + 1, W, tiles_x, counts);
            m.z = mean_by_count(s.z, 4 * i + 2, W, tiles_x, counts);
            m.w = mean_by_count(s.w, 4 * i + 3, W, tiles_x, counts);
            reinterpret_cast<float4*>(out)[i] = m;
        }
        if (i < (n & 3)) {                  // the last n % 4 floats
            const size_t j = (n4 << 2) + i;
            out[j] = mean_by_count(S[j], j, W, tiles_x, counts);
        }
    } else if (i < n) {
        out[i] = mean_by_count(S[i], i, W, tiles_x, counts);
    }
}

// ---------------------------------------------------------------------------
// Denoiser: an a-trous filter in the style of SVGF's spatial pass, guided by the
// per-pixel variance of the mean (from S and Q) and by the primary-hit cache
// (depth, world normal, model).  include/pathtracer_amd.h (pt_renderer_denoise)
// states the arithmetic; the kernels keep its float32 operations and their order
// (IEEE add, multiply, divide, square root; -ffp-contract=off), so the result
// equals the numpy restatement in tests/denoise_ref.py bit for bit.  pt_renderer_denoise_ex adds
// two options to prep, and a remodulation after the last pass (tests/denoise_albedo_ref.py).
//
// Per-pixel records, built once per call by k_denoise_prep: (c.rgb, V) ping-pong,
// (n.xyz, d), the model and the depth slope.  No atomics: a call repeats bit for bit.
// ---------------------------------------------------------------------------
__device__ inline float dn_h5(int i) { return i == 2 ? 0.375f : ((i == 1) | (i == 3)) ? 0.25f : 0.0625f; }
__device__ inline float dn_g3(int i) { return i == 1 ? 0.5f : 0.25f; }
__device__ inline int dn_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// depth of frame pixel idx in the primary-hit cache; pixels tail_drop left out count as misses
__device__ inline float dn_depth(const float4* __restrict__ cache_hit, int npix, size_t idx) {
    return idx < (size_t)npix ? cache_hit[idx].x : FLT_MAX;
}

// pt_renderer_denoise_ex, PT_DENOISE_DEMODULATE: per channel the sqrt-space albedo sa of pixel
// p's primary hit on model k, and the divisor e = max(sa, 1e-3f).  A is what
// pt_renderer_primary_albedo reports: the albedo plane's texel when the allocation has textures
// (`plane`), else the model's colour.  Both are kernel arguments, so the choice is wave-uniform.
// k < 0 (a miss, or a pixel tail_drop left out; the plane ends at the traced count): sa = e = 1.
__device__ inline void dn_sqrt_albedo(int k, size_t p, const float4* __restrict__ plane,
                                      const ModelShade* __restrict__ shade, float* sa, float* e) {
    if (k < 0) {
        for (int c = 0; c < 3; c++) sa[c] = e[c] = 1.0f;
        return;
    }
    float a[3];
    if (plane) {
        const float4 t = plane[p];
        a[0] = t.x; a[1] = t.y; a[2] = t.z;
    } else {
        for (int c = 0; c < 3; c++) a[c] = shade[k].color[c];
    }
    for (int c = 0; c < 3; c++) {
        const float t = a[c] > 0.0f ? a[c] : 0.0f;      // a NaN gives 0
        sa[c] = sqrtf(t);
        e[c] = sa[c] > 1e-3f ? sa[c] : 1e-3f;
    }
}

// What the variants of k_denoise_prep read beyond the plain one's arguments.
struct DnPrepOpt {
    const float4* albedo;       // DEMOD: the albedo plane (KParams::cache_albedo), or null:
    const ModelShade* shade;    // ... the models' colours
    const int* counts;          // COUNTS: samples per 16 x 16 tile
    int tiles_x;
};

// One pixel's records from its sums s, q (3 floats each).  DEMOD: c and the channel variances
// divided by the primary hit's sqrt-space albedo.  COUNTS: nf is the pixel's tile's own count.
template <bool DEMOD, bool COUNTS>
__device__ inline void dn_prep_pixel(size_t p, const float* s, const float* q, float nf, const DnPrepOpt& opt,
                                     const float4* __restrict__ cache_hit, const int* __restrict__ cache_model, int npix,
                                     int W, int H, float4* __restrict__ cv, float4* __restrict__ nd,
                                     int* __restrict__ model, float* __restrict__ slope) {
    if (COUNTS) {
        const int ty = (int)(p / (size_t)W), tx = (int)(p - (size_t)ty * W);
        nf = (float)opt.counts[(ty / kTile) * opt.tiles_x + (tx / kTile)];
    }
    float m[3], v[3];
    for (int k = 0; k < 3; k++) {
        m[k] = s[k] / nf;
        const float qq = q[k] / nf;
        float t = qq - m[k] * m[k];
        t = t > 0.0f ? t : 0.0f;
        v[k] = t / (nf - 1.0f);
    }
    if (DEMOD) {
        float sa[3], e[3];
        dn_sqrt_albedo(p < (size_t)npix ? cache_model[p] : -1, p, opt.albedo, opt.shade, sa, e);
        for (int k = 0; k < 3; k++) {
            m[k] = m[k] / e[k];
            v[k] = v[k] / (e[k] * e[k]);
        }
    }
    cv[p] = make_float4(m[0], m[1], m[2], (v[0] + v[1]) + v[2]);
    const bool live = p < (size_t)npix;
    const float4 h = live ? cache_hit[p] : make_float4(FLT_MAX, 0.0f, 0.0f, 0.0f);
    nd[p] = make_float4(h.y, h.z, h.w, h.x);
    model[p] = live ? cache_model[p] : -1;
    const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
    const int xm = dn_clamp(x - 1, W - 1), xp = dn_clamp(x + 1, W - 1);
    const int ym = dn_clamp(y - 1, H - 1), yp = dn_clamp(y + 1, H - 1);
    const float gx = fabsf(dn_depth(cache_hit, npix, (size_t)y * W + xp) - dn_depth(cache_hit, npix, (size_t)y * W + xm)) * 0.5f;
    const float gy = fabsf(dn_depth(cache_hit, npix, (size_t)yp * W + x) - dn_depth(cache_hit, npix, (size_t)ym * W + x)) * 0.5f;
    slope[p] = gx > gy ? gx : gy;
}

// VEC: a lane takes 4 pixels = 3 float4 of S and of Q (16-byte aligned S and Q; the last
// npixels % 4 pixels go one per lane); otherwise one pixel per lane, scalar reads.
// DEMOD, COUNTS: pt_renderer_denoise_ex's options; <VEC, false, false> is pt_renderer_denoise's
// prep and reads nothing of `opt`.  DEMOD adds one float4 of the albedo plane per pixel (a lane's
// 4 pixels are 64 consecutive bytes) or, without textures, a gather of the model's colour; COUNTS
// one int per pixel, the same for 16 consecutive pixels of a row.
template <bool VEC, bool DEMOD, bool COUNTS>
__global__ __launch_bounds__(256) void k_denoise_prep(const float* __restrict__ S, const float* __restrict__ Q, float nf,
                                                      const float4* __restrict__ cache_hit,
                                                      const int* __restrict__ cache_model, int npix, int W, int H,
                                                      float4* __restrict__ cv, float4* __restrict__ nd,
                                                      int* __restrict__ model, float* __restrict__ slope, DnPrepOpt opt) {
    const size_t n = (size_t)W * H;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const size_t n4 = n >> 2;
        if (i < n4) {
            float s[12], q[12];
            for (int k = 0; k < 3; k++) {
                const float4 a = reinterpret_cast<const float4*>(S)[3 * i + k];
                const float4 b = reinterpret_cast<const float4*>(Q)[3 * i + k];
                s[4 * k] = a.x; s[4 * k + 1] = a.y; s[4 * k + 2] = a.z; s[4 * k + 3] = a.w;
                q[4 * k] = b.x; q[4 * k + 1] = b.y; q[4 * k + 2] = b.z; q[4 * k + 3] = b.w;
            }
            for (int k = 0; k < 4; k++)
                dn_prep_pixel<DEMOD, COUNTS>(4 * i + k, s + 3 * k, q + 3 * k, nf, opt, cache_hit, cache_model, npix, W, H,
                                             cv, nd, model, slope);
        }
        if (i < (n & 3)) {
            const size_t p = (n4 << 2) + i;
            const float s[3] = {S[3 * p], S[3 * p + 1], S[3 * p + 2]};
            const float q[3] = {Q[3 * p], Q[3 * p + 1], Q[3 * p + 2]};
            dn_prep_pixel<DEMOD, COUNTS>(p, s, q, nf, opt, cache_hit, cache_model, npix, W, H, cv, nd, model, slope);
        }
    } else if (i < n) {
        const float s[3] = {S[3 * i], S[3 * i + 1], S[3 * i + 2]};
        const float q[3] = {Q[3 * i], Q[3 * i + 1], Q[3 * i + 2]};
        dn_prep_pixel<DEMOD, COUNTS>(i, s, q, nf, opt, cache_hit, cache_model, npix, W, H, cv, nd, model, slope);
    }
}

// The staged image of a pass: the 16 x 16 tile and its 2 * STEP halo.  Rows of the
// float4 planes are padded to a multiple of 16 records (256 B = every bank once): a
// ds_read_b128 lane group spans two tile rows, whose 16 x positions then fall on 16
// different 16-byte bank groups.  The model plane (ds_read_b32, 32 banks, a lane group
// = two tile rows) has rows of 48 words, so the second row lands 16 banks on.
template <int STEP>
struct DnTile {
    static constexpr int kHalo = 2 * STEP;
    static constexpr int kEdge = kTile + 2 * kHalo;             // 20, 24, 32, 48
    static constexpr int kRow = (kEdge + 15) / 16 * 16;         // 32, 32, 32, 48
    static constexpr int kRowM = 48;
    static_assert(kEdge <= kRowM, "the staged variant stops at step 8");
};

// One a-trous pass with taps STEP apart: reads (c, V) of the previous pass, writes the
// next.  One workgroup per 16 x 16 tile (edge tiles partial), one lane per pixel.
// STAGE: the tile's records and their halo go through LDS (positions outside the frame
// carry model -2, which equals no pixel's model); otherwise the 25 taps are read from
// global memory.  Both variants evaluate the same expressions in the same order.
template <int STEP, bool STAGE>
__global__ __launch_bounds__(kTileWG) void k_denoise_pass(const float4* __restrict__ cv_in, float4* __restrict__ cv_out,
                                                          const float4* __restrict__ nd, const int* __restrict__ model,
                                                          const float* __restrict__ slope, int W, int H, int tiles_x,
                                                          float sigma_l, float sigma_z) {
    using T = DnTile<STAGE ? STEP : 1>;
    __shared__ float4 s_cv[STAGE ? T::kEdge * T::kRow : 1];
    __shared__ float4 s_nd[STAGE ? T::kEdge * T::kRow : 1];
    __shared__ int s_k[STAGE ? T::kEdge * T::kRowM : 1];
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int x = tx * kTile + (threadIdx.x % kTile), y = ty * kTile + (threadIdx.x / kTile);
    const int x0 = tx * kTile - T::kHalo, y0 = ty * kTile - T::kHalo;    // frame position of the staged image's corner
    if (STAGE) {
        for (int idx = threadIdx.x; idx < T::kEdge * T::kEdge; idx += kTileWG) {
            const int sy = idx / T::kEdge, sx = idx - sy * T::kEdge;
            const int gx = x0 + sx, gy = y0 + sy;
            int k = -2;
            if ((gx >= 0) & (gx < W) & (gy >= 0) & (gy < H)) {
                const size_t g = (size_t)gy * W + gx;
                k = model[g];
                s_cv[sy * T::kRow + sx] = cv_in[g];
                s_nd[sy * T::kRow + sx] = nd[g];
            }
            s_k[sy * T::kRowM + sx] = k;
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    // records of frame position (qx, qy): inside the staged image for every tap and every
    // clamped 3 x 3 neighbour of a tile pixel
    auto rec_cv = [&](int qx, int qy) { return STAGE ? s_cv[(qy - y0) * T::kRow + (qx - x0)] : cv_in[(size_t)qy * W + qx]; };
    auto rec_nd = [&](int qx, int qy) { return STAGE ? s_nd[(qy - y0) * T::kRow + (qx - x0)] : nd[(size_t)qy * W + qx]; };
    const int kp = STAGE ? s_k[(y - y0) * T::kRowM + (x - x0)] : model[p];
    const float4 cp = rec_cv(x, y);
    if (kp < 0) {                            // miss or dropped: passes through, contributes nowhere
        cv_out[p] = cp;
        return;
    }
    float vbar = 0.0f;
#pragma unroll
    for (int j = -1; j <= 1; j++)
#pragma unroll
        for (int i = -1; i <= 1; i++)
            vbar += (dn_g3(j + 1) * dn_g3(i + 1)) * rec_cv(dn_clamp(x + i, W - 1), dn_clamp(y + j, H - 1)).w;
    const float4 np4 = rec_nd(x, y);
    const float dp = np4.w, gp = slope[p];
    const float lp = (cp.x + cp.y) + cp.z;
    const float den_l = sigma_l * sqrtf(vbar) + 1e-4f;
    float sw = 0.0f, sc0 = 0.0f, sc1 = 0.0f, sc2 = 0.0f, sv = 0.0f;
#pragma unroll
    for (int j = -2; j <= 2; j++) {
#pragma unroll
        for (int i = -2; i <= 2; i++) {
            const int qx = x + i * STEP, qy = y + j * STEP;
            int kq;
            if (STAGE) {
                kq = s_k[(qy - y0) * T::kRowM + (qx - x0)];
            } else {
                if ((qx < 0) | (qx >= W) | (qy < 0) | (qy >= H)) continue;
                kq = model[(size_t)qy * W + qx];
            }
            if (kq != kp) continue;
            const float4 cq = rec_cv(qx, qy);
            float w;
            if (i == 0 && j == 0) {
                w = dn_h5(2) * dn_h5(2);
            } else {
                const float4 nq = rec_nd(qx, qy);
                const float dot = (np4.x * nq.x + np4.y * nq.y) + np4.z * nq.z;
                float wn = dot > 0.0f ? dot : 0.0f;
                wn = wn * wn; wn = wn * wn; wn = wn * wn; wn = wn * wn; wn = wn * wn; wn = wn * wn;
                const float r = (float)(STEP * ((i < 0 ? -i : i) + (j < 0 ? -j : j)));
                const float a = (nq.w - dp) / (sigma_z * (gp * r + 1e-3f * dp));
                const float wz = 1.0f / (1.0f + a * a);
                const float xl = (((cq.x + cq.y) + cq.z) - lp) / den_l;
                const float wl = 1.0f / (1.0f + xl * xl);
                w = (dn_h5(j + 2) * dn_h5(i + 2)) * ((wn * wz) * wl);
            }
            sw += w;
            sc0 += w * cq.x;
            sc1 += w * cq.y;
            sc2 += w * cq.z;
            sv += (w * w) * cq.w;
        }
    }
    cv_out[p] = make_float4(sc0 / sw, sc1 / sw, sc2 / sw, sv / (sw * sw));
}

// The packed result as W*H*3 floats in the caller's (or another) device buffer.
__global__ __launch_bounds__(256) void k_denoise_out(const float4* __restrict__ cv, size_t n, float* __restrict__ rgb) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float4 c = cv[i];
        rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
    }
}

// PT_DENOISE_DEMODULATE, after the last pass: D = c * sa in place, one lane per pixel; V stays
// (demodulated units).  sa is recomputed from prep's source (sqrtf is correctly rounded, so it is
// prep's value) and the model prep recorded; a pixel with k < 0 has sa = 1 and keeps its bits.
__global__ __launch_bounds__(256) void k_denoise_remod(float4* __restrict__ cv, const int* __restrict__ model, size_t n,
                                                       const float4* __restrict__ albedo,
                                                       const ModelShade* __restrict__ shade) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float sa[3], e[3];
    dn_sqrt_albedo(model[i], i, albedo, shade, sa, e);
    float4 c = cv[i];
    c.x = c.x * sa[0]; c.y = c.y * sa[1]; c.z = c.z * sa[2];
    cv[i] = c;
}

// ---------------------------------------------------------------------------
// Sampled first-hit guides (pt_renderer_enable_guides, PT_DENOISE_SAMPLED_GUIDES): G holds per
// pixel the sums (Nx, Ny, Nz, Z, Ar, Ag, Ab, Hc) of the records k_guide_first (renderer.hip)
// wrote for the generated iterations; the guided prep reads their means where the plain one
// reads the primary-hit cache.  tests/guides_ref.py restates both bit for bit.
// ---------------------------------------------------------------------------

// Whether pixel px lies in a tile the mask keeps (null: every tile).
__device__ inline bool dn_tile_on(const unsigned char* __restrict__ tile_mask, int tiles_x, int W, size_t px) {
    if (!tile_mask) return true;
    const int y = (int)(px / (size_t)W), x = (int)(px - (size_t)y * W);
    return tile_mask[(y / kTile) * tiles_x + (x / kTile)] != 0;
}

// G += one generated iteration's records, n = W*H pixels of 8 floats, one add per float.
// Memory bound (one stream read-modify-write, one read): VEC moves 16 bytes per lane, two
// lanes per pixel, and needs a 16-byte aligned G (rec is the renderer's own allocation); a
// caller-bound G with less alignment takes the scalar variant, as in k_merge_m2.  Under a tile
// mask (a kernel argument: wave-uniform) only the pixels of active tiles are added: the
// pipeline's buffer still holds an earlier iteration's records for the others.
template <bool VEC>
__global__ __launch_bounds__(256) void k_merge_guides(float* __restrict__ G, const float* __restrict__ rec, size_t n,
                                                      const unsigned char* __restrict__ tile_mask, int tiles_x, int W) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        if (i >= 2 * n || !dn_tile_on(tile_mask, tiles_x, W, i >> 1)) return;
        const float4 c = reinterpret_cast<const float4*>(rec)[i];
        float4 g = reinterpret_cast<float4*>(G)[i];
        g.x += c.x; g.y += c.y; g.z += c.z; g.w += c.w;
        reinterpret_cast<float4*>(G)[i] = g;
    } else {
        if (i >= 8 * n || !dn_tile_on(tile_mask, tiles_x, W, i >> 3)) return;
        G[i] += rec[i];
    }
}

// Pixel p's record of G.  vec (a kernel argument: wave-uniform): G is 16-byte aligned, two
// 16-byte loads; else eight 4-byte loads (a caller-bound G).
__device__ inline void dn_guide_load(const float* __restrict__ G, size_t p, bool vec, float* g) {
    if (vec) {
        const float4 a = reinterpret_cast<const float4*>(G)[2 * p], b = reinterpret_cast<const float4*>(G)[2 * p + 1];
        g[0] = a.x; g[1] = a.y; g[2] = a.z; g[3] = a.w; g[4] = b.x; g[5] = b.y; g[6] = b.z; g[7] = b.w;
    } else {
        for (int k = 0; k < 8; k++) g[k] = G[8 * p + k];
    }
}

// Depth of frame pixel (x, y) from the sums: Z / Hc, FLT_MAX where no sample hit.
__device__ inline float dn_guide_depth(const float* __restrict__ G, int W, int x, int y) {
    const float* g = G + 8 * ((size_t)y * W + x);
    const float h = g[7];
    return h > 0.0f ? g[3] / h : FLT_MAX;
}

// The sampled sqrt-space albedo of a pixel with sums a (Ar, Ag, Ab) and Hc = h over nf samples:
// a sample that missed counts as albedo 1.  The sum is rounded before the division.
__device__ inline void dn_guide_albedo(const float* a, float h, float nf, float* sa, float* e) {
    for (int c = 0; c < 3; c++) {
        sa[c] = (a[c] + (nf - h)) / nf;
        e[c] = sa[c] > 1e-3f ? sa[c] : 1e-3f;
    }
}

// pt_renderer_denoise_ex with PT_DENOISE_SAMPLED_GUIDES: k_denoise_prep's records from G in place
// of the primary-hit cache.  One pixel per lane: 24 bytes of S and Q, the pixel's 32-byte record
// and (Z, Hc) of its four neighbours.  model = 0 where a sample hit, -1 elsewhere, so the passes'
// model test is "both pixels saw a surface"; the normal is the mean one, not renormalised.
template <bool DEMOD, bool COUNTS>
__global__ __launch_bounds__(256) void k_denoise_prep_guided(const float* __restrict__ S, const float* __restrict__ Q,
                                                             float nf, const float* __restrict__ G, int W, int H,
                                                             float4* __restrict__ cv, float4* __restrict__ nd,
                                                             int* __restrict__ model, float* __restrict__ slope,
                                                             const int* __restrict__ counts, int tiles_x, bool vec) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)W * H) return;
    const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
    if (COUNTS) nf = (float)counts[(y / kTile) * tiles_x + (x / kTile)];
    float g[8];
    dn_guide_load(G, p, vec, g);
    const float h = g[7];
    float m[3], v[3];
    for (int k = 0; k < 3; k++) {
        m[k] = S[3 * p + k] / nf;
        const float qq = Q[3 * p + k] / nf;
        float t = qq - m[k] * m[k];
        t = t > 0.0f ? t : 0.0f;
        v[k] = t / (nf - 1.0f);
    }
    if (DEMOD) {
        float sa[3], e[3];
        dn_guide_albedo(g + 4, h, nf, sa, e);
        for (int k = 0; k < 3; k++) {
            m[k] = m[k] / e[k];
            v[k] = v[k] / (e[k] * e[k]);
        }
    }
    cv[p] = make_float4(m[0], m[1], m[2], (v[0] + v[1]) + v[2]);
    const bool hit = h > 0.0f;
    nd[p] = hit ? make_float4(g[0] / h, g[1] / h, g[2] / h, g[3] / h) : make_float4(0.0f, 0.0f, 0.0f, FLT_MAX);
    model[p] = hit ? 0 : -1;
    const int xm = dn_clamp(x - 1, W - 1), xp = dn_clamp(x + 1, W - 1);
    const int ym = dn_clamp(y - 1, H - 1), yp = dn_clamp(y + 1, H - 1);
    const float gx = fabsf(dn_guide_depth(G, W, xp, y) - dn_guide_depth(G, W, xm, y)) * 0.5f;
    const float gy = fabsf(dn_guide_depth(G, W, x, yp) - dn_guide_depth(G, W, x, ym)) * 0.5f;
    slope[p] = gx > gy ? gx : gy;
}

// k_denoise_remod for the guided prep: D = c * sa with prep's sampled sa, recomputed from G and
// the same nf by the same expression (so it is prep's value), also for a pixel no sample hit
// (sa = 1: it keeps its bits).
template <bool COUNTS>
__global__ __launch_bounds__(256) void k_denoise_remod_guided(float4* __restrict__ cv, const float* __restrict__ G,
                                                              size_t n, float nf, int W, const int* __restrict__ counts,
                                                              int tiles_x, bool vec) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (COUNTS) {
        const int y = (int)(i / (size_t)W), x = (int)(i - (size_t)y * W);
        nf = (float)counts[(y / kTile) * tiles_x + (x / kTile)];
    }
    float g[8];
    dn_guide_load(G, i, vec, g);
    float sa[3], e[3];
    dn_guide_albedo(g + 4, g[7], nf, sa, e);
    float4 c = cv[i];
    c.x = c.x * sa[0]; c.y = c.y * sa[1]; c.z = c.z * sa[2];
    cv[i] = c;
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
int Renderer::enableGuides(float* device_g) {
    if (allocated) { last_error = "enable_guides must precede allocateOnGPU"; return -1; }
    guides_on = true;
    ext_guides = device_g;
    return 0;
}

// allocateOnGPU: G (unless the caller owns it) and one record buffer per pipeline, zeroed: a
// pixel that never emits a ray (tail_drop) contributes zeros.
int Renderer::allocGuides() {
    const size_t bytes = (size_t)cfg.width * cfg.height * 8 * sizeof(float);
    void* d = nullptr;
    if (ext_guides) {
        guides = ext_guides;
    } else {
        PT_HIP(hipMalloc(&d, bytes));
        allocs.push_back(d);
        guides = (float*)d;
    }
    for (int i = 0; i < npipes; i++) {
        PT_HIP(hipMalloc(&d, bytes));
        allocs.push_back(d);
        guide_contrib[i] = (float*)d;
        PT_HIP(hipMemsetAsync(d, 0, bytes, stream));
    }
    return 0;
}

// G += pipeline q's records on its stream st, right after launchMergeM2: the same place in the
// ordered merge chain, so the sums do not depend on the pipeline count.
int Renderer::launchMergeGuides(int q, hipStream_t st, const unsigned char* tile_mask) {
    const size_t n = (size_t)cfg.width * cfg.height;
    const int tx = noiseTilesX();
    if (((uintptr_t)guides & 15) == 0)
        hipLaunchKernelGGL(k_merge_guides<true>, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, st, guides,
                           guide_contrib[q], n, tile_mask, tx, cfg.width);
    else
        hipLaunchKernelGGL(k_merge_guides<false>, dim3((unsigned)((8 * n + 255) / 256)), dim3(256), 0, st, guides,
                           guide_contrib[q], n, tile_mask, tx, cfg.width);
    PT_HIP(hipGetLastError());
    return 0;
}

int Renderer::readGuides(float* host_g) {
    if (!allocated) { last_error = "not allocated"; return -1; }
    if (!guides_on) { last_error = "guides not enabled"; return -1; }
    PT_HIP(hipMemcpyAsync(host_g, guides, (size_t)cfg.width * cfg.height * 8 * sizeof(float), hipMemcpyDeviceToHost, stream));
    PT_HIP(hipStreamSynchronize(stream));
    return checkFaults();
}

int Renderer::guideCounts(int* tile_counts_host) {
    if (!allocated) { last_error = "not allocated"; return -1; }
    if (!guides_on) { last_error = "guides not enabled"; return -1; }
    if (tile_counts_host) std::copy(guide_tile_counts.begin(), guide_tile_counts.end(), tile_counts_host);
    return (int)guide_tile_counts.size();
}

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
    if (samples <= 0 && !countsUniform()) return refuseMixedCounts("noise");
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
    if (!countsUniform()) return refuseMixedCounts("render_until");      // it stops on noise(0)
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

// The denoiser's records, on the first denoise call: 56 bytes per pixel, freed with
// the renderer's other buffers.
int Renderer::allocDenoise() {
    if (dn_cv[0]) return 0;
    const size_t n = (size_t)cfg.width * cfg.height;
    void* d[5] = {};
    const size_t bytes[5] = {n * sizeof(float4), n * sizeof(float4), n * sizeof(float4), n * sizeof(int), n * sizeof(float)};
    for (int i = 0; i < 5; i++) {
        PT_HIP(hipMalloc(&d[i], bytes[i]));
        allocs.push_back(d[i]);
    }
    dn_cv[1] = (float4*)d[1];
    dn_nd = (float4*)d[2];
    dn_model = (int*)d[3];
    dn_slope = (float*)d[4];
    dn_cv[0] = (float4*)d[0];
    return 0;
}

template <int STEP>
static void launchDenoisePass(bool stage, dim3 grid, hipStream_t st, const float4* in, float4* out, const float4* nd,
                              const int* model, const float* slope, int W, int H, int tiles_x, float sl, float sz) {
    if (stage) hipLaunchKernelGGL((k_denoise_pass<STEP, true>), grid, dim3(kTileWG), 0, st, in, out, nd, model, slope, W, H, tiles_x, sl, sz);
    else hipLaunchKernelGGL((k_denoise_pass<STEP, false>), grid, dim3(kTileWG), 0, st, in, out, nd, model, slope, W, H, tiles_x, sl, sz);
}

template <bool VEC>
static void launchDenoisePrep(int flags, dim3 grid, hipStream_t st, const float* S, const float* Q, float nf,
                              const float4* cache_hit, const int* cache_model, int npix, int W, int H, float4* cv,
                              float4* nd, int* model, float* slope, const DnPrepOpt& opt) {
#define PT_PREP(D, C) \
    hipLaunchKernelGGL((k_denoise_prep<VEC, D, C>), grid, dim3(256), 0, st, S, Q, nf, cache_hit, cache_model, npix, W, H, \
                       cv, nd, model, slope, opt)
    switch (flags & (PT_DENOISE_DEMODULATE | PT_DENOISE_TILE_COUNTS)) {
        case 0: PT_PREP(false, false); break;
        case PT_DENOISE_DEMODULATE: PT_PREP(true, false); break;
        case PT_DENOISE_TILE_COUNTS: PT_PREP(false, true); break;
        default: PT_PREP(true, true); break;
    }
#undef PT_PREP
}

int Renderer::denoise(int samples, int passes, float sigma_l, float sigma_z, float* device_rgb_out, float* host_rgb,
                      float* host_var) {
    return denoiseEx(samples, passes, sigma_l, sigma_z, 0, device_rgb_out, host_rgb, host_var);
}

// flags 0: pt_renderer_denoise, launch for launch.  PT_DENOISE_DEMODULATE: prep divides by the
// primary hit's sqrt-space albedo and k_denoise_remod multiplies the last pass's colour by it, in
// the result buffer, before anything reads that.  PT_DENOISE_TILE_COUNTS: prep's nf is each
// tile's own sample count (the counts go up on the stream first, as for adaptiveNoise).
int Renderer::denoiseEx(int samples, int passes, float sigma_l, float sigma_z, int flags, float* device_rgb_out,
                        float* host_rgb, float* host_var) {
    if (!allocated) { last_error = "not allocated"; return -1; }
    if (!moments_on) { last_error = "moments not enabled"; return -1; }
    const bool demod = (flags & PT_DENOISE_DEMODULATE) != 0, by_tile = (flags & PT_DENOISE_TILE_COUNTS) != 0;
    const bool guided = (flags & PT_DENOISE_SAMPLED_GUIDES) != 0;
    const bool vouched = samples > 0;        // an explicit count: the caller vouches that every sample left a record
    if (flags & ~(PT_DENOISE_DEMODULATE | PT_DENOISE_TILE_COUNTS | PT_DENOISE_SAMPLED_GUIDES)) {
        last_error = "denoise_ex: unknown flag bits";
        return -1;
    }
    // without pt_renderer_enable_guides the bit is as unknown to this renderer as it was before guides existed
    if (guided && !guides_on) {
        last_error = "denoise_ex: unknown flag bits (PT_DENOISE_SAMPLED_GUIDES: guides not enabled; call "
                     "pt_renderer_enable_guides before allocate_on_gpu)";
        return -1;
    }
    if (by_tile && samples > 0) {
        last_error = "denoise_ex: PT_DENOISE_TILE_COUNTS takes every tile's own sample count; samples must be <= 0";
        return -1;
    }
    if (demod && cfg.max_bounces < 1) {
        last_error = "denoise_ex: PT_DENOISE_DEMODULATE needs max_bounces >= 1 (without a bounce no hit multiplies by its albedo)";
        return -1;
    }
    if (by_tile) {
        for (int c : tile_counts)
            if (c < 2) { last_error = "denoise_ex: PT_DENOISE_TILE_COUNTS needs at least 2 samples in every tile"; return -1; }
    } else {
        if (samples <= 0 && !countsUniform()) return refuseMixedCounts("denoise");
        if (samples <= 0) samples = samples_accumulated;
        if (samples < 2) { last_error = "need at least 2 samples"; return -1; }
    }
    if (guided && !vouched && guide_tile_counts != tile_counts) {
        last_error = "denoise_ex: PT_DENOISE_SAMPLED_GUIDES: a tile's guide count differs from its sample count; every "
                     "sample since the last clear must be a generated (jittered or lens) iteration, or pass samples > 0";
        return -1;
    }
    if (passes < 1 || passes > PT_DENOISE_MAX_PASSES || !std::isfinite(sigma_l) || !(sigma_l > 0.0f) ||
        !std::isfinite(sigma_z) || !(sigma_z > 0.0f)) {
        last_error = "bad denoise parameters";
        return -1;
    }
    // the largest step whose pass stages its tile in LDS (0: none); results are the same for every value
    int lds_step = kDenoiseLdsDefault;
    if (const char* e = std::getenv("PT_DENOISE_LDS")) {
        lds_step = std::atoi(e);
        if (lds_step != 0 && lds_step != 1 && lds_step != 2 && lds_step != 4 && lds_step != 8) {
            last_error = "PT_DENOISE_LDS must be 0, 1, 2, 4 or 8";
            return -1;
        }
    }
    if (allocDenoise() != 0) return -1;
    if (!guided && !cache_valid && launchPrimary() != 0) return -1;     // the guided prep reads G, not the cache
    if (by_tile && uploadTileCounts() != 0) return -1;
    const int W = cfg.width, H = cfg.height;
    const size_t n = (size_t)W * H;
    // HIP events around every kernel when profiling is on (denoiseTimes)
    for (hipEvent_t ev : dn_events) hipEventDestroy(ev);
    dn_events.clear();
    dn_event_passes = 0;
    dn_event_remod = false;
    const bool timed = profiling != 0;
    auto mark = [&]() -> int {
        if (!timed) return 0;
        hipEvent_t ev;
        PT_HIP(hipEventCreate(&ev));
        dn_events.push_back(ev);
        PT_HIP(hipEventRecord(ev, stream));
        return 0;
    };
    if (mark() != 0) return -1;
    const int tx = noiseTilesX();
    const DnPrepOpt opt = {demod ? kp.cache_albedo : nullptr, demod ? kp.shade : nullptr,
                           by_tile ? tile_counts_dev : nullptr, tx};
    const bool vec = (((uintptr_t)kp.image | (uintptr_t)m2) & 15) == 0;
    const bool gvec = ((uintptr_t)guides & 15) == 0;
    const dim3 gpix((unsigned)((n + 255) / 256));
    if (guided) {
#define PT_PREP_G(D, C) \
    hipLaunchKernelGGL((k_denoise_prep_guided<D, C>), gpix, dim3(256), 0, stream, kp.image, m2, (float)samples, guides, W, H, \
                       dn_cv[0], dn_nd, dn_model, dn_slope, opt.counts, tx, gvec)
        if (demod && by_tile) PT_PREP_G(true, true);
        else if (demod) PT_PREP_G(true, false);
        else if (by_tile) PT_PREP_G(false, true);
        else PT_PREP_G(false, false);
#undef PT_PREP_G
    } else if (vec) {
        const size_t n4 = n >> 2;
        launchDenoisePrep<true>(flags, dim3((unsigned)std::max<size_t>(1, (n4 + 255) / 256)), stream, kp.image, m2,
                                (float)samples, kp.cache_hit, kp.cache_model, kp.npix, W, H, dn_cv[0], dn_nd, dn_model,
                                dn_slope, opt);
    } else {
        launchDenoisePrep<false>(flags, dim3((unsigned)((n + 255) / 256)), stream, kp.image, m2, (float)samples,
                                 kp.cache_hit, kp.cache_model, kp.npix, W, H, dn_cv[0], dn_nd, dn_model, dn_slope, opt);
    }
    PT_HIP(hipGetLastError());
    if (mark() != 0) return -1;
    const dim3 grid((unsigned)(tx * noiseTilesY()));
    for (int s = 0; s < passes; s++) {
        const float4* in = dn_cv[s & 1];
        float4* out = dn_cv[(s + 1) & 1];
        const int step = 1 << s;
        const bool stage = step <= lds_step;
        switch (step) {
            case 1: launchDenoisePass<1>(stage, grid, stream, in, out, dn_nd, dn_model, dn_slope, W, H, tx, sigma_l, sigma_z); break;
            case 2: launchDenoisePass<2>(stage, grid, stream, in, out, dn_nd, dn_model, dn_slope, W, H, tx, sigma_l, sigma_z); break;
            case 4: launchDenoisePass<4>(stage, grid, stream, in, out, dn_nd, dn_model, dn_slope, W, H, tx, sigma_l, sigma_z); break;
            case 8: launchDenoisePass<8>(stage, grid, stream, in, out, dn_nd, dn_model, dn_slope, W, H, tx, sigma_l, sigma_z); break;
            case 16: hipLaunchKernelGGL((k_denoise_pass<16, false>), grid, dim3(kTileWG), 0, stream, in, out, dn_nd, dn_model, dn_slope, W, H, tx, sigma_l, sigma_z); break;
            default: hipLaunchKernelGGL((k_denoise_pass<32, false>), grid, dim3(kTileWG), 0, stream, in, out, dn_nd, dn_model, dn_slope, W, H, tx, sigma_l, sigma_z); break;
        }
        PT_HIP(hipGetLastError());
        if (mark() != 0) return -1;
    }
    dn_event_passes = timed ? passes : 0;
    float4* result = dn_cv[passes & 1];
    if (demod) {
        if (guided && by_tile)
            hipLaunchKernelGGL(k_denoise_remod_guided<true>, gpix, dim3(256), 0, stream, result, guides, n, (float)samples,
                               W, opt.counts, tx, gvec);
        else if (guided)
            hipLaunchKernelGGL(k_denoise_remod_guided<false>, gpix, dim3(256), 0, stream, result, guides, n, (float)samples,
                               W, opt.counts, tx, gvec);
        else
            hipLaunchKernelGGL(k_denoise_remod, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, result, dn_model, n,
                               kp.cache_albedo, kp.shade);
        PT_HIP(hipGetLastError());
        if (mark() != 0) return -1;
        dn_event_remod = timed;
    }
    if (device_rgb_out) {
        hipLaunchKernelGGL(k_denoise_out, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, result, n, device_rgb_out);
        PT_HIP(hipGetLastError());
    }
    if (mark() != 0) return -1;
    std::vector<float4> host;
    if (host_rgb || host_var) {
        host.resize(n);
        PT_HIP(hipMemcpyAsync(host.data(), result, n * sizeof(float4), hipMemcpyDeviceToHost, stream));
    }
    PT_HIP(hipStreamSynchronize(stream));
    if (checkFaults() != 0) return -1;
    for (size_t i = 0; i < host.size(); i++) {
        if (host_rgb) { host_rgb[3 * i] = host[i].x; host_rgb[3 * i + 1] = host[i].y; host_rgb[3 * i + 2] = host[i].z; }
        if (host_var) host_var[i] = host[i].w;
    }
    return 0;
}

// ms[0] prep, ms[1..6] the passes (0: not run), ms[7] the copy to the caller's device
// buffer, ms[8] first kernel to last, ms[9] the remodulation (0: not run): of the last
// denoise call made with profiling on.
int Renderer::denoiseTimes(double* ms, int n) {
    const int extra = dn_event_remod ? 1 : 0;
    if (dn_event_passes == 0 || (int)dn_events.size() != dn_event_passes + 3 + extra) {
        last_error = "no timed denoise call (set_profiling, then denoise)";
        return -1;
    }
    double v[10] = {};
    auto span = [&](int a, int b) {
        float t = 0.0f;
        hipEventElapsedTime(&t, dn_events[a], dn_events[b]);
        return (double)t;
    };
    v[0] = span(0, 1);
    for (int s = 0; s < dn_event_passes; s++) v[1 + s] = span(1 + s, 2 + s);
    if (extra) v[9] = span(dn_event_passes + 1, dn_event_passes + 2);
    v[7] = span(dn_event_passes + 1 + extra, dn_event_passes + 2 + extra);
    v[8] = span(0, dn_event_passes + 2 + extra);
    for (int i = 0; i < n; i++) ms[i] = i < 10 ? v[i] : 0.0;
    return 0;
}

// The denoised mean D through renderImage's writer: bytes of D * 255.
int Renderer::renderImageDenoised(const std::string& path, int samples, int passes, float sigma_l, float sigma_z,
                                  int flags) {
    std::vector<float> img((size_t)cfg.width * cfg.height * 3);
    if (denoiseEx(samples, passes, sigma_l, sigma_z, flags, nullptr, img.data(), nullptr) != 0) return -1;
    return writeBmp(path, img.data(), 1.0f);         // x * 1.0f is x
}

// ---------------------------------------------------------------------------
// Tile-masked sampling and the adaptive render.  The mask and the counts use the noise
// estimate's tiles.  Nothing here is allocated until the first masked or adaptive call.
// ---------------------------------------------------------------------------
bool Renderer::countsUniform() const {
    for (int c : tile_counts)
        if (c != tile_counts[0]) return false;
    return true;
}

int Renderer::refuseMixedCounts(const char* call) {
    last_error = std::string(call) + ": tiles have different sample counts after masked iterations; pass samples > 0, or use "
                 "pt_renderer_adaptive_noise / pt_renderer_adaptive_mean / pt_renderer_render_adaptive";
    return -1;
}

// Device mask and counts, and the pinned staging ring of the mask uploads: a slot is
// written again only after the copy that read it has completed (its event).
int Renderer::allocAdaptive() {
    if (tile_mask_dev) return 0;
    const size_t nt = (size_t)noiseTilesX() * noiseTilesY();
    void* d = nullptr;
    PT_HIP(hipMalloc(&d, nt * sizeof(int)));
    allocs.push_back(d);
    tile_counts_dev = (int*)d;
    PT_HIP(hipHostMalloc(&d, nt * kMaskSlots, hipHostMallocDefault));
    mask_stage = (unsigned char*)d;
    for (int i = 0; i < kMaskSlots; i++) PT_HIP(hipEventCreateWithFlags(&mask_ev[i], hipEventDisableTiming));
    mask_slot = 0;
    PT_HIP(hipMalloc(&d, nt));
    allocs.push_back(d);
    tile_mask_dev = (unsigned char*)d;
    return 0;
}

// freeBuffers: the streams are idle; the device buffers go with `allocs`
void Renderer::freeAdaptive() {
    if (mask_stage) hipHostFree(mask_stage);
    mask_stage = nullptr;
    for (int i = 0; i < kMaskSlots; i++) {
        if (mask_ev[i]) hipEventDestroy(mask_ev[i]);
        mask_ev[i] = nullptr;
    }
    tile_mask_dev = nullptr;
    tile_counts_dev = nullptr;
    am_out = nullptr;
}

int Renderer::uploadTileCounts() {
    if (allocAdaptive() != 0) return -1;
    // the callers synchronize before they return, and the counts change only in host calls
    PT_HIP(hipMemcpyAsync(tile_counts_dev, tile_counts.data(), tile_counts.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    return 0;
}

int Renderer::renderLoopMasked(int first_iter, int n_iters, const unsigned char* tile_mask_host) {
    if (!allocated) { last_error = "render_loop_masked before allocateOnGPU"; return -1; }
    if (!moments_on) { last_error = "moments not enabled (masked iterations need pt_renderer_enable_moments)"; return -1; }
    if (n_iters < 0 || first_iter < 0) { last_error = "bad iteration range"; return -1; }
    const size_t nt = tile_counts.size();
    size_t active = nt;
    if (tile_mask_host) {
        active = 0;
        for (size_t t = 0; t < nt; t++) active += tile_mask_host[t] != 0;
    }
    if (active == 0 || n_iters == 0) return 0;       // nothing to sample: nothing enqueued, nothing changed
    if (allocAdaptive() != 0) return -1;
    // The mask goes up on the caller's stream, before renderIters forks the pipeline
    // streams off it and after the join of every earlier call: the iterations of an
    // earlier masked call have read their mask before this copy overwrites it.
    unsigned char* stage = mask_stage + (size_t)mask_slot * nt;
    PT_HIP(hipEventSynchronize(mask_ev[mask_slot]));         // the copy that last read this slot (none: returns at once)
    for (size_t t = 0; t < nt; t++) stage[t] = tile_mask_host ? (tile_mask_host[t] != 0) : 1;
    PT_HIP(hipMemcpyAsync(tile_mask_dev, stage, nt, hipMemcpyHostToDevice, stream));
    PT_HIP(hipEventRecord(mask_ev[mask_slot], stream));
    mask_slot = (mask_slot + 1) % kMaskSlots;
    int done = 0;
    const int rc = renderIters(first_iter, n_iters, tile_mask_dev, &done);
    const bool gen = guides_on && generatedIterations();
    for (size_t t = 0; t < nt; t++)
        if (stage[t]) {
            tile_counts[t] += done;
            if (gen) guide_tile_counts[t] += done;
        }
    return rc;
}

int Renderer::sampleCounts(int* tile_counts_host) {
    if (!allocated) { last_error = "not allocated"; return -1; }
    if (tile_counts_host) std::copy(tile_counts.begin(), tile_counts.end(), tile_counts_host);
    return (int)tile_counts.size();
}

int Renderer::adaptiveNoise(double* mean_err, float* max_tile_err, float* tile_err_host) {
    if (!allocated) { last_error = "not allocated"; return -1; }
    if (!moments_on) { last_error = "moments not enabled"; return -1; }
    if (uploadTileCounts() != 0) return -1;
    const int tx = noiseTilesX(), ty = noiseTilesY(), nt = tx * ty;
    hipLaunchKernelGGL(k_noise_tiles_counts, dim3((unsigned)nt), dim3(kTileWG), 0, stream, kp.image, m2, cfg.width,
                       cfg.height, tx, tile_counts_dev, noise_sum, noise_err);
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

int Renderer::adaptiveMean(float* device_rgb_out, float* host_rgb) {
    if (!allocated) { last_error = "not allocated"; return -1; }
    if (uploadTileCounts() != 0) return -1;
    const size_t n3 = (size_t)cfg.width * cfg.height * 3;
    float* out = device_rgb_out;
    if (!out) {
        if (!am_out) {
            void* d = nullptr;
            PT_HIP(hipMalloc(&d, n3 * sizeof(float)));
            allocs.push_back(d);
            am_out = (float*)d;
        }
        out = am_out;
    }
    const bool vec = (((uintptr_t)kp.image | (uintptr_t)out) & 15) == 0;
    if (vec) {
        const size_t n4 = n3 >> 2;
        hipLaunchKernelGGL(k_mean_counts<true>, dim3((unsigned)std::max<size_t>(1, (n4 + 255) / 256)), dim3(256), 0, stream,
                           kp.image, out, n3, cfg.width, noiseTilesX(), tile_counts_dev);
    } else {
        hipLaunchKernelGGL(k_mean_counts<false>, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, stream,
                           kp.image, out, n3, cfg.width, noiseTilesX(), tile_counts_dev);
    }
    PT_HIP(hipGetLastError());
    if (host_rgb) PT_HIP(hipMemcpyAsync(host_rgb, out, n3 * sizeof(float), hipMemcpyDeviceToHost, stream));
    PT_HIP(hipStreamSynchronize(stream));
    return checkFaults();
}

int Renderer::renderImageAdaptive(const std::string& path) {
    std::vector<float> img((size_t)cfg.width * cfg.height * 3);
    if (adaptiveMean(nullptr, img.data()) != 0) return -1;
    return writeBmp(path, img.data(), 1.0f);         // x * 1.0f is x
}

// Chunks of check_every masked iterations, every tile active at first; after each chunk
// that brings this call's count to max(min_iters, 2) or more, the per-tile estimate over
// every sample in the accumulator switches off, for the rest of the call, the tiles at or
// below tile_target.  1: no tile is active any more, 0: max_iters reached.
int Renderer::renderAdaptive(int first_iter, int min_iters, int max_iters, int check_every, double tile_target,
                             int* iters_done, long long* pixel_samples, double* mean_err) {
    if (!allocated) { last_error = "not allocated"; return -1; }
    if (!moments_on) { last_error = "moments not enabled"; return -1; }
    if (first_iter < 0 || max_iters < 1) { last_error = "bad iteration range"; return -1; }
    if (check_every <= 0) check_every = 32;
    const int min_check = std::max(min_iters, 2);
    const int tx = noiseTilesX(), ty = noiseTilesY(), nt = tx * ty;
    std::vector<unsigned char> mask((size_t)nt, 1);
    std::vector<float> terr((size_t)nt);
    auto tile_pixels = [&](int t) {
        const int rw = cfg.width - (t % tx) * kTile, rh = cfg.height - (t / tx) * kTile;
        return (long long)std::min(rw, kTile) * std::min(rh, kTile);
    };
    int done = 0, n_active = nt;
    long long taken = 0, active_pixels = (long long)cfg.width * cfg.height;
    double mean = -1.0;
    bool fresh = false;
    while (done < max_iters && n_active > 0) {
        const int n = std::min(check_every, max_iters - done);
        if (renderLoopMasked(first_iter + done, n, mask.data()) != 0) return -1;
        done += n;
        taken += active_pixels * n;
        fresh = false;
        if (done >= min_check) {
            if (adaptiveNoise(&mean, nullptr, terr.data()) != 0) return -1;
            fresh = true;
            n_active = 0;
            active_pixels = 0;
            for (int t = 0; t < nt; t++) {
                if (mask[t] && (double)terr[t] <= tile_target) mask[t] = 0;
                if (mask[t]) { n_active++; active_pixels += tile_pixels(t); }
            }
        }
    }
    if (!fresh && adaptiveNoise(&mean, nullptr, nullptr) != 0) return -1;     // min_iters beyond max_iters
    if (iters_done) *iters_done = done;
    if (pixel_samples) *pixel_samples = taken;
    if (mean_err) *mean_err = mean;
    return n_active == 0 ? 1 : 0;
}

// ---------------------------------------------------------------------------
// Environment lighting (pt_env.h): the host side.  The shading pass reads the record through
// KParams::env (shade_mat, renderer.hip); nothing else on the device knows of it.
// ---------------------------------------------------------------------------

// Test hook (pt_renderer_env_lookup): env_radiance of caller-given directions.
__global__ __launch_bounds__(256) void k_env_lookup(const EnvRec* env, int n, const float* __restrict__ dirs,
                                                    float* __restrict__ rgb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const f3 v = env_radiance(*env, mk3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
    rgb[3 * i] = v.x; rgb[3 * i + 1] = v.y; rgb[3 * i + 2] = v.z;
}

// The texels and the record, on the caller's stream.  The host copies (env_texels, env_rec)
// stay as they are until the next setEnvironment, which waits for the stream first.
int Renderer::uploadEnvironment() {
    const size_t nt = env_texels.size();
    if (nt > env_texels_cap) {
        if (env_texels_dev) PT_HIP(hipFree(env_texels_dev));
        env_texels_dev = nullptr;
        env_texels_cap = 0;
        PT_HIP(hipMalloc(&env_texels_dev, nt * sizeof(float4)));
        env_texels_cap = nt;
    }
    PT_HIP(hipMemcpyAsync(env_texels_dev, env_texels.data(), nt * sizeof(float4), hipMemcpyHostToDevice, stream));
    env_rec.texels = env_texels_dev;
    PT_HIP(hipMemcpyAsync(env_dev, &env_rec, sizeof(EnvRec), hipMemcpyHostToDevice, stream));
    return 0;
}

int Renderer::setEnvironment(const pt_environment* env) {
    if (env) {
        if (env->n < 1 || env->n > kEnvMaxN) { last_error = "set_environment: n must be 1 .. 2048"; return -1; }
        if (!env->texels_rgb) { last_error = "set_environment: null texels"; return -1; }
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(env->scale[k])) { last_error = "set_environment: every scale entry must be finite"; return -1; }
        for (int k = 0; k < 9; k++)
            if (!std::isfinite(env->rotation[k])) { last_error = "set_environment: every rotation entry must be finite"; return -1; }
        const size_t nf = (size_t)env->n * env->n * 3;
        for (size_t i = 0; i < nf; i++)
            if (!std::isfinite(env->texels_rgb[i])) { last_error = "set_environment: every texel must be finite"; return -1; }
    }
    if (allocated) {
        // Every render call has joined its pipelines back into the caller's stream; once that
        // stream is idle nothing reads the old texels or the host copies.  Captured launches
        // hold KParams::env by value, so the graphs go when it changes between null and set.
        PT_HIP(hipStreamSynchronize(stream));
        if ((env != nullptr) != env_on) {
            for (int i = 1; i < npipes; i++) PT_HIP(hipStreamSynchronize(pstream[i]));
            dropGraphs();
        }
    }
    env_on = env != nullptr;
    if (env) {
        const size_t nt = (size_t)env->n * env->n;
        env_texels.resize(nt);
        for (size_t i = 0; i < nt; i++)
            env_texels[i] = make_float4(env->texels_rgb[3 * i], env->texels_rgb[3 * i + 1], env->texels_rgb[3 * i + 2], 0.0f);
        env_rec.n = env->n;
        for (int k = 0; k < 3; k++) env_rec.scale[k] = env->scale[k];
        for (int k = 0; k < 9; k++) env_rec.rot[k] = env->rotation[k];
    }
    if (!allocated) return 0;
    if (env && uploadEnvironment() != 0) return -1;
    kp.env = env ? env_dev : nullptr;
    for (int i = 0; i < kMaxPipes; i++) pk[i].env = kp.env;
    return clearImage();                             // a new environment is a new render; the primary hits stay
}

int Renderer::environment(pt_environment* out, float* texels_out) const {
    if (!env_on) return 0;
    if (out) {
        out->n = env_rec.n;
        out->texels_rgb = nullptr;
        for (int k = 0; k < 3; k++) out->scale[k] = env_rec.scale[k];
        for (int k = 0; k < 9; k++) out->rotation[k] = env_rec.rot[k];
    }
    if (texels_out)
        for (size_t i = 0; i < env_texels.size(); i++) {
            texels_out[3 * i] = env_texels[i].x; texels_out[3 * i + 1] = env_texels[i].y; texels_out[3 * i + 2] = env_texels[i].z;
        }
    return 1;
}

int Renderer::envLookup(int count, const float* dirs, float* rgb_out) {
    if (!allocated) { last_error = "env_lookup: not allocated"; return -1; }
    if (!env_on) { last_error = "env_lookup: no environment is set"; return -1; }
    if (count < 0 || (count > 0 && (!dirs || !rgb_out))) { last_error = "env_lookup: bad arguments"; return -1; }
    if (count == 0) return 0;
    float *d_d = nullptr, *d_c = nullptr;
    const size_t bytes = (size_t)count * 3 * sizeof(float);
    PT_HIP(hipMalloc(&d_d, bytes));
    hipError_t e = hipMalloc(&d_c, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(d_d, dirs, bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_env_lookup, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, env_dev, count, d_d, d_c);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(rgb_out, d_c, bytes, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    hipFree(d_d);
    hipFree(d_c);
    if (e != hipSuccess) return fail(e, "env_lookup");
    return 0;
}

}  // namespace pt
