// pt_env.h -- environment lighting: the radiance a ray that leaves the scene brings back,
// read from an octahedral map (pt_environment, include/pathtracer_amd.h; no counterpart in
// the reference, whose missing rays are a constant 0.01 grey).
//
// Octahedral rather than latitude-longitude: the mapping needs only IEEE add, multiply,
// divide, sqrt and compare, so it is bit-reproducible without atan2 / acos.  All arithmetic
// is float32 in the order written; the translation units are built with -ffp-contract=off.
#pragma once

#include "pt_math.h"

namespace pt {

constexpr int kEnvMaxN = 2048;      // largest map edge: 2048 * 2048 float4 texels = 64 MiB

// One device record per renderer behind KParams::env.
struct EnvRec {
    const float4* texels;   // n * n texels, row y column x at [y * n + x]: (r, g, b, unused)
    int n;                  // 1 .. kEnvMaxN
    float scale[3];         // multiplies the interpolated texel
    float rot[9];           // row-major, world -> environment frame; the frame's +z is the map's centre
};

// One axis of the bilinear footprint: octahedral coordinate p in [-1, 1] -> texel i0, its
// clamped neighbour i1 and the weight t of i1.  fmaxf drops a NaN (it returns its other
// argument), so a NaN coordinate reads texel 0 with weight 0: no load leaves the map.
PT_HD void env_axis(float p, int n, int& i0, int& i1, float& t) {
    float f = ((p * 0.5f + 0.5f) * (float)n) - 0.5f;
    f = fminf(fmaxf(f, 0.0f), (float)(n - 1));
    i0 = (int)f;
    i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
    t = f - (float)i0;
}

// The radiance from direction d (any length).  Clamp-to-edge bilinear: the map's outer edge
// is a fold line of the lower hemisphere, where the interpolation is off by at most half a
// texel (no octahedral wrap).
PT_HD f3 env_radiance(const EnvRec& env, f3 d) {
    const f3 u = normalize(d);
    const f3 e = mk3(dot(mk3(env.rot[0], env.rot[1], env.rot[2]), u), dot(mk3(env.rot[3], env.rot[4], env.rot[5]), u),
                     dot(mk3(env.rot[6], env.rot[7], env.rot[8]), u));
    const float l = (fabsf(e.x) + fabsf(e.y)) + fabsf(e.z);
    float px = e.x / l, py = e.y / l;
    if (e.z < 0.0f) {       // the lower hemisphere folds over the diamond's edges into the corners
        const float qx = (1.0f - fabsf(py)) * (px >= 0.0f ? 1.0f : -1.0f);
        const float qy = (1.0f - fabsf(px)) * (py >= 0.0f ? 1.0f : -1.0f);
        px = qx;
        py = qy;
    }
    int x0, x1, y0, y1;
    float tx, ty;
    env_axis(px, env.n, x0, x1, tx);
    env_axis(py, env.n, y0, y1, ty);
    const float4 a = env.texels[y0 * env.n + x0], b = env.texels[y0 * env.n + x1];
    const float4 c = env.texels[y1 * env.n + x0], g = env.texels[y1 * env.n + x1];
    const f3 top = mk3(a.x + (b.x - a.x) * tx, a.y + (b.y - a.y) * tx, a.z + (b.z - a.z) * tx);
    const f3 bot = mk3(c.x + (g.x - c.x) * tx, c.y + (g.y - c.y) * tx, c.z + (g.z - c.z) * tx);
    const f3 v = top + (bot - top) * ty;
    return v * mk3(env.scale[0], env.scale[1], env.scale[2]);
}

}  // namespace pt
