// main.cpp -- command-line renderer (the reference's main.cpp:11-27):
// load a scene, allocate on the GPU, run the render loop, write Render.bmp.
//
//   pathtracer_amd <scene.txt> [out.bmp] [--res W H] [--iter N] [--bounces B] [--grid|--grid-fast|--bvh]
//                  [--pipelines P] [--noise-target X [--check-every N]] [--denoise [--denoise-passes N]]
//                  [--denoise-albedo] [--denoise-guides] [--adaptive X [--check-every N] [--min-iter N]] [--jitter WIDTH]
//                  [--look-from X Y Z --look-at X Y Z [--up X Y Z] [--fov DEG] [--focus D] [--lens R]]
//                  [--sky ZR ZG ZB HR HG HB [--ground R G B]] [--smooth]
//
// --smooth: smooth shading for every model (pt_scene_set_model_smooth with model -1): a hit's
// normal interpolates the vertex normals instead of using one per triangle.  Without it the
// scene file's shading:smooth attributes apply.
//
// --sky: environment lighting (pt_environment_sky, pt_renderer_set_environment): a ray that
// leaves the scene brings back the horizon colour blended towards the zenith colour with its
// height, and --ground (default 0 0 0) from below the horizon; world +y is up.  A 64 x 64
// octahedral map.  Without it such a ray brings back the reference's constant 0.01.
//
// --look-from / --look-at: a free camera (pt_camera_look_at, pt_renderer_set_camera) at the
// first point looking at the second, with --up (default 0 1 0), a vertical field of view of
// --fov degrees (default 45), the plane in focus --focus away (default the distance between
// the two points) and a thin lens of radius --lens (default 0: a pinhole, everything sharp).
// Without them the scene file's camera_* keys apply, and without those the legacy camera.
//
// --jitter WIDTH: anti-aliasing (pt_renderer_set_pixel_jitter): every iteration's camera
// rays go through a point drawn from a WIDTH-pixel square about the pixel's own point
// (1 = the pixel's extent); works with every other option.
//
// --noise-target X: render until the mean relative noise estimate (pt_renderer_noise)
// is at most X, checked every N iterations (default 32); --iter is then the most
// iterations to render, and the BMP is divided by the iterations actually rendered.
//
// --adaptive X: tile-based adaptive sampling (pt_renderer_render_adaptive): a 16 x 16 tile
// stops receiving samples once its noise estimate is at most X, checked every N iterations
// (default 32) from --min-iter (default 2) on; --iter is the most iterations, and the BMP
// is the per-tile mean (pt_renderer_render_image_adaptive).
//
// --denoise: keep the second moments and write the BMP of the denoised mean
// (pt_renderer_render_image_denoised over the iterations actually rendered, N a-trous
// passes, default 5) instead of the raw mean.  --denoise-albedo implies --denoise and filters the
// image with the primary hit's albedo divided out (pt_renderer_render_image_denoised_ex with
// PT_DENOISE_DEMODULATE), so a texture is not blurred.  --denoise-guides implies --denoise too:
// the filter's guides are the means of the samples' own first hits (pt_renderer_enable_guides,
// PT_DENOISE_SAMPLED_GUIDES); it needs --jitter or a lens, whose iterations accumulate them.
//
// --direct-light: direct lighting (pt_renderer_set_direct_light): every diffuse hit samples the
// lights through a shadow ray.  It implies the moments; the scene file's RENDER key
// direct_light: 1 does the same.
//
// Default: PT_ACCEL_GRID_FAST (the reference grid's image, bit for bit) with 16
// iterations in flight, each on its own HIP stream and hardware queue.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/pathtracer_amd.h"

int main(int argc, char** argv) {
    // one hardware queue per pipeline stream; read once when the HIP runtime starts
    // (the library sets the same default when it loads; an explicit choice wins)
    setenv("GPU_MAX_HW_QUEUES", "16", /*overwrite=*/0);
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s scene.txt [out.bmp] [--res W H] [--iter N] [--bounces B] "
                             "[--grid|--grid-fast|--bvh] [--pipelines P] [--noise-target X [--check-every N]] "
                             "[--denoise [--denoise-passes N]] [--denoise-albedo] [--denoise-guides] [--adaptive X [--check-every N] [--min-iter N]] "
                             "[--jitter WIDTH] [--look-from X Y Z --look-at X Y Z [--up X Y Z] [--fov DEG] "
                             "[--focus D] [--lens R]] [--sky ZR ZG ZB HR HG HB [--ground R G B]] [--smooth] [--direct-light]\n", argv[0]);
        return 2;
    }
    pt_render_config cfg;
    pt_default_config(&cfg);
    pt_scene* s = pt_scene_create();
    if (pt_scene_load_config(s, argv[1]) < 0) { std::fprintf(stderr, "%s\n", pt_last_error()); return 1; }
    pt_scene_apply_settings(s, &cfg);
    const char* out = "Render.bmp";
    double noise_target = -1.0;          // < 0: render cfg.iterations
    int check_every = 32;
    double adaptive_target = -1.0;       // >= 0: tile-based adaptive sampling
    int min_iter = 2;
    bool denoise = false;
    int denoise_flags = 0;
    bool jitter = false;
    float jitter_width = 1.0f;
    bool has_from = false, has_at = false, has_focus = false, cam_opt = false;
    double eye[3] = {0, 0, 0}, target[3] = {0, 0, 0}, up[3] = {0, 1, 0};
    double fov = 45.0, focus = 0.0, lens = 0.0;       // no --focus: the distance from eye to target
    auto vec3 = [&](double* v, int& i) { for (int k = 0; k < 3; k++) v[k] = std::atof(argv[++i]); };
    bool sky = false, has_ground = false, smooth = false;
    bool direct = pt_scene_direct_light(s) > 0;
    double zenith[3] = {0, 0, 0}, horizon[3] = {0, 0, 0}, ground[3] = {0, 0, 0};
    pt_denoise_params dn;
    pt_default_denoise_params(&dn);
    for (int i = 2; i < argc; i++) {
        if (!std::strcmp(argv[i], "--res") && i + 2 < argc) { cfg.width = std::atoi(argv[++i]); cfg.height = std::atoi(argv[++i]); }
        else if (!std::strcmp(argv[i], "--iter") && i + 1 < argc) cfg.iterations = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--bounces") && i + 1 < argc) cfg.max_bounces = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--bvh")) cfg.accel = PT_ACCEL_BVH;
        else if (!std::strcmp(argv[i], "--grid-fast")) cfg.accel = PT_ACCEL_GRID_FAST;
        else if (!std::strcmp(argv[i], "--grid")) cfg.accel = PT_ACCEL_GRID;
        else if (!std::strcmp(argv[i], "--pipelines") && i + 1 < argc) cfg.pipelines = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--noise-target") && i + 1 < argc) noise_target = std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--check-every") && i + 1 < argc) check_every = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--adaptive") && i + 1 < argc) adaptive_target = std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--min-iter") && i + 1 < argc) min_iter = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--jitter") && i + 1 < argc) { jitter = true; jitter_width = (float)std::atof(argv[++i]); }
        else if (!std::strcmp(argv[i], "--look-from") && i + 3 < argc) { vec3(eye, i); has_from = true; }
        else if (!std::strcmp(argv[i], "--look-at") && i + 3 < argc) { vec3(target, i); has_at = true; }
        else if (!std::strcmp(argv[i], "--up") && i + 3 < argc) { vec3(up, i); cam_opt = true; }
        else if (!std::strcmp(argv[i], "--fov") && i + 1 < argc) { fov = std::atof(argv[++i]); cam_opt = true; }
        else if (!std::strcmp(argv[i], "--focus") && i + 1 < argc) { focus = std::atof(argv[++i]); has_focus = cam_opt = true; }
        else if (!std::strcmp(argv[i], "--lens") && i + 1 < argc) { lens = std::atof(argv[++i]); cam_opt = true; }
        else if (!std::strcmp(argv[i], "--sky") && i + 6 < argc) { vec3(zenith, i); vec3(horizon, i); sky = true; }
        else if (!std::strcmp(argv[i], "--ground") && i + 3 < argc) { vec3(ground, i); has_ground = true; }
        else if (!std::strcmp(argv[i], "--smooth")) smooth = true;
        else if (!std::strcmp(argv[i], "--direct-light")) direct = true;
        else if (!std::strcmp(argv[i], "--denoise")) denoise = true;
        else if (!std::strcmp(argv[i], "--denoise-albedo")) { denoise = true; denoise_flags |= PT_DENOISE_DEMODULATE; }
        else if (!std::strcmp(argv[i], "--denoise-guides")) { denoise = true; denoise_flags |= PT_DENOISE_SAMPLED_GUIDES; }
        else if (!std::strcmp(argv[i], "--denoise-passes") && i + 1 < argc) dn.passes = std::atoi(argv[++i]);
        else out = argv[i];
    }
    if (adaptive_target >= 0 && (noise_target >= 0 || denoise)) {
        std::fprintf(stderr, "--adaptive excludes --noise-target and --denoise\n");
        return 2;
    }
    if (has_from != has_at || (cam_opt && !has_from)) {
        std::fprintf(stderr, "a camera needs both --look-from and --look-at\n");
        return 2;
    }
    if (has_ground && !sky) {
        std::fprintf(stderr, "--ground needs --sky\n");
        return 2;
    }
    pt_camera cam;
    int has_cam = 0;
    if (has_from) {
        if (!has_focus) {
            double d2 = 0;
            for (int k = 0; k < 3; k++) d2 += (target[k] - eye[k]) * (target[k] - eye[k]);
            focus = std::sqrt(d2);
        }
        has_cam = pt_camera_look_at(eye, target, up, fov, focus, lens, cfg.width, cfg.height, &cam) < 0 ? -1 : 1;
    } else {
        has_cam = pt_scene_camera(s, cfg.width, cfg.height, &cam);
    }
    if (has_cam < 0) { std::fprintf(stderr, "%s\n", pt_last_error()); return 1; }
    const bool guides = (denoise_flags & PT_DENOISE_SAMPLED_GUIDES) != 0;
    if (guides && !jitter && !(has_cam > 0 && cam.lens_radius > 0.0f)) {
        std::fprintf(stderr, "--denoise-guides needs --jitter or a lens (--lens R): only their iterations accumulate guides\n");
        return 2;
    }
    if (smooth && pt_scene_set_model_smooth(s, -1, 1) < 0) { std::fprintf(stderr, "%s\n", pt_last_error()); return 1; }
    if (pt_scene_build(s, cfg.grid, cfg.accel != PT_ACCEL_GRID) < 0) { std::fprintf(stderr, "%s\n", pt_last_error()); return 1; }
    pt_renderer* r = pt_renderer_create(&cfg);
    if (!r || ((noise_target >= 0 || denoise || adaptive_target >= 0 || direct) && pt_renderer_enable_moments(r, nullptr) < 0) ||
        (direct && pt_renderer_set_direct_light(r, 1) < 0) || (guides && pt_renderer_enable_guides(r, nullptr) < 0) || pt_renderer_allocate_on_gpu(r, s) < 0) {
        std::fprintf(stderr, "%s\n", pt_last_error());
        return 1;
    }
    if (has_cam > 0 && pt_renderer_set_camera(r, &cam) < 0) { std::fprintf(stderr, "%s\n", pt_last_error()); return 1; }
    if (sky) {
        constexpr int n = 64;
        static float texels[n * n * 3];
        float z[3], h[3], g[3];
        for (int k = 0; k < 3; k++) { z[k] = (float)zenith[k]; h[k] = (float)horizon[k]; g[k] = (float)ground[k]; }
        // the environment frame's +z (the zenith) is world +y: e = (u.z, u.x, u.y)
        pt_environment env = {n, texels, {1.0f, 1.0f, 1.0f}, {0, 0, 1, 1, 0, 0, 0, 1, 0}};
        if (pt_environment_sky(z, h, g, n, texels) < 0 || pt_renderer_set_environment(r, &env) < 0) {
            std::fprintf(stderr, "%s\n", pt_last_error());
            return 1;
        }
    }
    if (jitter && pt_renderer_set_pixel_jitter(r, 1, jitter_width) < 0) { std::fprintf(stderr, "%s\n", pt_last_error()); return 1; }
    int iters = cfg.iterations;
    auto t0 = std::chrono::high_resolution_clock::now();
    if (adaptive_target >= 0) {
        double mean = 0.0;
        long long taken = 0;
        const int rc = pt_renderer_render_adaptive(r, 0, min_iter, cfg.iterations, check_every, adaptive_target, &iters,
                                                   &taken, &mean);
        if (rc < 0) { std::fprintf(stderr, "%s\n", pt_last_error()); return 1; }
        const double full = (double)iters * cfg.width * cfg.height;
        std::printf("%s after %d of at most %d iterations: %lld pixel samples, %.1f %% of iterations x pixels; "
                    "noise estimate %.6g (tile target %.6g)\n", rc ? "Every tile converged" : "Not every tile converged",
                    iters, cfg.iterations, taken, full > 0 ? 100.0 * (double)taken / full : 0.0, mean, adaptive_target);
    } else if (noise_target >= 0) {
        double mean = 0.0;
        const int rc = pt_renderer_render_until(r, 0, 2, cfg.iterations, check_every, noise_target, &iters, &mean);
        if (rc < 0) { std::fprintf(stderr, "%s\n", pt_last_error()); return 1; }
        std::printf("%s after %d of at most %d iterations: noise estimate %.6g (target %.6g)\n",
                    rc ? "Converged" : "Not converged", iters, cfg.iterations, mean, noise_target);
    } else if (pt_renderer_render_loop(r, 0, cfg.iterations) < 0 || pt_renderer_synchronize(r) < 0) {
        std::fprintf(stderr, "%s\n", pt_last_error());
        return 1;
    }
    auto t1 = std::chrono::high_resolution_clock::now();
    double us = std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
    long long seg = pt_renderer_segments(r);
    std::printf("Full run: %.0f microseconds, %lld ray segments, %.2f Mrays/s\n", us, seg, seg / us);
    if ((adaptive_target >= 0 ? pt_renderer_render_image_adaptive(r, out)
         : denoise ? (denoise_flags ? pt_renderer_render_image_denoised_ex(r, out, iters, &dn, denoise_flags)
                                 : pt_renderer_render_image_denoised(r, out, iters, &dn)) : pt_renderer_render_image(r, out, iters)) < 0) { std::fprintf(stderr, "%s\n", pt_last_error()); return 1; }
    pt_renderer_free(r);
    pt_scene_destroy(s);
    return 0;
}
