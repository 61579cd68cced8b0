// renderer.h -- MI355X wavefront renderer (Renderer.h:46-55 mirror).
//
// allocateOnGPU / renderLoop / renderImage / free keep the reference's
// entry points; underneath, each bounce is a persistent trace kernel
// (grid_fast / bvh; grid_fast after a counting sort of the live rays) and a
// shading kernel (BSDF scatter + block-local stable compaction + framebuffer
// accumulate of terminated rays), then a one-workgroup block-offset scan --
// no host round trip inside an iteration.  `pipelines` iterations run at once
// on their own HIP streams; their contributions merge in iteration order.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/pathtracer_amd.h"   // PT_NOISE_TILE, pt_environment
#include "pt_env.h"
#include "scene.h"

namespace pt {

struct RenderConfig {            // Config.h + generateRaysKernel constants, at runtime
    int width = 1000, height = 800;       // RESOLUTION_X/Y
    int iterations = 500;                 // ITER
    int max_bounces = 5;                  // Renderer.cpp:550
    int accel = ACCEL_GRID_FAST;          // the reference grid's results, bit for bit, through the BLAS
    int grid[3] = {25, 25, 25};           // GRID_X/Y/Z
    int tail_drop = 0;                    // replicate ceil(n/32) launch truncation (Renderer.cpp:573)
    int block = 64;                       // bounce-kernel workgroup size = compaction chunk (64/128/256)
    int ray_sort = -1;                    // -1 auto (grid_fast: key 7), 0 off, 1..8 key layout (k_sort_hist)
    int pipelines = 16;                   // iterations in flight on their own HIP streams (1..kMaxPipes)
    double cam[3] = {0.0, 0.0, 920.0};    // Renderer.cpp:528
    double plane_z = 900.0;               // Renderer.cpp:543
    double plane_x0 = -10.0, plane_y0 = -4.0, plane_w = 20.0, plane_h = 16.0;  // Renderer.cpp:538-542
};

// The free camera (pt_camera, include/pathtracer_amd.h; no counterpart in the reference): one
// device record per renderer behind KParams::camera, written by k_set_camera on the renderer's
// stream.  The same layout as pt_camera.
struct CameraRec {
    float origin[3];            // centre of the lens
    float p0[3];                // world point of pixel coordinates (0, 0)
    float du[3], dv[3];         // world step per pixel in x and in y
    float lens_u[3], lens_v[3]; // the lens's two spanning vectors
    float lens_radius;          // 0: pinhole
};

// Everything a kernel needs, passed by value as the kernel argument.
struct KParams {
    // scene (read-only, stays L2/MALL resident)
    const ModelRec* models;
    const ModelShade* shade;    // per model: material (shading pass)
    int nmodels;
    int gdim[3];
    const float4* tri_geom;     // 3 float4 per triangle: v0, e1, e2
    const float4* tri_normal;   // 1 float4 per triangle
    const int2* voxels;         // (start, end)
    const int* per_voxel;
    const Bvh4Node* bvh4;       // the BLAS, 4-wide: every BLAS path walks it (nullptr when the scene has none)
    const float4* bvh_tri_geom; // leaf-ordered triangle records, v0.w = triangle index
    int* spill;                 // traversal-stack spill beyond the LDS entries, lane-minor
    int spill_stride;           // lanes in the spill layout
    // frame
    int width, height, npix, max_bounces, nblocks, chunk;
    float step_x, step_y, cam_x, cam_y, cam_z, plane_z;
    double plane_x0, plane_y0;
    float4* ray[2][3];          // ping-pong SoA planes: (o, pixel) (d, bounces) (color, -)
    float4* cache_hit;          // primary hit: dist, normal
    int* cache_model;
    float* image;               // W*H*3 accumulator (Pixel::color)
    int* blk_cnt;
    int* blk_off;
    int* dst_start;
    int* n_live;                // live rays per bounce
    unsigned long long* segments;      // [0] total, [1 + b] live rays entering bounce b, [65] diagnostics
    int debug;                          // timing-only ablation switches (PT_DEBUG_ABLATE); 0 in production
    int4* hs_pool;                      // ACCEL_GRID_FAST overflow hit sets (64-member blocks)
    int* hs_pool_next;                  // bump allocator, reset by k_scan every bounce
    int hs_pool_blocks;
    float4* hit4;                       // split trace/shade (ACCEL_BVH): per-slot dist, normal
    int* hitm;                          // per-slot model
    int* trace_next;                    // persistent trace: next unclaimed source block, reset by k_scan
    int trace_refill;                   // refill a wave's idle lanes once this many are idle
    int trace_rpl;                      // main trace launch: waves beyond ceil(n / (64 * trace_rpl)) exit at once (0: off)
    int trace_min_blocks;               // ... but at least this many waves run
    int trace_flags;                    // k_trace_bvh variant: 11 LDS model records, 10 global
    int* defer_slots;                   // k_trace_gf: slots whose hit set overflowed LDS (k_trace_deferred)
    int* defer_count;                   // reset by k_scan
    float* contrib;                     // pipelines > 1 or moments on: this pipeline's per-iteration contributions
                                        // (k_merge / k_merge_m2); null: k_bounce adds straight into the image
    int2* order;                        // ray sort: claim position -> (dense slot, source index); null: claim order
    int* sort_bins;                     // [kSortBins] rays per key, [kSortBins] scatter cursors; zeroed by k_scan
    unsigned short* sort_key;           // per source index of the previous bounce's pool
    int sort_mode;                      // key layout (k_sort_hist); 0 = no sort
    float sort_lo[3], sort_sc[3];       // origin cell = (o - lo) * sc, scene world box
    int* iter_dev;                      // hipGraph replay: k_bounce's iteration id (its `iter` argument is -1)
    int* cont;                          // drain continuations: rays a persistent trace handed on (SoA, stride cont_cap)
    int cont_cap;
    int* cont_count;                    // [level] records written by that launch, [kDrainLevels + level]
                                        // walk hand-ons it wrote (k_trace_gf; reset by k_scan)
    int cont_wcap;                      // walk hand-on records per launch (at the top of the buffer; 0: off)
    int* cont_next;                     // [level] of them claimed by the next tail launch (reset by k_scan)
    int drain_levels;                   // tail launches after the main one (PT_DRAIN_LEVELS); the last one
                                        // hands nothing on.  Record buffers alternate between levels
    int drain_dump;                     // hand a wave's rays on once the pool is exhausted and <= this many
                                        // lanes still trace (0: off; PT_DRAIN_DUMP overrides)
    int drain_dump_tail;                // the same for a tail launch that hands on again (PT_DRAIN_DUMP_TAIL)
    int tail_rpl;                       // tail launches: waves beyond ceil(records / (64 * tail_rpl)) exit at
                                        // once, so each lane resumes about tail_rpl records (PT_TAIL_RPL; 1 =
                                        // one wave per 64 records)
    int tail_refill;                    // a tail wave claims more records once this many lanes are idle
    int allphase_lanes;                 // k_trace_gf: every step kind each iteration once the rays are claimed
                                        // and at most this many lanes trace (PT_ALLPHASE_LANES; 0 = off)
    int defer_launch;                   // 0: k_trace_deferred is not launched (PT_DEFER_LAUNCH=0, timing
                                        // experiments); k_scan then counts a trace fault if any ray was deferred
    unsigned trace_iter_cap;            // persistent traces give up after this many loop iterations (a fault,
                                        // counted in segments[kTraceFaultCounter]); PT_TRACE_ITER_CAP overrides
    int* slot_src;                      // ray sort: dense slot -> source index, written by k_sort_scatter for the
                                        // shading pass of the same bounce; null: the pass searches blk_off
                                        // (PT_SLOT_MAP=0, and every bounce whose trace ran unsorted).  After the
                                        // fields the trace kernels read, so those keep their argument offsets
    const CameraRec* camera;            // setCamera: the free camera camera_ray and k_gen_camera read; null: the
                                        // config's legacy camera (cam_*, plane_*, step_*).  Last, for the same reason
    const EnvRec* env;                  // setEnvironment: the map shade_mat reads for a ray that misses; null: the
                                        // reference's constant 0.01.  Last, for the same reason
    const TriShade* smooth;             // the shading table (one record per scene triangle) of a scene with a
                                        // smooth model; null: every hit normal is the flat one and nothing
                                        // more is loaded.  Static per allocation.  Last, for the same reason
    const float4* tex;                  // the albedo textures of a scene with a textured model: one TexRec per
                                        // model, then every texture's texels, a float4 each (rgb, w unused);
                                        // null: a hit's albedo is its model's colour and nothing more is loaded.
                                        // With it, `smooth` is set too (the table carries the vertex uvs).
                                        // Static per allocation.  Last, for the same reason
    float4* cache_albedo;               // with tex: the albedo of each pixel's cached primary hit (k_primary),
                                        // which bounce 0 multiplies by instead of ModelShade::color; else null
    const ModelShade* glass;            // `shade` again in a scene with a MAT_DIELECTRIC model, else null: it picks
                                        // the hit-buffer pass's GLASS forms at launch.  Static per allocation.  Last,
                                        // for the same reason
};

// denoise(): the largest a-trous step whose pass stages its tile in LDS (PT_DENOISE_LDS overrides)
constexpr int kDenoiseLdsDefault = 4;
constexpr int kMaxBounceCounters = 64;
constexpr int kDrainLevels = 4;          // most tail launches per trace (drain continuations)
constexpr int kDiagCounters = 96;        // diagnostic counters after the per-bounce ones (PT_TRACE_STATS builds)
// segments[] slot counting persistent-trace waves that hit trace_iter_cap and left
// rays untraced (their hit records are stale): any non-zero value invalidates the image
constexpr int kTraceFaultCounter = 7 + kMaxBounceCounters;
// segments[] slot counting rays k_trace_deferred traced (grid_fast hit sets that
// outgrew the overflow pool, or walks past the hand-on records' room); every build
constexpr int kDeferredRayCounter = 50 + kMaxBounceCounters;

struct KernelStats {
    double bounce_ms = 0, scan_ms = 0, primary_ms = 0, first_ms = 0, trace_ms = 0;
    double sort_ms = 0;                  // ray sort before each persistent trace (k_sort_hist/prefix/scatter)
    long long sort_launches = 0;
    long long bounce_launches = 0, scan_launches = 0, first_launches = 0;   // bounce_* = secondary bounces
    long long trace_launches = 0;        // k_trace_bvh (split trace/shade); bounce_* is then the shading pass
};

class Renderer {
public:
    explicit Renderer(const RenderConfig& cfg);
    ~Renderer();
    int allocateOnGPU(const Scene& scene);          // Renderer.cpp:65-130
    int clearImage();                                // initImageKernel (Renderer.cpp:557-565)
    int renderLoop(int first_iter, int n_iters);     // Renderer.cpp:567-648 (asynchronous)
    int renderImage(const std::string& path, int iterations_total);  // Renderer.cpp:15-63
    int readImage(float* host_rgb);
    int synchronize();
    void free();                                     // Renderer.cpp:132-148

    int setStream(hipStream_t s);
    int bindImage(float* device_rgb);
    int setProfiling(int on);              // 0 off, 1 every kernel group, 2 pipeline 0's trace phases
    int kernelStats(KernelStats* out);
    long long segments();
    long long traceFaults();                         // waves that gave up (see kTraceFaultCounter); -1 on error
    int pipelines() const { return npipes; }
    int segmentsPerBounce(long long* out, int n);
    int primaryHits(float* dist, float* normal, int* model);
    int intersectRays(int n, const float* orig, const float* dir, float* dist, float* normal, int* model);
    // test hook (grid_fast): walk certificates vs the exact walk on the same hit sets; 4 ints per ray
    int certifyCheck(int n, const float* orig, const float* dir, int* out4);
    // test hook (split bvh / grid_fast): the caller's rays as bounce 0's survivors in pipeline 0's
    // pool (block_counts: survivors per source block, null = dense), then bounce 1's k_scan / sort /
    // persistent-trace launches over them; per ray the hit record the shading pass would read
    int traceRays(int n, const float* orig, const float* dir, const int* block_counts, int n_blocks,
                  float* dist, float* normal, int* model, int* tri);
    // film.hip: per-pixel second moment of the contributions, the noise estimate read from it
    // and render-until-converged (no counterpart in the reference)
    int enableMoments(float* device_m2);             // before allocateOnGPU; null: own buffer
    int readMoments(float* host_m2);
    int noise(int samples, double* mean_err, float* max_tile_err, float* tile_err_host);
    int renderUntil(int first_iter, int min_iters, int max_iters, int check_every, double target,
                    int* iters_done, double* mean_err);
    int noiseTilesX() const { return (cfg.width + PT_NOISE_TILE - 1) / PT_NOISE_TILE; }
    int noiseTilesY() const { return (cfg.height + PT_NOISE_TILE - 1) / PT_NOISE_TILE; }
    // film.hip: variance-guided edge-avoiding denoiser of the accumulated image (no counterpart
    // in the reference); the image and the moments are read only
    int denoise(int samples, int passes, float sigma_l, float sigma_z, float* device_rgb_out, float* host_rgb,
                float* host_var);
    // denoise with options (pt_renderer_denoise_ex): PT_DENOISE_DEMODULATE filters the image divided by the
    // primary hit's sqrt-space albedo and multiplies it back afterwards; PT_DENOISE_TILE_COUNTS divides by
    // each tile's own sample count, so an image of masked or adaptive iterations can be filtered.  flags 0 is denoise
    int denoiseEx(int samples, int passes, float sigma_l, float sigma_z, int flags, float* device_rgb_out,
                  float* host_rgb, float* host_var);
    int renderImageDenoised(const std::string& path, int samples, int passes, float sigma_l, float sigma_z,
                            int flags = 0);
    int denoiseTimes(double* ms, int n);             // HIP-event times of the last denoise call under setProfiling
    // Tile-masked sampling and the adaptive render (no counterpart in the reference): iterations whose
    // first bounce emits only the rays of the active 16 x 16 tiles, per-tile sample counts, the estimate
    // and the mean that divide by them, and the loop that switches converged tiles off
    int renderLoopMasked(int first_iter, int n_iters, const unsigned char* tile_mask_host);
    int sampleCounts(int* tile_counts_host);         // returns the tile count
    int adaptiveNoise(double* mean_err, float* max_tile_err, float* tile_err_host);
    int adaptiveMean(float* device_rgb_out, float* host_rgb);
    int renderImageAdaptive(const std::string& path);
    int renderAdaptive(int first_iter, int min_iters, int max_iters, int check_every, double tile_target,
                       int* iters_done, long long* pixel_samples, double* mean_err);
    // Pixel-jittered camera rays (anti-aliasing; no counterpart in the reference): while on, every
    // iteration enqueued generates its camera rays through a per-(iteration, pixel) point of the
    // pixel (k_gen_jitter) and traces them as bounce 1.  Host state; before or after allocateOnGPU
    int setPixelJitter(int on, float width);
    int pixelJitter(int* on, float* width) const;
    // Free camera with a thin lens (no counterpart in the reference): null = the config's legacy
    // camera.  A pinhole with the jitter off renders through the ordinary loop (camera_ray takes the
    // general form); a lens or the jitter generates the rays (k_gen_camera) and traces them as bounce
    // 1.  Before or after allocateOnGPU; after it, a new view starts a new render
    int setCamera(const CameraRec* cam);
    int camera(CameraRec* out) const;                // 1: a camera is set; 0: legacy (out = its equivalent)
    // Environment lighting (film.hip, pt_env.h; no counterpart in the reference): the colour of a ray
    // that misses, from an octahedral map of n * n RGB texels.  Null = the constant 0.01.  Before or
    // after allocateOnGPU; after it, a new environment starts a new render (the primary hits stay)
    int setEnvironment(const pt_environment* env);
    // 1: set, 0: none.  out: n, scale and rotation (texels_rgb null); texels_out: n * n * 3 floats
    int environment(pt_environment* out, float* texels_out) const;
    int envLookup(int count, const float* dirs, float* rgb_out);     // test hook: env_radiance of each direction
    int primaryAlbedo(float* rgb_out);   // W*H*3: the albedo of each pixel's cached primary hit, 0 for a miss
    // test hook: the albedo definition evaluated on the device for caller-given hits
    int hitAlbedo(int n, const float* orig, const float* dir, const float* dist, const int* model, const int* tri,
                  float* rgb_out);
    // Sampled first-hit guides (film.hip; no counterpart in the reference): per pixel the sums G of
    // the first hit's (normal, depth, sqrt albedo, hit flag) over the generated (jittered or lens)
    // iterations, accumulated beside the image and the moments; PT_DENOISE_SAMPLED_GUIDES makes the
    // denoiser's prep read their means in place of the primary-hit cache
    int enableGuides(float* device_g);               // before allocateOnGPU; null: own buffer
    int readGuides(float* host_g);                   // W*H*8 floats
    int guideCounts(int* tile_counts_host);          // returns the tile count
    // Direct lighting (no counterpart in the reference): while on, every MAT_DIFFUSE hit of a live
    // ray samples one point of one EMISSIVE triangle and traces a shadow ray (k_direct), and an
    // EMISSIVE hit directly after a DIFFUSE vertex counts nothing.  Before or after allocateOnGPU;
    // a change after it starts a new render.  Needs moments, the split trace and max_bounces <= 63
    int setDirectLight(int on);
    int directLight(int* on, int* n_lights, float* area) const;
    // the allocation's light table: kLightFloats floats per light (Scene::lightTable); returns the count
    int lights(float* recs_out, int max_lights) const;
    // test hooks: segment visibility (1: occluded) and the light sample of caller-given hits
    int occludedSegments(int n, const float* orig, const float* target, int* out);
    int directSample(int n, const float* orig, const float* dir, const float* dist, const int* model, const int* tri,
                     const float* color, const int* ids, float* out_f, int* out_i);

    RenderConfig cfg;
    std::string last_error;

private:
    int launchPrimary();
    void launchTrace(const KParams& k, hipStream_t st, int b);
    int enqueueSortTrace(const KParams& k, hipStream_t st, int b, bool pall, bool ptrace, bool host_rays);
    void launchBounce(const KParams& k, hipStream_t st, bool first, dim3 grid, int iter, int b, int accel);
    int allocPipe(KParams& k, size_t cap, hipStream_t st);
    int fail(hipError_t e, const char* what);
    void freeBuffers();
    int enqueueIteration(int q, hipStream_t st, int iter, int passes, const unsigned char* tile_mask = nullptr,
                         bool jitter = false);
    void launchGenJitter(const KParams& k, hipStream_t st, int iter, const unsigned char* tile_mask);
    void launchGenCamera(const KParams& k, hipStream_t st, int iter, const unsigned char* tile_mask);
    int renderIters(int first_iter, int n_iters, const unsigned char* tile_mask, int* done_out);
    void launchBounceMasked(const KParams& k, hipStream_t st, dim3 grid, int iter, const unsigned char* tile_mask);
    int allocAdaptive();
    void freeAdaptive();
    int uploadTileCounts();
    bool countsUniform() const;
    int refuseMixedCounts(const char* call);
    void dropGraphs();
    int joinPipes(int np);
    int checkFaults();
    int allocMoments();
    int launchMergeM2(const KParams& k, hipStream_t st);
    int allocGuides();
    bool splitTraceWanted() const;
    // the iterations enqueued now generate their camera rays (k_gen_jitter / k_gen_camera)
    bool generatedIterations() const { return jitter_on || (camera_on && cam_rec.lens_radius > 0.0f); }
    int launchGuideFirst(const KParams& k, int q, hipStream_t st);
    int launchMergeGuides(int q, hipStream_t st, const unsigned char* tile_mask);
    int allocDenoise();
    int directRefusal(bool need_moments);              // direct lighting cannot run as configured: last_error says why
    int ensureDirect();                  // the device table and the per-pipeline state, once per allocation
    bool directActive() const { return direct_on && direct_ready; }
    int launchDirect(const KParams& k, int q, hipStream_t st, bool first, int iter, int b, const unsigned char* tile_mask);
    int launchDirectResolve(int q, hipStream_t st);
    int writeBmp(const std::string& path, const float* rgb, float div);     // Renderer.cpp:15-63

    KParams kp{};                   // pipeline 0 (and everything the pipelines share)
    hipStream_t stream = nullptr;    // the caller's stream; pipeline 0 runs on it
    static constexpr int kMaxPipes = 32;
    int npipes = 1;
    KParams pk[kMaxPipes]{};         // pipeline i's parameters (pk[0] == kp)
    hipStream_t pstream[kMaxPipes]{};    // pstream[0] == stream; 1.. created here
    hipEvent_t merge_ev[kMaxPipes]{};    // last k_merge recorded on each pipeline
    hipEvent_t fork_ev = nullptr;
    hipGraphExec_t gexec[kMaxPipes]{};   // PT_GRAPH: pipeline i's bounce loop captured once, replayed per iteration
    bool use_graph = false;
    bool own_stream = false;
    bool stream_set = false;
    bool allocated = false;
    bool cache_valid = false;        // is_first_intersection_cached (Renderer.cpp:580)
    int alloc_ntris = 0;             // the allocation's scene triangle count (hitAlbedo's range check)
    std::vector<float> alloc_color;  // the allocation's model colours, 3 per model (primaryAlbedo without textures)
    size_t tex_bytes = 0;            // bytes the allocation uploaded for textures (texels, records, shading table)
    bool external_image = false;
    float* ext_image = nullptr;
    bool moments_on = false;         // enableMoments: every pipeline has a contribution buffer, k_merge_m2 merges
    float* ext_m2 = nullptr;         // the caller's moment buffer (null: allocated here)
    float* m2 = nullptr;             // W*H*3 sums of squared contributions
    bool guides_on = false;          // enableGuides: generated iterations accumulate first-hit guides
    float* ext_guides = nullptr;     // the caller's guide buffer (null: allocated here)
    float* guides = nullptr;         // W*H*8 sums G
    float* guide_contrib[kMaxPipes]{};   // pipeline i's per-iteration records (k_guide_first -> k_merge_guides)
    std::vector<int> guide_tile_counts;  // generated samples per noise tile since allocateOnGPU / clearImage (host)
    bool direct_on = false;              // setDirectLight
    bool direct_ready = false;           // the allocation has lights and their device state exists
    bool direct_textured = false;        // the allocation's scene has a textured EMISSIVE model (refused)
    std::vector<float> light_recs;       // the allocation's light table (host), kLightFloats floats per light
    double light_area = 0.0;             // A_total
    float4* lights_dev = nullptr;
    float* direct_D[kMaxPipes]{};        // pipeline i's direct light of the iteration in flight, 3 floats per pixel
    unsigned char* direct_flags[kMaxPipes]{};    // ... and its flag byte per pixel
    double* noise_sum = nullptr;     // noise(): per-tile sums, then the mean
    float* noise_err = nullptr;      // per-tile errors, then the largest
    int samples_accumulated = 0;     // iterations enqueued since allocateOnGPU / clearImage
    float4* dn_cv[2] = {};           // denoise(): per pixel (c.rgb, V), ping-pong; allocated by the first call
    float4* dn_nd = nullptr;         // (n.xyz, d) of the primary hit
    int* dn_model = nullptr;         // its model (-1: miss or dropped by tail_drop)
    float* dn_slope = nullptr;       // depth slope
    std::vector<hipEvent_t> dn_events;   // profiling: around prep, each pass and the output copy
    int dn_event_passes = 0;
    bool dn_event_remod = false;         // ... and the remodulation (PT_DENOISE_DEMODULATE)
    std::vector<int> tile_counts;        // samples per noise tile since allocateOnGPU / clearImage (host)
    static constexpr int kMaskSlots = 4;     // masked calls whose mask copy may be in flight at once
    unsigned char* tile_mask_dev = nullptr;  // the mask the enqueued masked iterations read; set by the first masked call
    unsigned char* mask_stage = nullptr;     // pinned host staging, kMaskSlots masks
    hipEvent_t mask_ev[kMaskSlots]{};        // slot i's upload has completed
    int mask_slot = 0;
    bool jitter_on = false;              // setPixelJitter: the iterations enqueued from now on are jittered
    float jitter_width = 1.0f;           // ... over this many pixels about the pixel's corner
    bool camera_on = false;              // setCamera: cam_rec holds the view; kp.camera / pk[].camera point at cam_dev
    CameraRec cam_rec{};
    CameraRec* cam_dev = nullptr;        // the device record (allocateOnGPU)
    bool env_on = false;                 // setEnvironment: kp.env / pk[].env point at env_dev
    EnvRec env_rec{};                    // n, scale, rot (texels: env_texels_dev once allocated)
    std::vector<float4> env_texels;      // the host copy, one float4 per texel
    EnvRec* env_dev = nullptr;           // the device record (allocateOnGPU)
    float4* env_texels_dev = nullptr;    // the device texels and how many fit
    size_t env_texels_cap = 0;
    int uploadEnvironment();
    bool slot_map = true;                // k_sort_scatter writes KParams::slot_src for the shading pass (PT_SLOT_MAP)
    bool jitter_sort1 = false;           // ray sort before a jittered iteration's bounce-1 trace too (PT_JITTER_SORT=1)
    int* tile_counts_dev = nullptr;      // adaptiveNoise / adaptiveMean: the counts, uploaded per call
    float* am_out = nullptr;             // adaptiveMean's result when the caller gives no device buffer
    int profiling = 0;
    std::vector<void*> allocs;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> bounce_events, first_events, scan_events, trace_events, sort_events;
    bool split_trace = false;        // persistent k_trace_bvh / k_trace_gf + shading pass
    int trace_blocks = 0;
    int tail_blocks = 0;             // grid of k_trace_gf's tail launches (PT_TAIL_BLOCKS; default trace_blocks)
    int gf_flags = 9;                // k_trace_gf variant: 1 LDS model records, 8 phase scheduling
    bool gf_wide_lds = false;        // k_trace_gf default variants with 9..12 models: 12 LDS records (F | 32)
    bool bvh_wide_lds = false;       // k_trace_bvh default variant with 9..12 models: 12 LDS records (F = 43)
    KernelStats stats;
};

// Device math conformance hook (pt_selftest_math).
int selftest_math(int n, const float* x, const float* y, float* out, std::string* err);
// Device conformance hook of the dielectric material (pt_selftest_dielectric).
int selftest_dielectric(int n, const float* dir, const float* nrm, const float* ior, const float* u, float* out_dir,
                        int* out_event, std::string* err);

}  // namespace pt
