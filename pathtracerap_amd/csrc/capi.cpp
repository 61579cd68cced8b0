// capi.cpp -- extern "C" boundary (include/pathtracer_amd.h).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pathtracer_amd.h"
#include "renderer.h"
#include "scene.h"

// bvh_mu: pt_renderer_allocate_on_gpu may add the BLAS to a scene built grid-only;
// renderers allocating from one shared scene on several threads (ctypes drops the
// GIL) take turns there, and only the first one builds
struct pt_scene { pt::Scene s; std::mutex bvh_mu; };
struct pt_renderer { pt::Renderer* r; };

static thread_local std::string g_err;

// Iterations in flight run on their own HIP streams (pt_render_config.pipelines,
// default 16); HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues (default
// 4), so with the default several pipelines share a queue and serialise
// (DESIGN.md "Results": 8 pipelines on 4 queues ran 1570 Mrays/s at configs[1]).  The variable is read once, when
// the HIP runtime initialises: set it at load time unless the process already
// chose a value.  (A process whose HIP runtime started before this library was
// loaded keeps its own setting.)
// What the process had chosen is recorded (pt_hw_queue_info), so a host can
// report the queue count in effect or warn when it differs from the default.
static int g_queues_at_load = -1;        // GPU_MAX_HW_QUEUES when the library loaded (-1: unset)
static int g_queues_set_by_lib = 0;      // 1: the library set it (the process had not)
__attribute__((constructor)) static void pt_default_hw_queues() {
    const char* e = std::getenv("GPU_MAX_HW_QUEUES");
    if (e) {
        g_queues_at_load = std::atoi(e);
    } else {
        setenv("GPU_MAX_HW_QUEUES", "16", /*overwrite=*/0);
        g_queues_set_by_lib = 1;
    }
}

static int set_err(const std::string& m) { g_err = m; return -1; }

extern "C" {

int pt_abi_version(void) { return PT_ABI_VERSION; }

int pt_hw_queue_info(int* at_load, int* set_by_library) {
    if (at_load) *at_load = g_queues_at_load;
    if (set_by_library) *set_by_library = g_queues_set_by_lib;
    return 0;
}
const char* pt_last_error(void) { return g_err.c_str(); }

void pt_default_config(pt_render_config* c) {
    pt::RenderConfig d;
    c->width = d.width; c->height = d.height; c->iterations = d.iterations; c->max_bounces = d.max_bounces;
    c->accel = d.accel;
    for (int k = 0; k < 3; k++) { c->grid[k] = d.grid[k]; c->cam[k] = d.cam[k]; }
    c->tail_drop = d.tail_drop;
    c->plane_z = d.plane_z; c->plane_x0 = d.plane_x0; c->plane_y0 = d.plane_y0;
    c->plane_w = d.plane_w; c->plane_h = d.plane_h;
    c->block = d.block;
    c->pipelines = d.pipelines;
    c->ray_sort = d.ray_sort;
}

static pt::RenderConfig to_cfg(const pt_render_config* c) {
    pt::RenderConfig d;
    d.width = c->width; d.height = c->height; d.iterations = c->iterations; d.max_bounces = c->max_bounces;
    d.accel = c->accel;
    for (int k = 0; k < 3; k++) { d.grid[k] = c->grid[k]; d.cam[k] = c->cam[k]; }
    d.tail_drop = c->tail_drop;
    d.plane_z = c->plane_z; d.plane_x0 = c->plane_x0; d.plane_y0 = c->plane_y0;
    d.plane_w = c->plane_w; d.plane_h = c->plane_h;
    d.block = c->block;
    d.pipelines = c->pipelines;
    d.ray_sort = c->ray_sort;
    return d;
}

pt_scene* pt_scene_create(void) {
    try { return new pt_scene(); } catch (...) { set_err("out of memory"); return nullptr; }
}
void pt_scene_destroy(pt_scene* s) { delete s; }

#define SCENE_CALL(expr)                                  \
    do {                                                  \
        if (!s) return set_err("null scene");             \
        try {                                             \
            int _rc = (expr);                             \
            if (_rc < 0) return set_err(s->s.last_error); \
            return _rc;                                   \
        } catch (const std::exception& e) {               \
            return set_err(e.what());                     \
        }                                                 \
    } while (0)

int pt_scene_load_config(pt_scene* s, const char* path) { SCENE_CALL(s->s.loadConfig(path ? path : "")); }

int pt_scene_apply_settings(const pt_scene* s, pt_render_config* c) {
    if (!s || !c) return set_err("null argument");
    const pt::RenderSettings& st = s->s.settings;
    if (st.has_width) { c->width = st.width; c->height = st.height; }
    if (st.has_iterations) c->iterations = st.iterations;
    if (st.has_bounces) c->max_bounces = st.max_bounces;
    if (st.has_accel) c->accel = st.accel;
    for (int k = 0; k < 3; k++) c->grid[k] = st.grid[k];
    return 0;
}

int pt_scene_load_obj(pt_scene* s, const char* path) { SCENE_CALL(s->s.loadObj(path ? path : "")); }

int pt_scene_add_mesh(pt_scene* s, const float* pos, const float* nrm, int nv, const int* tris, int nt) {
    if (!pos || !nrm || !tris || nv < 0 || nt < 0) return set_err("pt_scene_add_mesh: bad arguments");
    SCENE_CALL(s->s.addMesh(pos, nrm, nv, tris, nt));
}

int pt_scene_add_model(pt_scene* s, int mesh, const float scale[3], const float rot[3], const float tr[3],
                       int material, const float color[3]) {
    if (!scale || !rot || !tr || !color) return set_err("pt_scene_add_model: null argument");
    SCENE_CALL(s->s.addModel(mesh, scale, rot, tr, material, color));
}

int pt_scene_set_model_smooth(pt_scene* s, int model, int on) { SCENE_CALL(s->s.setModelSmooth(model, on != 0)); }

int pt_scene_model_smooth(const pt_scene* s, int model) {
    if (!s) return set_err("null scene");
    const int rc = s->s.modelSmooth(model);
    return rc < 0 ? set_err("pt_scene_model_smooth: bad model index") : rc;
}

int pt_scene_set_model_ior(pt_scene* s, int model, float ior) { SCENE_CALL(s->s.setModelIor(model, ior)); }

float pt_scene_model_ior(const pt_scene* s, int model) {
    if (!s) { set_err("null scene"); return -1.0f; }
    const float v = s->s.modelIor(model);
    if (v < 0.0f) set_err("pt_scene_model_ior: bad model index");
    return v;
}

int pt_scene_set_mesh_uv(pt_scene* s, int mesh, const float* uv, int nv) {
    if (!uv) return set_err("pt_scene_set_mesh_uv: null argument");
    SCENE_CALL(s->s.setMeshUv(mesh, uv, nv));
}

int pt_scene_export_uv(const pt_scene* s, float* uv_out) {
    if (!s) return set_err("null scene");
    const pt::Scene& S = s->s;
    if (uv_out)
        for (size_t i = 0; i < S.vertices.size() * 2; i++) uv_out[i] = i < S.vertex_uv.size() ? S.vertex_uv[i] : 0.0f;
    return (int)S.vertices.size();
}

int pt_scene_mesh_has_uv(const pt_scene* s, int mesh) {
    if (!s) return set_err("null scene");
    const int rc = s->s.meshHasUv(mesh);
    return rc < 0 ? set_err("pt_scene_mesh_has_uv: bad mesh index") : rc;
}

int pt_scene_add_texture(pt_scene* s, int w, int h, const float* rgb) {
    if (!rgb) return set_err("pt_scene_add_texture: null argument");
    SCENE_CALL(s->s.addTexture(w, h, rgb));
}

int pt_scene_set_model_texture(pt_scene* s, int model, int texture) { SCENE_CALL(s->s.setModelTexture(model, texture)); }

int pt_scene_model_texture(const pt_scene* s, int model) {
    if (!s) return set_err("null scene");
    int t = -1;
    if (s->s.modelTexture(model, &t) < 0) { set_err("pt_scene_model_texture: bad model index"); return -2; }
    return t;
}

int pt_scene_texture_count(const pt_scene* s) {
    if (!s) return set_err("null scene");
    return (int)s->s.textures.size();
}

int pt_scene_texture(const pt_scene* s, int texture, int* w, int* h, float* rgb_out) {
    if (!s) return set_err("null scene");
    if (texture < 0 || texture >= (int)s->s.textures.size()) return set_err("pt_scene_texture: bad texture index");
    const pt::Texture& t = s->s.textures[texture];
    if (w) *w = t.w;
    if (h) *h = t.h;
    if (rgb_out) std::memcpy(rgb_out, t.rgb.data(), t.rgb.size() * sizeof(float));
    return 0;
}

int pt_scene_build(pt_scene* s, const int grid[3], int with_bvh) {
    const int def[3] = {25, 25, 25};
    SCENE_CALL(s->s.build(grid ? grid : def, with_bvh != 0));
}

int pt_scene_counts(const pt_scene* s, int c[9]) {
    if (!s || !c) return set_err("null argument");
    const pt::Scene& S = s->s;
    c[0] = (int)S.vertices.size(); c[1] = (int)S.triangles.size(); c[2] = (int)S.meshes.size();
    c[3] = (int)S.models.size(); c[4] = (int)S.grids.size(); c[5] = (int)S.voxels.size();
    c[6] = (int)S.per_voxel_data_pool.size(); c[7] = (int)S.bvh_nodes.size(); c[8] = (int)S.bvh_tri_order.size();
    return 0;
}

int pt_scene_export(const pt_scene* s, float* vpos, float* vnrm, int* tris, int* mesh_ranges, float* mesh_bbox,
                    int* model_ints, float* m2w, float* w2m, float* color, int* grid_ints, float* grid_vw,
                    int* vox, int* per_voxel) {
    if (!s) return set_err("null scene");
    const pt::Scene& S = s->s;
    for (size_t i = 0; i < S.vertices.size(); i++) {
        const pt::Vertex& v = S.vertices[i];
        if (vpos) { vpos[3 * i] = v.position.x; vpos[3 * i + 1] = v.position.y; vpos[3 * i + 2] = v.position.z; }
        if (vnrm) { vnrm[3 * i] = v.normal.x; vnrm[3 * i + 1] = v.normal.y; vnrm[3 * i + 2] = v.normal.z; }
    }
    if (tris) for (size_t i = 0; i < S.triangles.size(); i++) std::memcpy(tris + 3 * i, S.triangles[i].vertex_indices, 12);
    for (size_t i = 0; i < S.meshes.size(); i++) {
        const pt::Mesh& m = S.meshes[i];
        if (mesh_ranges) {
            mesh_ranges[4 * i] = m.vertex_indices.start_index; mesh_ranges[4 * i + 1] = m.vertex_indices.end_index;
            mesh_ranges[4 * i + 2] = m.triangle_indices.start_index; mesh_ranges[4 * i + 3] = m.triangle_indices.end_index;
        }
        if (mesh_bbox) {
            const pt::BoundingBox& b = m.bounding_box;
            const float v[6] = {b.min.x, b.min.y, b.min.z, b.max.x, b.max.y, b.max.z};
            std::memcpy(mesh_bbox + 6 * i, v, 24);
        }
    }
    for (size_t i = 0; i < S.models.size(); i++) {
        const pt::Model& m = S.models[i];
        if (model_ints) { model_ints[3 * i] = m.mesh_index; model_ints[3 * i + 1] = m.grid_index; model_ints[3 * i + 2] = m.mat.material_type; }
        if (m2w) std::memcpy(m2w + 16 * i, m.model_to_world, 64);
        if (w2m) std::memcpy(w2m + 16 * i, m.world_to_model, 64);
        if (color) std::memcpy(color + 3 * i, m.mat.color, 12);
    }
    for (size_t i = 0; i < S.grids.size(); i++) {
        const pt::Grid& g = S.grids[i];
        if (grid_ints) {
            grid_ints[4 * i] = g.voxelIndices.start_index; grid_ints[4 * i + 1] = g.voxelIndices.end_index;
            grid_ints[4 * i + 2] = g.entity_type; grid_ints[4 * i + 3] = g.entity_index;
        }
        if (grid_vw) std::memcpy(grid_vw + 3 * i, g.voxel_width, 12);
    }
    if (vox)
        for (size_t i = 0; i < S.voxels.size(); i++) {
            vox[3 * i] = S.voxels[i].entity_index_range.start_index;
            vox[3 * i + 1] = S.voxels[i].entity_index_range.end_index;
            vox[3 * i + 2] = S.voxels[i].entity_type;
        }
    if (per_voxel && !S.per_voxel_data_pool.empty())
        std::memcpy(per_voxel, S.per_voxel_data_pool.data(), S.per_voxel_data_pool.size() * sizeof(int));
    return 0;
}

int pt_scene_export_bvh(const pt_scene* s, float* nodes, int* refs, int* roots) {
    if (!s) return set_err("null scene");
    const pt::Scene& S = s->s;
    if (nodes && !S.bvh_nodes.empty()) std::memcpy(nodes, S.bvh_nodes.data(), S.bvh_nodes.size() * sizeof(pt::BvhNode));
    if (refs && !S.bvh_tri_order.empty()) std::memcpy(refs, S.bvh_tri_order.data(), S.bvh_tri_order.size() * sizeof(int));
    if (roots)
        for (size_t i = 0; i < S.meshes.size(); i++) roots[i] = S.mesh_bvh_root.empty() ? -1 : S.mesh_bvh_root[i];
    return 0;
}

int pt_scene_export_bvh4(const pt_scene* s, float* nodes, int* roots) {
    if (!s) return set_err("null scene");
    const pt::Scene& S = s->s;
    if (nodes && !S.bvh4_nodes.empty()) std::memcpy(nodes, S.bvh4_nodes.data(), S.bvh4_nodes.size() * sizeof(pt::Bvh4Node));
    if (roots)
        for (size_t i = 0; i < S.meshes.size(); i++) roots[i] = S.mesh_bvh4_root.empty() ? -1 : S.mesh_bvh4_root[i];
    return (int)S.bvh4_nodes.size();
}

int pt_scene_export_bvh4_leaf_base(const pt_scene* s, int* bases) {
    if (!s) return set_err("null scene");
    const pt::Scene& S = s->s;
    if (bases)
        for (size_t i = 0; i < S.meshes.size(); i++) bases[i] = S.mesh_leaf_base.empty() ? 0 : S.mesh_leaf_base[i];
    return (int)S.meshes.size();
}

pt_renderer* pt_renderer_create(const pt_render_config* c) {
    if (!c) { set_err("null config"); return nullptr; }
    if (c->accel != PT_ACCEL_GRID && c->accel != PT_ACCEL_BVH && c->accel != PT_ACCEL_GRID_FAST) {
        set_err("bad accel");
        return nullptr;
    }
    // block: 64, 128 or 256; any other value falls back to 256 (Renderer::allocateOnGPU, kp.chunk)
    try {
        pt_renderer* r = new pt_renderer();
        r->r = new pt::Renderer(to_cfg(c));
        return r;
    } catch (...) {
        set_err("out of memory");
        return nullptr;
    }
}

#define R_CALL(expr)                                     \
    do {                                                 \
        if (!r || !r->r) return set_err("null renderer"); \
        int _rc = (expr);                                \
        if (_rc < 0) return set_err(r->r->last_error);   \
        return _rc;                                      \
    } while (0)

int pt_renderer_set_stream(pt_renderer* r, void* st) { R_CALL(r->r->setStream((hipStream_t)st)); }
int pt_renderer_bind_image(pt_renderer* r, float* d) { R_CALL(r->r->bindImage(d)); }
int pt_renderer_allocate_on_gpu(pt_renderer* r, const pt_scene* s) {
    if (!s) return set_err("null scene");
    if (!r || !r->r) return set_err("null renderer");
    // grid_fast / bvh traverse the per-mesh BLAS: a scene built grid-only gets it here,
    // once (the scene's grid tables are rebuilt identically alongside); the lock also
    // keeps other renderers from reading the scene while that happens
    pt_scene* ms = const_cast<pt_scene*>(s);
    std::lock_guard<std::mutex> lock(ms->bvh_mu);
    if (r->r->cfg.accel != PT_ACCEL_GRID && ms->s.built && ms->s.bvh_nodes.empty() && ms->s.ensureBvh() < 0)
        return set_err(ms->s.last_error);
    R_CALL(r->r->allocateOnGPU(s->s));
}
int pt_renderer_clear_image(pt_renderer* r) { R_CALL(r->r->clearImage()); }
int pt_renderer_render_loop(pt_renderer* r, int first, int n) { R_CALL(r->r->renderLoop(first, n)); }
int pt_renderer_synchronize(pt_renderer* r) { R_CALL(r->r->synchronize()); }
int pt_renderer_read_image(pt_renderer* r, float* h) {
    if (!h) return set_err("null buffer");
    R_CALL(r->r->readImage(h));
}
int pt_renderer_render_image(pt_renderer* r, const char* path, int iters) {
    if (!path || iters <= 0) return set_err("bad arguments");
    R_CALL(r->r->renderImage(path, iters));
}
long long pt_renderer_segments(pt_renderer* r) {
    if (!r || !r->r) { set_err("null renderer"); return -1; }
    return r->r->segments();
}
long long pt_renderer_trace_faults(pt_renderer* r) {
    if (!r || !r->r) { set_err("null renderer"); return -1; }
    const long long f = r->r->traceFaults();
    if (f < 0) set_err("reading the trace fault counter failed");
    return f;
}
int pt_renderer_segments_per_bounce(pt_renderer* r, long long* out, int n) {
    if (!out || n < 0) return set_err("bad arguments");
    R_CALL(r->r->segmentsPerBounce(out, n));
}
int pt_renderer_pipelines(pt_renderer* r) {
    if (!r || !r->r) return set_err("null renderer");
    return r->r->pipelines();
}
int pt_renderer_set_profiling(pt_renderer* r, int on) { R_CALL(r->r->setProfiling(on)); }
int pt_renderer_kernel_stats(pt_renderer* r, double st[7]) {
    if (!r || !r->r || !st) return set_err("null argument");
    pt::KernelStats k;
    if (r->r->kernelStats(&k) < 0) return set_err(r->r->last_error);
    st[0] = k.bounce_ms; st[1] = k.scan_ms; st[2] = k.primary_ms;
    st[3] = (double)k.bounce_launches; st[4] = (double)k.scan_launches;
    st[5] = k.first_ms; st[6] = (double)k.first_launches;
    return 0;
}
int pt_renderer_kernel_stats_ex(pt_renderer* r, double* st, int n) {
    if (!r || !r->r || !st || n < 0) return set_err("bad arguments");
    pt::KernelStats k;
    if (r->r->kernelStats(&k) < 0) return set_err(r->r->last_error);
    const double v[11] = {k.bounce_ms, k.scan_ms, k.primary_ms, (double)k.bounce_launches, (double)k.scan_launches,
                          k.first_ms, (double)k.first_launches, k.trace_ms, (double)k.trace_launches,
                          k.sort_ms, (double)k.sort_launches};
    for (int i = 0; i < n; i++) st[i] = i < 11 ? v[i] : 0.0;
    return 0;
}
int pt_renderer_primary_hits(pt_renderer* r, float* d, float* n, int* m) {
    if (!d || !n || !m) return set_err("null buffer");
    R_CALL(r->r->primaryHits(d, n, m));
}
int pt_renderer_intersect_rays(pt_renderer* r, int n, const float* o, const float* d, float* t, float* nn, int* m) {
    if (n < 0 || (n > 0 && (!o || !d || !t || !nn || !m))) return set_err("bad arguments");
    R_CALL(r->r->intersectRays(n, o, d, t, nn, m));
}
int pt_renderer_certify_check(pt_renderer* r, int n, const float* o, const float* d, int* out4) {
    if (n < 0 || (n > 0 && (!o || !d || !out4))) return set_err("bad arguments");
    R_CALL(r->r->certifyCheck(n, o, d, out4));
}
int pt_renderer_trace_rays(pt_renderer* r, int n, const float* o, const float* d, const int* block_counts, int n_blocks,
                           float* t, float* nn, int* m, int* tri) {
    if (n > 0 && (!o || !d || !t || !nn || !m || !tri)) return set_err("bad arguments");
    if (block_counts && n_blocks < 0) return set_err("bad arguments");
    R_CALL(r->r->traceRays(n, o, d, block_counts, n_blocks, t, nn, m, tri));
}
int pt_renderer_enable_moments(pt_renderer* r, float* device_m2) { R_CALL(r->r->enableMoments(device_m2)); }
int pt_renderer_read_moments(pt_renderer* r, float* h) {
    if (!h) return set_err("null buffer");
    R_CALL(r->r->readMoments(h));
}
int pt_renderer_noise(pt_renderer* r, int samples, double* mean_err, float* max_tile_err, float* tile_err_host) {
    R_CALL(r->r->noise(samples, mean_err, max_tile_err, tile_err_host));
}
int pt_renderer_render_until(pt_renderer* r, int first_iter, int min_iters, int max_iters, int check_every,
                             double target, int* iters_done, double* mean_err) {
    R_CALL(r->r->renderUntil(first_iter, min_iters, max_iters, check_every, target, iters_done, mean_err));
}
void pt_default_denoise_params(pt_denoise_params* p) {
    if (!p) return;
    p->passes = 5;
    p->sigma_l = 4.0f;
    p->sigma_z = 1.0f;
}
int pt_renderer_denoise(pt_renderer* r, int samples, const pt_denoise_params* p, float* device_rgb_out, float* host_rgb,
                        float* host_var) {
    pt_denoise_params d;
    pt_default_denoise_params(&d);
    if (p) d = *p;
    R_CALL(r->r->denoise(samples, d.passes, d.sigma_l, d.sigma_z, device_rgb_out, host_rgb, host_var));
}
int pt_renderer_render_image_denoised(pt_renderer* r, const char* path, int samples, const pt_denoise_params* p) {
    if (!path) return set_err("bad arguments");
    pt_denoise_params d;
    pt_default_denoise_params(&d);
    if (p) d = *p;
    R_CALL(r->r->renderImageDenoised(path, samples, d.passes, d.sigma_l, d.sigma_z));
}
int pt_renderer_denoise_ex(pt_renderer* r, int samples, const pt_denoise_params* p, int flags, float* device_rgb_out,
                           float* host_rgb, float* host_var) {
    pt_denoise_params d;
    pt_default_denoise_params(&d);
    if (p) d = *p;
    R_CALL(r->r->denoiseEx(samples, d.passes, d.sigma_l, d.sigma_z, flags, device_rgb_out, host_rgb, host_var));
}
int pt_renderer_render_image_denoised_ex(pt_renderer* r, const char* path, int samples, const pt_denoise_params* p,
                                         int flags) {
    if (!path) return set_err("bad arguments");
    pt_denoise_params d;
    pt_default_denoise_params(&d);
    if (p) d = *p;
    R_CALL(r->r->renderImageDenoised(path, samples, d.passes, d.sigma_l, d.sigma_z, flags));
}
int pt_renderer_denoise_times(pt_renderer* r, double* ms, int n) {
    if (!ms || n < 0) return set_err("bad arguments");
    R_CALL(r->r->denoiseTimes(ms, n));
}
int pt_renderer_enable_guides(pt_renderer* r, void* device_ptr) { R_CALL(r->r->enableGuides((float*)device_ptr)); }
int pt_renderer_read_guides(pt_renderer* r, float* out) {
    if (!out) return set_err("null buffer");
    R_CALL(r->r->readGuides(out));
}
int pt_renderer_guide_counts(pt_renderer* r, int* tiles) { R_CALL(r->r->guideCounts(tiles)); }
int pt_renderer_render_loop_masked(pt_renderer* r, int first_iter, int n_iters, const unsigned char* tile_mask_host) {
    R_CALL(r->r->renderLoopMasked(first_iter, n_iters, tile_mask_host));
}
int pt_renderer_sample_counts(pt_renderer* r, int* tile_counts_host) { R_CALL(r->r->sampleCounts(tile_counts_host)); }
int pt_renderer_adaptive_noise(pt_renderer* r, double* mean_err, float* max_tile_err, float* tile_err_host) {
    R_CALL(r->r->adaptiveNoise(mean_err, max_tile_err, tile_err_host));
}
int pt_renderer_adaptive_mean(pt_renderer* r, void* device_rgb_out, float* host_rgb) {
    R_CALL(r->r->adaptiveMean((float*)device_rgb_out, host_rgb));
}
int pt_renderer_render_image_adaptive(pt_renderer* r, const char* path) {
    if (!path) return set_err("bad arguments");
    R_CALL(r->r->renderImageAdaptive(path));
}
int pt_renderer_render_adaptive(pt_renderer* r, int first_iter, int min_iters, int max_iters, int check_every,
                                double tile_target, int* iters_done, long long* pixel_samples, double* mean_err) {
    R_CALL(r->r->renderAdaptive(first_iter, min_iters, max_iters, check_every, tile_target, iters_done, pixel_samples,
                                mean_err));
}
int pt_renderer_set_pixel_jitter(pt_renderer* r, int on, float width) { R_CALL(r->r->setPixelJitter(on, width)); }
int pt_renderer_pixel_jitter(pt_renderer* r, int* on, float* width) { R_CALL(r->r->pixelJitter(on, width)); }
static_assert(sizeof(pt_camera) == sizeof(pt::CameraRec), "pt_camera and pt::CameraRec share one layout");
int pt_renderer_set_camera(pt_renderer* r, const pt_camera* cam) {
    pt::CameraRec c;
    if (cam) std::memcpy(&c, cam, sizeof c);
    R_CALL(r->r->setCamera(cam ? &c : nullptr));
}
int pt_renderer_camera(pt_renderer* r, pt_camera* out) {
    if (!r || !r->r) return set_err("null renderer");
    pt::CameraRec c;
    const int rc = r->r->camera(&c);
    if (out) std::memcpy(out, &c, sizeof c);
    return rc;
}

int pt_renderer_set_environment(pt_renderer* r, const pt_environment* env) { R_CALL(r->r->setEnvironment(env)); }
int pt_renderer_environment(pt_renderer* r, pt_environment* out, float* texels_out) {
    R_CALL(r->r->environment(out, texels_out));
}
int pt_renderer_env_lookup(pt_renderer* r, int count, const float* dirs, float* rgb_out) {
    R_CALL(r->r->envLookup(count, dirs, rgb_out));
}

int pt_renderer_primary_albedo(pt_renderer* r, float* rgb_out) {
    if (!r || !rgb_out) return set_err("pt_renderer_primary_albedo: null argument");
    R_CALL(r->r->primaryAlbedo(rgb_out));
}

int pt_renderer_hit_albedo(pt_renderer* r, int n, const float* orig, const float* dir, const float* dist,
                           const int* model, const int* tri, float* rgb_out) {
    if (!r || (n > 0 && (!orig || !dir || !dist || !model || !tri || !rgb_out)))
        return set_err("pt_renderer_hit_albedo: null argument");
    R_CALL(r->r->hitAlbedo(n, orig, dir, dist, model, tri, rgb_out));
}

static_assert(PT_LIGHT_FLOATS == pt::kLightFloats, "PT_LIGHT_FLOATS is the light record's size");
int pt_renderer_set_direct_light(pt_renderer* r, int on) { R_CALL(r->r->setDirectLight(on)); }
int pt_renderer_direct_light(pt_renderer* r, int* on, int* n_lights, float* area) {
    R_CALL(r->r->directLight(on, n_lights, area));
}
int pt_scene_lights(const pt_scene* s, int max_lights, float* recs_out, float* area_total) {
    if (!s) return set_err("null scene");
    std::vector<float> recs;
    double area = 0.0;
    const int n = s->s.lightTable(recs, &area, nullptr);
    if (recs_out && max_lights > 0)
        std::memcpy(recs_out, recs.data(), (size_t)(n < max_lights ? n : max_lights) * pt::kLightFloats * sizeof(float));
    if (area_total) *area_total = (float)area;
    return n;
}
int pt_renderer_lights(pt_renderer* r, int max_lights, float* recs_out, float* area_total) {
    if (!r || !r->r) return set_err("null renderer");
    if (area_total) r->r->directLight(nullptr, nullptr, area_total);
    return r->r->lights(recs_out, max_lights);
}
int pt_scene_direct_light(const pt_scene* s) {
    if (!s) return set_err("null scene");
    return s->s.settings.direct_light ? 1 : 0;
}
int pt_renderer_occluded(pt_renderer* r, int n, const float* orig, const float* target, int* out) {
    if (n < 0 || (n > 0 && (!orig || !target || !out))) return set_err("pt_renderer_occluded: bad arguments");
    R_CALL(r->r->occludedSegments(n, orig, target, out));
}
int pt_renderer_direct_sample(pt_renderer* r, int n, const float* orig, const float* dir, const float* dist,
                              const int* model, const int* tri, const float* color, const int* ids, float* out_f,
                              int* out_i) {
    if (n < 0 || (n > 0 && (!orig || !dir || !dist || !model || !tri || !color || !ids || !out_f || !out_i)))
        return set_err("pt_renderer_direct_sample: bad arguments");
    R_CALL(r->r->directSample(n, orig, dir, dist, model, tri, color, ids, out_f, out_i));
}

int pt_environment_sky(const float zenith[3], const float horizon[3], const float ground[3], int n, float* texels_out) {
    if (!zenith || !horizon || !ground || !texels_out) return set_err("environment_sky: null argument");
    if (n < 1 || n > pt::kEnvMaxN) return set_err("environment_sky: n must be 1 .. 2048");
    for (int y = 0; y < n; y++)
        for (int x = 0; x < n; x++) {
            const float px = (((float)x + 0.5f) / (float)n) * 2.0f - 1.0f;
            const float py = (((float)y + 0.5f) / (float)n) * 2.0f - 1.0f;
            const float ez = (1.0f - fabsf(px)) - fabsf(py);
            float ex = px, ey = py;
            if (ez < 0.0f) {
                ex = (1.0f - fabsf(py)) * (px >= 0.0f ? 1.0f : -1.0f);
                ey = (1.0f - fabsf(px)) * (py >= 0.0f ? 1.0f : -1.0f);
            }
            const float uz = pt::normalize(pt::mk3(ex, ey, ez)).z;
            float* t = texels_out + 3 * ((size_t)y * n + x);
            for (int k = 0; k < 3; k++) t[k] = ez >= 0.0f ? horizon[k] + (zenith[k] - horizon[k]) * uz : ground[k];
        }
    return 0;
}

int pt_camera_look_at(const double eye[3], const double target[3], const double up[3], double vfov_deg,
                      double focus_dist, double lens_radius, int W, int H, pt_camera* out) {
    if (!eye || !target || !up || !out) return set_err("look_at: null argument");
    if (W <= 0 || H <= 0) return set_err("look_at: bad resolution");
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(eye[k]) || !std::isfinite(target[k]) || !std::isfinite(up[k]))
            return set_err("look_at: every value must be finite");
    if (!std::isfinite(vfov_deg) || !std::isfinite(focus_dist) || !std::isfinite(lens_radius))
        return set_err("look_at: every value must be finite");
    auto norm = [](const double v[3]) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    auto cross = [](const double a[3], const double b[3], double o[3]) {
        o[0] = a[1] * b[2] - a[2] * b[1];
        o[1] = a[2] * b[0] - a[0] * b[2];
        o[2] = a[0] * b[1] - a[1] * b[0];
    };
    double f[3] = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]};
    const double fl = norm(f);
    if (!(fl > 0.0)) return set_err("look_at: eye and target coincide");
    for (int k = 0; k < 3; k++) f[k] /= fl;
    const double ul = norm(up);
    double r[3], u[3];
    cross(f, up, r);
    const double rl = norm(r);
    // |f x up| = |up| sin(angle): parallel to within rounding counts as parallel
    if (!(ul > 0.0) || !(rl > 1e-12 * ul)) return set_err("look_at: up is parallel to the view");
    for (int k = 0; k < 3; k++) r[k] /= rl;
    cross(r, f, u);
    if (!(vfov_deg > 0.0 && vfov_deg < 180.0)) return set_err("look_at: vfov_deg must lie in (0, 180)");
    if (!(focus_dist > 0.0)) return set_err("look_at: focus_dist must be > 0");
    if (lens_radius < 0.0) return set_err("look_at: lens_radius must be >= 0");
    const double hh = focus_dist * std::tan(vfov_deg * (3.14159265358979323846 / 180.0) * 0.5);
    const double hw = hh * (double)W / (double)H;
    for (int k = 0; k < 3; k++) {
        out->origin[k] = (float)eye[k];
        out->p0[k] = (float)(eye[k] + f[k] * focus_dist - r[k] * hw - u[k] * hh);
        out->du[k] = (float)(r[k] * (2.0 * hw / (double)W));
        out->dv[k] = (float)(u[k] * (2.0 * hh / (double)H));
        out->lens_u[k] = (float)r[k];
        out->lens_v[k] = (float)u[k];
    }
    out->lens_radius = (float)lens_radius;
    return 0;
}

int pt_scene_camera(const pt_scene* s, int W, int H, pt_camera* out) {
    if (!s || !out) return set_err("null argument");
    const pt::RenderSettings& st = s->s.settings;
    if (!st.has_camera) return 0;
    double focus = st.cam_focus;
    if (focus < 0.0) {
        double d2 = 0.0;
        for (int k = 0; k < 3; k++) d2 += (st.cam_target[k] - st.cam_eye[k]) * (st.cam_target[k] - st.cam_eye[k]);
        focus = std::sqrt(d2);
        if (!(focus > 0.0)) return set_err("look_at: eye and target coincide");
    }
    if (pt_camera_look_at(st.cam_eye, st.cam_target, st.cam_up, st.cam_fov, focus, st.cam_lens, W, H, out) < 0) return -1;
    return 1;
}

void pt_renderer_free(pt_renderer* r) {
    if (!r) return;
    delete r->r;
    delete r;
}

int pt_selftest_math(int n, const float* x, const float* y, float* out) {
    if (n < 0 || (n > 0 && (!x || !y || !out))) return set_err("bad arguments");
    std::string e;
    if (pt::selftest_math(n, x, y, out, &e) < 0) return set_err(e);
    return 0;
}

int pt_selftest_dielectric(int n, const float* dir, const float* nrm, const float* ior, const float* u, float* out_dir,
                           int* out_event) {
    if (n < 0 || (n > 0 && (!dir || !nrm || !ior || !u || !out_dir || !out_event))) return set_err("bad arguments");
    std::string e;
    if (pt::selftest_dielectric(n, dir, nrm, ior, u, out_dir, out_event, &e) < 0) return set_err(e);
    return 0;
}

int pt_render(const char* scene_config, const pt_render_config* cfg, const char* bmp_out) {
    pt_render_config c;
    if (cfg) c = *cfg; else pt_default_config(&c);
    pt_scene* s = pt_scene_create();
    if (!s) return -1;
    int rc = pt_scene_load_config(s, scene_config);
    if (rc >= 0) rc = pt_scene_apply_settings(s, &c);
    if (rc >= 0) rc = pt_scene_build(s, c.grid, c.accel != PT_ACCEL_GRID ? 1 : 0);
    pt_renderer* r = rc >= 0 ? pt_renderer_create(&c) : nullptr;
    if (rc >= 0 && !r) rc = -1;
    pt_camera cam;
    const int has_cam = rc >= 0 ? pt_scene_camera(s, c.width, c.height, &cam) : 0;
    if (has_cam < 0) rc = -1;
    if (rc >= 0 && has_cam > 0) rc = pt_renderer_set_camera(r, &cam);
    if (rc >= 0 && pt_scene_direct_light(s) > 0) {       // the RENDER block's direct_light: 1 (it implies moments)
        rc = pt_renderer_enable_moments(r, nullptr);
        if (rc >= 0) rc = pt_renderer_set_direct_light(r, 1);
    }
    if (rc >= 0) rc = pt_renderer_allocate_on_gpu(r, s);
    if (rc >= 0) rc = pt_renderer_render_loop(r, 0, c.iterations);
    if (rc >= 0) rc = pt_renderer_synchronize(r);
    if (rc >= 0 && bmp_out) rc = pt_renderer_render_image(r, bmp_out, c.iterations);
    pt_renderer_free(r);
    pt_scene_destroy(s);
    return rc < 0 ? -1 : 0;
}

}  // extern "C"
