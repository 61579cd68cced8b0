/*
 * bridge.cpp -- C entry points over the reference's own code, built for the
 * host into oracle/_ref/libptref.so.  TEST INFRASTRUCTURE ONLY, like the rest
 * of oracle/.
 *
 * What is compiled is the reference's text, not a restatement of it:
 *   - Primitive.h, Config.h, GPUMemoryPool.h, Scene.h, Renderer.h, utility.h
 *     and the reference's glm are #included whole and unchanged;
 *   - the device functions and kernel bodies of Renderer.cpp and the grid
 *     builder of Scene.cpp are copied, unchanged, into oracle/_ref/*.inc by
 *     extract.py when the library is built (those two files cannot compile
 *     whole on a host: kernel launch syntax and Assimp).
 * Everything in this directory is our own text: the shim headers (empty CUDA
 * qualifiers, malloc/memcpy behind the few cuda* names, forward declarations
 * for Assimp), this bridge and the Makefile rule.  No GPU runtime is called
 * or linked.
 *
 * Where this build differs from the reference's CUDA build -- the whole list:
 *   1. MATH.  utility.h's sin, cos, sinf, cosf and powf calls are routed to
 *      the oracle's ptor_sinf / ptor_cosf / ptor_powf by macros defined after
 *      glm and thrust are included and removed right after utility.h.  The
 *      host libm and CUDA's libdevice both differ from these by a few ulp on
 *      about 1 % of arguments, so without the routing nothing downstream
 *      could be compared bit for bit.
 *   2. FRAME SIZE.  RESOLUTION_X / RESOLUTION_Y are compile-time constants in
 *      Config.h; they are re-pointed at two variables so one library renders
 *      any frame.  The expressions that use them are untouched.
 *   3. LAUNCH INDICES.  __global__ is empty and threadIdx / blockIdx /
 *      blockDim are per-thread host variables; a "launch" is a loop that sets
 *      them and calls the kernel body once per thread.
 *   4. THE MISSING RETURN.  computeRayGridIntersection has no return
 *      statement on the path where the ray misses the mesh's bounding box.
 *      That is undefined behaviour in C++.  An optimising compiler may treat
 *      the path as unreachable, drop the bounding-box rejection altogether
 *      and walk the grid for rays that miss the box; the triangle test's
 *      EPSILON slack then accepts hits just outside a face.  The library is
 *      built with -fno-strict-return so the path stays; the value returned
 *      there is still unspecified, and in this build it is "no hit" on every
 *      ray tested (tests/test_reference_code.py would fail otherwise).  See
 *      DESIGN.md, "The reference's own code as a second oracle".
 *   5. Host float->int conversion (cvttss2si) gives INT_MIN for NaN and
 *      out-of-range values where the GPU saturates.  The one place the
 *      intersection code can reach it is computeRayGridIntersection's
 *      ivoxel_3d = ABS(...) / voxel_width with a zero voxel width (a flat
 *      mesh); the reference scene's voxel widths are all 68 or more (a
 *      stand-alone program over this file built with
 *      -fsanitize=float-cast-overflow reports nothing on the tests' 420,000
 *      rays), and the tests use this library on scenes without flat meshes.
 * -ffp-contract=off, as everywhere else in this project.
 */
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "cuda.h"
#include "cuda_runtime_api.h"
#include "device_launch_parameters.h"

#define GLM_FORCE_CUDA
#include <glm/glm.hpp>
#include <glm/gtc/matrix_transform.hpp>
#include <thrust/random.h>
#include <thrust/remove.h>

#include "../ptoracle.h"

#include "Renderer.h"

/* 2. frame size */
static int ptref_res_x = RESOLUTION_X;
static int ptref_res_y = RESOLUTION_Y;
#undef RESOLUTION_X
#undef RESOLUTION_Y
#define RESOLUTION_X ptref_res_x
#define RESOLUTION_Y ptref_res_y

/* 1. math */
#define sin(x) ptor_sinf(x)
#define cos(x) ptor_cosf(x)
#define sinf(x) ptor_sinf(x)
#define cosf(x) ptor_cosf(x)
#define powf(x, y) ptor_powf(x, y)
#include "utility.h"
#undef sin
#undef cos
#undef sinf
#undef cosf
#undef powf

/* 3. launch indices */
struct ptref_dim3 { int x, y, z; };
static thread_local ptref_dim3 ptref_threadIdx = {0, 0, 0};
static thread_local ptref_dim3 ptref_blockIdx = {0, 0, 0};
static thread_local ptref_dim3 ptref_blockDim = {1, 1, 1};
#undef __global__
#define __global__
#define threadIdx ptref_threadIdx
#define blockIdx ptref_blockIdx
#define blockDim ptref_blockDim

#include "renderer_device.inc"

#undef threadIdx
#undef blockIdx
#undef blockDim

/* Scene's constructor loads meshes through Assimp in the reference.  Here it
 * takes the flat arrays instead and then calls the reference's own
 * addMeshesToGrid (a private member, reachable from a constructor). */
static const ptor_scene *ptref_scene_in = nullptr;

Scene::Scene(string config)
{
    const ptor_scene *s = ptref_scene_in;
    (void)config;
    for (int i = 0; i < s->nv; i++) {
        Vertex v;
        v.position = glm::vec3(s->vpos[3 * i], s->vpos[3 * i + 1], s->vpos[3 * i + 2]);
        v.normal = glm::vec3(s->vnrm[3 * i], s->vnrm[3 * i + 1], s->vnrm[3 * i + 2]);
        v.uv = glm::vec2(0.0f, 0.0f);
        vertices.push_back(v);
    }
    for (int i = 0; i < s->nt; i++) {
        Triangle t;
        for (int j = 0; j < 3; j++) t.vertex_indices[j] = s->tris[3 * i + j];
        triangles.push_back(t);
    }
    for (int i = 0; i < s->nmesh; i++) {
        Mesh m;
        m.vertex_indices.start_index = s->mesh_ranges[4 * i + 0];
        m.vertex_indices.end_index = s->mesh_ranges[4 * i + 1];
        m.triangle_indices.start_index = s->mesh_ranges[4 * i + 2];
        m.triangle_indices.end_index = s->mesh_ranges[4 * i + 3];
        m.bounding_box.min = glm::vec3(s->mesh_bbox[6 * i], s->mesh_bbox[6 * i + 1], s->mesh_bbox[6 * i + 2]);
        m.bounding_box.max = glm::vec3(s->mesh_bbox[6 * i + 3], s->mesh_bbox[6 * i + 4], s->mesh_bbox[6 * i + 5]);
        meshes.push_back(m);
    }
    for (int i = 0; i < s->nmodel; i++) {
        Model m;
        m.mesh_index = s->model_ints[3 * i + 0];
        m.grid_index = s->model_ints[3 * i + 1];
        memcpy(&m.model_to_world[0][0], s->model_m2w + 16 * i, 64);
        memcpy(&m.world_to_model[0][0], s->model_w2m + 16 * i, 64);
        m.mat.material_type = (Material::MaterialType)s->model_ints[3 * i + 2];
        m.mat.refractive_index = 0.0f;
        m.mat.reflectivity = 0.0f;
        m.mat.color = glm::vec3(s->model_color[3 * i], s->model_color[3 * i + 1], s->model_color[3 * i + 2]);
        models.push_back(m);
    }
    addMeshesToGrid();
}

#include "scene_grid.inc"

namespace {

void set_launch(int i)
{
    ptref_threadIdx.x = 0;
    ptref_blockDim.x = 1;
    ptref_blockIdx.x = i;
}

int check_grid(const ptor_scene *s)
{
    if (s->gdim[0] != GRID_X || s->gdim[1] != GRID_Y || s->gdim[2] != GRID_Z) {
        fprintf(stderr, "ptref: the reference's grid is %dx%dx%d (Config.h), the scene's is %dx%dx%d\n",
                GRID_X, GRID_Y, GRID_Z, s->gdim[0], s->gdim[1], s->gdim[2]);
        return -1;
    }
    return 0;
}

/* One kernel "launch" spread over host threads, 256 indices at a time. */
template <typename F>
void parallel_for(int n, int threads, F body)
{
    int nt = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    nt = std::max(1, std::min(nt, std::min(16, (n + 255) / 256)));
    if (nt == 1) {
        for (int i = 0; i < n; i++) body(i);
        return;
    }
    std::atomic<int> next(0);
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; t++)
        pool.emplace_back([&]() {
            for (;;) {
                int b = next.fetch_add(256);
                if (b >= n) return;
                int e = std::min(n, b + 256);
                for (int i = b; i < e; i++) body(i);
            }
        });
    for (auto &th : pool) th.join();
}

template <typename T>
void drop_pool(GPUMemoryPool<T> *p)
{
    p->free();
    std::free(p);
}

template <typename T>
GPUMemoryPool<T> *make_pool(const std::vector<T> &data)
{
    GPUMemoryPool<T> local;
    GPUMemoryPool<T> *p = local.getInstance();
    p->allocate(data);
    return p;
}

/* The pools Renderer::allocateOnGPU fills, from the flat arrays (grids
 * included: the walk is tested apart from the builder). */
struct Pools {
    RenderData rd;

    Pools(const ptor_scene *s, int nrays, int npixels)
    {
        memset(&rd, 0, sizeof rd);
        std::vector<Model> models(s->nmodel);
        for (int i = 0; i < s->nmodel; i++) {
            Model &m = models[i];
            m.mesh_index = s->model_ints[3 * i + 0];
            m.grid_index = s->model_ints[3 * i + 1];
            memcpy(&m.model_to_world[0][0], s->model_m2w + 16 * i, 64);
            memcpy(&m.world_to_model[0][0], s->model_w2m + 16 * i, 64);
            m.mat.material_type = (Material::MaterialType)s->model_ints[3 * i + 2];
            m.mat.refractive_index = 0.0f;
            m.mat.reflectivity = 0.0f;
            m.mat.color = glm::vec3(s->model_color[3 * i], s->model_color[3 * i + 1], s->model_color[3 * i + 2]);
        }
        std::vector<Mesh> meshes(s->nmesh);
        for (int i = 0; i < s->nmesh; i++) {
            Mesh &m = meshes[i];
            m.vertex_indices.start_index = s->mesh_ranges[4 * i + 0];
            m.vertex_indices.end_index = s->mesh_ranges[4 * i + 1];
            m.triangle_indices.start_index = s->mesh_ranges[4 * i + 2];
            m.triangle_indices.end_index = s->mesh_ranges[4 * i + 3];
            m.bounding_box.min = glm::vec3(s->mesh_bbox[6 * i], s->mesh_bbox[6 * i + 1], s->mesh_bbox[6 * i + 2]);
            m.bounding_box.max = glm::vec3(s->mesh_bbox[6 * i + 3], s->mesh_bbox[6 * i + 4], s->mesh_bbox[6 * i + 5]);
        }
        std::vector<Vertex> vertices(s->nv);
        for (int i = 0; i < s->nv; i++) {
            vertices[i].position = glm::vec3(s->vpos[3 * i], s->vpos[3 * i + 1], s->vpos[3 * i + 2]);
            vertices[i].normal = glm::vec3(s->vnrm[3 * i], s->vnrm[3 * i + 1], s->vnrm[3 * i + 2]);
            vertices[i].uv = glm::vec2(0.0f, 0.0f);
        }
        std::vector<Triangle> triangles(s->nt);
        for (int i = 0; i < s->nt; i++)
            for (int j = 0; j < 3; j++) triangles[i].vertex_indices[j] = s->tris[3 * i + j];
        std::vector<Grid> grids(s->ngrid);
        for (int i = 0; i < s->ngrid; i++) {
            grids[i].voxelIndices.start_index = s->grid_ints[4 * i + 0];
            grids[i].voxelIndices.end_index = s->grid_ints[4 * i + 1];
            grids[i].entity_type = (EntityType)s->grid_ints[4 * i + 2];
            grids[i].entity_index = s->grid_ints[4 * i + 3];
            grids[i].voxel_width.x = s->grid_vw[3 * i + 0];
            grids[i].voxel_width.y = s->grid_vw[3 * i + 1];
            grids[i].voxel_width.z = s->grid_vw[3 * i + 2];
        }
        std::vector<Voxel> voxels(s->nvox);
        for (int i = 0; i < s->nvox; i++) {
            voxels[i].entity_index_range.start_index = s->vox[3 * i + 0];
            voxels[i].entity_index_range.end_index = s->vox[3 * i + 1];
            voxels[i].entity_type = (EntityType)s->vox[3 * i + 2];
        }
        std::vector<EntityIndex> per_voxel(s->per_voxel, s->per_voxel + s->npv);

        rd.dev_model_data = make_pool(models);
        rd.dev_mesh_data = make_pool(meshes);
        rd.dev_per_vertex_data = make_pool(vertices);
        rd.dev_triangle_data = make_pool(triangles);
        rd.dev_grid_data = make_pool(grids);
        rd.dev_voxel_data = make_pool(voxels);
        rd.dev_per_voxel_data = make_pool(per_voxel);
        /* vector<Ray>(n) and the rest start zero-filled, as in allocateOnGPU */
        std::vector<Ray> rays(nrays);
        memset((void *)rays.data(), 0, sizeof(Ray) * rays.size());
        rd.dev_ray_data = make_pool(rays);
        std::vector<Pixel> image(npixels);
        memset((void *)image.data(), 0, sizeof(Pixel) * image.size());
        rd.dev_image_data = make_pool(image);
        std::vector<int> stencil(nrays, 0);
        rd.dev_stencil = make_pool(stencil);
        std::vector<IntersectionData> isect(nrays);
        memset((void *)isect.data(), 0, sizeof(IntersectionData) * isect.size());
        rd.dev_intersection_data = make_pool(isect);
        rd.dev_first_intersection_cache = make_pool(isect);
    }

    ~Pools()
    {
        drop_pool(rd.dev_model_data); drop_pool(rd.dev_mesh_data); drop_pool(rd.dev_per_vertex_data);
        drop_pool(rd.dev_triangle_data); drop_pool(rd.dev_grid_data); drop_pool(rd.dev_voxel_data);
        drop_pool(rd.dev_per_voxel_data); drop_pool(rd.dev_ray_data); drop_pool(rd.dev_image_data);
        drop_pool(rd.dev_stencil); drop_pool(rd.dev_intersection_data); drop_pool(rd.dev_first_intersection_cache);
    }
};

}  // namespace

extern "C" {

/* makeSeededRandomEngine + the first uniform_real_distribution<float>(0,1) draw */
float ptref_u01_first(int iter, int index, int depth)
{
    thrust::default_random_engine rng = makeSeededRandomEngine(iter, index, depth);
    thrust::uniform_real_distribution<float> u01(0, 1);
    return u01(rng);
}

/* kind 0: calculateRandomDirectionInHemisphere, 1: calculateMetalScattering,
 * 2: calculateCoatScattering, 3: reflectRay.  One engine per ray, seeded
 * (iter[i], slot[i], depth[i]).  dir is used as given (not normalised). */
int ptref_scatter(int kind, int n, const int *iter, const int *slot, const int *depth,
                  const float *normal, const float *dir, float *out)
{
    for (int i = 0; i < n; i++) {
        glm::vec3 nn(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]);
        glm::vec3 d(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
        thrust::default_random_engine rng = makeSeededRandomEngine(iter[i], slot[i], depth[i]);
        glm::vec3 r;
        if (kind == 0) r = calculateRandomDirectionInHemisphere(nn, rng);
        else if (kind == 1) r = calculateMetalScattering(nn, d, rng);
        else if (kind == 2) r = calculateCoatScattering(nn, d, rng);
        else if (kind == 3) r = reflectRay(d, nn);
        else return -1;
        out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
    }
    return 0;
}

/* kind 0: transformPosition, 1: transformDirection, 2: transformNormal, with one
 * column-major matrix for the batch. */
int ptref_transform(int kind, int n, const float *m16, const float *v, float *out)
{
    glm::mat4 m;
    memcpy(&m[0][0], m16, 64);
    for (int i = 0; i < n; i++) {
        glm::vec3 p(v[3 * i], v[3 * i + 1], v[3 * i + 2]);
        glm::vec3 r;
        if (kind == 0) r = transformPosition(p, m);
        else if (kind == 1) r = transformDirection(p, m);
        else if (kind == 2) r = transformNormal(p, m);
        else return -1;
        out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
    }
    return 0;
}

/* The pattern Scene::Scene repeats for every model, with the reference's glm:
 * translate * rotate(about y) * scale, and its inverse. */
void ptref_model_matrix(const float scale[3], float rot_y_deg, const float translate[3],
                        float m2w[16], float w2m[16])
{
    const glm::mat4 one(1.0f);
    glm::mat4 a = glm::translate(one, glm::vec3(translate[0], translate[1], translate[2]))
                * glm::rotate(one, glm::radians(rot_y_deg), glm::vec3(0.0f, 1.0f, 0.0f))
                * glm::scale(one, glm::vec3(scale[0], scale[1], scale[2]));
    glm::mat4 b = glm::inverse(a);
    memcpy(m2w, &a[0][0], 64);
    memcpy(w2m, &b[0][0], 64);
}

/* computeRaySceneIntersectionKernel, one thread per ray.  mat_type is -1 and
 * dist FLOAT_MAX where nothing is hit. */
int ptref_intersect_rays(const ptor_scene *s, int n, const float *orig, const float *dir,
                         float *dist, float *normal, int *mat_type, float *mat_color, int threads)
{
    if (check_grid(s)) return -1;
    Pools P(s, n, 1);
    RenderData rd = P.rd;
    for (int i = 0; i < n; i++) {
        Ray &r = rd.dev_ray_data->pool[i];
        r.base.orig = glm::vec3(orig[3 * i], orig[3 * i + 1], orig[3 * i + 2]);
        r.base.dir = glm::vec3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
        IntersectionData &h = rd.dev_intersection_data->pool[i];
        h.impact_distance = FLOAT_MAX;
        h.impact_normal = glm::vec3(0.0f, 0.0f, 0.0f);
        h.impact_mat.material_type = (Material::MaterialType)-1;
        h.impact_mat.color = glm::vec3(0.0f, 0.0f, 0.0f);
    }
    parallel_for(n, threads, [&](int i) {
        set_launch(i);
        computeRaySceneIntersectionKernel(n, rd);
    });
    for (int i = 0; i < n; i++) {
        const IntersectionData &h = rd.dev_intersection_data->pool[i];
        dist[i] = h.impact_distance;
        normal[3 * i] = h.impact_normal.x; normal[3 * i + 1] = h.impact_normal.y; normal[3 * i + 2] = h.impact_normal.z;
        mat_type[i] = (int)h.impact_mat.material_type;
        mat_color[3 * i] = h.impact_mat.color.x; mat_color[3 * i + 1] = h.impact_mat.color.y; mat_color[3 * i + 2] = h.impact_mat.color.z;
    }
    return 0;
}

/* shadeRayKernel over a batch, laid out like ptor_shade: ray i is shaded as
 * the thread with index slot[i].  State arrays are updated in place; hit_dist
 * receives what the kernel leaves in impact_distance. */
int ptref_shade(int n, int iter, const int *slot, float *orig, float *dir, float *color, int *bounces,
                float *hit_dist, const float *hit_normal, const int *hit_type, const float *hit_color)
{
    RenderData rd;
    memset(&rd, 0, sizeof rd);
    GPUMemoryPool<Ray> rays;
    GPUMemoryPool<IntersectionData> hits;
    rd.dev_ray_data = &rays;
    rd.dev_intersection_data = &hits;
    for (int i = 0; i < n; i++) {
        Ray r;
        memset((void *)&r, 0, sizeof r);
        r.base.orig = glm::vec3(orig[3 * i], orig[3 * i + 1], orig[3 * i + 2]);
        r.base.dir = glm::vec3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
        r.color = glm::vec3(color[3 * i], color[3 * i + 1], color[3 * i + 2]);
        r.meta_data.remaining_bounces = bounces[i];
        IntersectionData h;
        memset((void *)&h, 0, sizeof h);
        h.impact_distance = hit_dist[i];
        h.impact_normal = glm::vec3(hit_normal[3 * i], hit_normal[3 * i + 1], hit_normal[3 * i + 2]);
        h.impact_mat.material_type = (Material::MaterialType)hit_type[i];
        h.impact_mat.color = glm::vec3(hit_color[3 * i], hit_color[3 * i + 1], hit_color[3 * i + 2]);
        /* the kernel indexes both pools with its thread index: point element
         * slot[i] of each pool at the one ray and hit record that exist */
        rays.pool = &r - slot[i];
        hits.pool = &h - slot[i];
        rays.size = hits.size = slot[i] + 1;
        set_launch(slot[i]);
        shadeRayKernel(slot[i] + 1, iter, rd);
        orig[3 * i] = r.base.orig.x; orig[3 * i + 1] = r.base.orig.y; orig[3 * i + 2] = r.base.orig.z;
        dir[3 * i] = r.base.dir.x; dir[3 * i + 1] = r.base.dir.y; dir[3 * i + 2] = r.base.dir.z;
        color[3 * i] = r.color.x; color[3 * i + 1] = r.color.y; color[3 * i + 2] = r.color.z;
        bounces[i] = r.meta_data.remaining_bounces;
        hit_dist[i] = h.impact_distance;
    }
    return 0;
}

/* Renderer::renderLoop's sequence over the reference's kernels: initImage,
 * then per iteration generateRays, (first-hit cache | intersect), shade,
 * compactStencil, stable partition, ..., gather.  std::stable_partition with
 * the reference's hasTerminated predicate over the stencil stands in for
 * thrust's.  tail_drop = 1 launches ceil(nrays / 32) blocks with the
 * reference's integer division, i.e. (nrays / 32) * 32 threads; 0 launches
 * every ray.  image[w*h*3] is overwritten; live[ib] receives the number of
 * rays entering bounce ib, summed over the iterations (live_cap entries). */
int ptref_render(const ptor_scene *s, int width, int height, int first_iter, int iterations,
                 int tail_drop, float *image, long long *live, int live_cap, int threads)
{
    if (check_grid(s)) return -1;
    ptref_res_x = width;
    ptref_res_y = height;
    const int total = width * height * SAMPLESX * SAMPLESY;
    Pools P(s, total, width * height);
    RenderData rd = P.rd;
    const int launched = tail_drop ? (total / 32) * 32 : total;
    for (int i = 0; i < live_cap; i++) live[i] = 0;

    int nrays = total;
    for (int i = 0; i < launched; i++) { set_launch(i); initImageKernel(nrays, rd); }
    bool have_cache = false;                 /* the first iteration's bounce-0 hits, reused by the later ones */
    std::vector<std::pair<Ray, int>> zipped;
    for (int it = 0; it < iterations; it++) {
        const int iter = first_iter + it;
        int bounce = 0;
        nrays = rd.dev_ray_data->size;
        for (int i = 0; i < launched; i++) { set_launch(i); generateRaysKernel(nrays, rd); }
        for (;;) {
            if (bounce < live_cap) live[bounce] += std::min(nrays, launched);
            IntersectionData *hits = rd.dev_intersection_data->pool;
            IntersectionData *kept = rd.dev_first_intersection_cache->pool;
            if (bounce == 0 && have_cache) {
                std::copy(kept, kept + rd.dev_first_intersection_cache->size, hits);
            } else {
                parallel_for(launched, threads, [&](int i) {
                    set_launch(i);
                    computeRaySceneIntersectionKernel(nrays, rd);
                });
                if (bounce == 0) {
                    std::copy(hits, hits + rd.dev_intersection_data->size, kept);
                    have_cache = true;
                }
            }
            for (int i = 0; i < launched; i++) { set_launch(i); shadeRayKernel(nrays, iter, rd); }
            for (int i = 0; i < launched; i++) {
                set_launch(i);
                compactStencilKernel(nrays, rd.dev_ray_data->pool, rd.dev_stencil->pool);
            }
            /* thrust::stable_partition(pool, pool + nrays, stencil, hasTerminated()) */
            zipped.resize(nrays);
            for (int i = 0; i < nrays; i++) zipped[i] = std::make_pair(rd.dev_ray_data->pool[i], rd.dev_stencil->pool[i]);
            hasTerminated pred;
            auto mid = std::stable_partition(zipped.begin(), zipped.end(),
                                             [&pred](const std::pair<Ray, int> &z) { return pred(z.second); });
            for (int i = 0; i < nrays; i++) rd.dev_ray_data->pool[i] = zipped[i].first;
            nrays = (int)(mid - zipped.begin());
            bounce++;
            if (nrays == 0) break;
        }
        for (int i = 0; i < launched; i++) { set_launch(i); gatherImageDataKernel(rd); }
    }
    for (int i = 0; i < width * height; i++) {
        const glm::vec3 &c = rd.dev_image_data->pool[i].color;
        image[3 * i] = c.x; image[3 * i + 1] = c.y; image[3 * i + 2] = c.z;
    }
    return 0;
}

/* Scene::addMeshesToGrid over the flat meshes and models.  Same outputs and
 * capacity convention as ptor_build_grids; model_grid[nmodel] receives each
 * model's grid_index. */
int ptref_build_grids(const ptor_scene *s, int *model_grid, int *ngrid, int *grid_ints, float *grid_vw,
                      int *nvox, int *vox, int pv_cap, int *npv, int *per_voxel)
{
    if (check_grid(s)) return -1;
    ptref_scene_in = s;
    Scene scene("");
    ptref_scene_in = nullptr;
    *ngrid = (int)scene.grids.size();
    *nvox = (int)scene.voxels.size();
    *npv = (int)scene.per_voxel_data_pool.size();
    if (*npv > pv_cap) return -*npv;
    for (int i = 0; i < s->nmodel; i++) model_grid[i] = scene.models[i].grid_index;
    for (int i = 0; i < *ngrid; i++) {
        const Grid &g = scene.grids[i];
        grid_ints[4 * i + 0] = g.voxelIndices.start_index;
        grid_ints[4 * i + 1] = g.voxelIndices.end_index;
        grid_ints[4 * i + 2] = (int)g.entity_type;
        grid_ints[4 * i + 3] = g.entity_index;
        grid_vw[3 * i + 0] = g.voxel_width.x; grid_vw[3 * i + 1] = g.voxel_width.y; grid_vw[3 * i + 2] = g.voxel_width.z;
    }
    for (int i = 0; i < *nvox; i++) {
        vox[3 * i + 0] = scene.voxels[i].entity_index_range.start_index;
        vox[3 * i + 1] = scene.voxels[i].entity_index_range.end_index;
        vox[3 * i + 2] = (int)scene.voxels[i].entity_type;
    }
    for (int i = 0; i < *npv; i++) per_voxel[i] = scene.per_voxel_data_pool[i];
    return 0;
}

}  /* extern "C" */
