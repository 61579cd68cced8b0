/*
 * pathtracer_amd.h -- C ABI of the MI355X-native PathTracerAP hot path.
 *
 * Drop-in boundary for the reference's render path
 * (purvakulkarni15/PathTracerAP).  Plain pointers and sizes only; the
 * implementation is libpathtracer_amd.so (C++ host + gfx950 HIP kernels).
 * Each entry point names the reference interface it replaces:
 *
 *   pt_scene_load_config     <- Scene::Scene(string config)          Scene.cpp:3, Scene.h:24
 *   pt_scene_load_obj        <- Scene::loadAndProcessMeshFile        Scene.cpp:226-238
 *   pt_scene_add_mesh        <- Scene::processMesh                   Scene.cpp:264-291
 *   pt_scene_add_model       <- Model setup in Scene::Scene          Scene.cpp:32-42 (x11)
 *   pt_scene_build           <- Scene::addMeshesToGrid               Scene.cpp:318-396 (+ the per-mesh BLAS)
 *   pt_renderer_allocate_on_gpu <- Renderer::allocateOnGPU           Renderer.cpp:65-130, Renderer.h:49
 *   pt_renderer_clear_image  <- initImageKernel                      Renderer.cpp:557-565
 *   pt_renderer_render_loop  <- Renderer::renderLoop                 Renderer.cpp:567-648, Renderer.h:50
 *   pt_renderer_render_image <- Renderer::renderImage                Renderer.cpp:15-63, Renderer.h:51
 *   pt_renderer_free         <- Renderer::free                       Renderer.cpp:132-148, Renderer.h:52
 *   pt_render                <- main()                               main.cpp:11-27
 *
 * Compile-time constants of Config.h (RESOLUTION_X/Y, ITER, GRID_X/Y/Z) and
 * the hard-coded camera/bounce count of generateRaysKernel
 * (Renderer.cpp:521-555) are fields of pt_render_config.
 *
 * Error behaviour: functions returning int return 0 on success and a
 * negative value on failure; pointer-returning functions return NULL.  The
 * message is available from pt_last_error() (per thread).  There is no CPU
 * fallback: without a usable gfx950 device, pt_renderer_allocate_on_gpu
 * fails.
 */
#ifndef PATHTRACER_AMD_H
#define PATHTRACER_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 9

/* Primitive.h:70-79 Material::MaterialType */
enum {
    PT_MAT_DIFFUSE = 0, PT_MAT_SPECULAR = 1, PT_MAT_REFLECTIVE = 2, PT_MAT_REFRACTIVE = 3,
    PT_MAT_EMISSIVE = 4, PT_MAT_COAT = 5, PT_MAT_METAL = 6,
    PT_MAT_DIELECTRIC = 7   /* glass; not the reference's: see "Dielectric material" below */
};

/* Intersect-stage acceleration structure. */
enum {
    PT_ACCEL_GRID = 0,      /* reference uniform grid + DDA (Renderer.cpp:238-360), bit-exact with the
                               reference's own code built for the host, a ray that misses a mesh's
                               bounding box reporting no hit (the source has no return there) */
    PT_ACCEL_BVH = 1,       /* MI355X BVH, exact closest hit with the reference triangle test */
    PT_ACCEL_GRID_FAST = 2  /* PT_ACCEL_GRID's result via BVH hit set + voxel-box DDA walk (needs BVH) */
};

typedef struct pt_scene pt_scene;
typedef struct pt_renderer pt_renderer;

typedef struct pt_render_config {
    int width, height;        /* RESOLUTION_X/Y (Config.h:12-13), default 1000 x 800 */
    int iterations;           /* ITER (Config.h:19), default 500: used by render_image / pt_render */
    int max_bounces;          /* remaining_bounces (Renderer.cpp:550), default 5 */
    int accel;                /* PT_ACCEL_*, default PT_ACCEL_GRID_FAST (the reference grid's results, bit for bit) */
    int grid[3];              /* GRID_X/Y/Z (Config.h:8-10), default 25^3 */
    int tail_drop;            /* 1: replicate the reference's ceil(n/32) launch truncation */
    double cam[3];            /* camera origin (Renderer.cpp:528), default (0,0,920) */
    double plane_z;           /* image plane z (Renderer.cpp:543), default 900 */
    double plane_x0, plane_y0, plane_w, plane_h;  /* Renderer.cpp:538-542: -10,-4,20,16 */
    int block;                /* bounce-kernel workgroup = compaction chunk: 64 (default), 128 or 256;
                                 any other value (0, 96, ...) falls back to 256.  Results are identical
                                 for every value */
    int pipelines;            /* iterations in flight on their own HIP streams, 1..32 (default 16); results
                                 are identical for every value (contributions merge in iteration order).
                                 Loading the library sets GPU_MAX_HW_QUEUES=16 (one hardware queue per
                                 pipeline stream) unless the process already set it */
    int ray_sort;             /* ray sort before each persistent trace: -1 auto (key 7 for grid_fast and bvh),
                                 0 off, 1..8 key layout; claim order only, results identical */
} pt_render_config;

int pt_abi_version(void);
const char *pt_last_error(void);
/* GPU_MAX_HW_QUEUES as the library found it when it was loaded (*at_load = -1: unset)
 * and whether the library then set it to 16 (*set_by_library = 1).  HIP reads the
 * variable once, when its runtime starts: a process whose HIP runtime started before
 * the library loaded runs with its own value (HIP's default is 4). */
int pt_hw_queue_info(int *at_load, int *set_by_library);
void pt_default_config(pt_render_config *cfg);

/* ---- Scene ---- */
pt_scene *pt_scene_create(void);
void pt_scene_destroy(pt_scene *s);
int pt_scene_load_config(pt_scene *s, const char *path);
/* Copies the config file's optional RENDER block over *cfg (only fields it sets). */
int pt_scene_apply_settings(const pt_scene *s, pt_render_config *cfg);
int pt_scene_load_obj(pt_scene *s, const char *path);                 /* -> mesh index */
int pt_scene_add_mesh(pt_scene *s, const float *pos, const float *nrm, int nv,
                      const int *tris, int nt);                        /* -> mesh index */
int pt_scene_add_model(pt_scene *s, int mesh, const float scale[3], const float rot_deg[3],
                       const float translate[3], int material, const float color[3]); /* -> model index */
/* ---- Smooth shading: the hit normal interpolates the vertex normals, per model (added within
 * ABI 9: new functions only; pt_scene_add_model, pt_render_config and PT_ABI_VERSION are
 * unchanged.  No counterpart in the reference, whose Renderer.cpp:203 averages a triangle's three
 * vertex normals into one, so every curved mesh renders as facets).  Off by default: a scene with
 * no smooth model allocates, launches and computes exactly what it did. ----
 * Sets (on != 0) or clears the flag of one model; model = -1: of every model added so far.  May be
 * called any time after the model exists, before or after pt_scene_build: the grid and the BLAS are
 * not touched.  pt_renderer_allocate_on_gpu snapshots the flags: a change made afterwards applies
 * to the next allocation.  When some model is smooth, the allocation also uploads a shading table
 * of 96 bytes per scene triangle (v0, e1, e2, n0, n1, n2), shared by all pipelines.  Refused:
 * "setModelSmooth: bad model index".
 * A hit on a smooth model uses the normal n below wherever the flat normal was used: the scatter
 * direction, the mirror reflection and the origin offset ip + n*0.1f of the shading; the
 * primary-hit cache, and hence pt_renderer_primary_hits and the denoiser's guides; and the normals
 * pt_renderer_intersect_rays and pt_renderer_trace_rays report.
 * Inputs: the world-space ray (o, d), d not normalised; the world distance dist; the hit model M
 * with its world_to_model w2m (rows 0..2) and nm = inverse(mat3(model_to_world)); the scene
 * triangle's v0, e1 = v1 - v0, e2 = v2 - v0 (model space, as the triangle test reads them) and its
 * stored vertex normals n0, n1, n2 (vnrm of pt_scene_export, the x1000 values); g, the flat unit
 * world normal normalize(nm * normalize((n0 + n1 + n2) * (1/3))).  float32 IEEE in exactly this
 * order, no fused multiply-add; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, normalize(a) =
 * a * (1.0f / sqrtf(dot(a, a))), (w2m * p)_k = (w2m[0][k]*p.x + w2m[1][k]*p.y) + (w2m[2][k]*p.z +
 * w2m[3][k]*1.0f), (nm * m)_r = (nm[r][0]*m.x + nm[r][1]*m.y) + nm[r][2]*m.z:
 *   dir = normalize(d);  ip = o + dir * dist                  (the shading's own hit point)
 *   pm  = w2m * ip;  q = pm - v0
 *   d11 = dot(e1,e1); d12 = dot(e1,e2); d22 = dot(e2,e2); q1 = dot(q,e1); q2 = dot(q,e2)
 *   den = d11*d22 - d12*d12
 *   b1 = (d22*q1 - d12*q2) / den;   b2 = (d11*q2 - d12*q1) / den
 *   b1 = fminf(fmaxf(b1, 0.0f), 1.0f);  b2 = fminf(fmaxf(b2, 0.0f), 1.0f - b1);  b0 = (1.0f - b1) - b2
 *   m  = (n0*b0 + n1*b1) + n2*b2                               (per component)
 *   s  = normalize(nm * m)
 *   n  = (s.x, s.y, s.z all finite and dot(s, g) > 0) ? s : g
 * fmaxf / fminf drop a NaN, so a zero-area triangle (den = 0) lands on n0 or a corner without a
 * special case.  The triangle test accepts points a tolerance outside the triangle; the clamp
 * keeps those on its edge.  n is a function of (o, d, dist, model, triangle) alone: every path
 * that shades a hit computes the same bits.
 * Limits.  A scattered or reflected direction may point below the geometric surface (the usual
 * shading-normal terminator); nothing is done about it.  g is itself the average of the vertex
 * normals, so dot(s, g) <= 0 catches a vertex normal that opposes its neighbours, which falls back
 * to the flat normal, not a mesh whose normals all oppose the winding: there g opposes it too and
 * smooth shading follows the normals, as flat shading does.  Normals that interpolate to zero
 * (s not finite) fall back to the flat normal as well.  An OBJ file without
 * `vn` gets per-corner geometric normals from the loader, so smooth equals flat there up to
 * rounding: welded normals are not generated.
 * Config grammar: the optional attribute shading:smooth or shading:flat on MESH, SPHERE and BOX
 * blocks (another value is refused: "bad attribute ..."). */
int pt_scene_set_model_smooth(pt_scene *s, int model, int on);
/* The flag of one model: 0 or 1; negative: error ("pt_scene_model_smooth: bad model index"). */
int pt_scene_model_smooth(const pt_scene *s, int model);
/* ---- Albedo textures: per-vertex uvs and a bilinear lookup at the hit, per model (added within
 * ABI 9: new functions only; pt_render_config, pt_scene_add_mesh, pt_scene_add_model and
 * PT_ABI_VERSION are unchanged.  No counterpart in the reference, whose Primitive.h declares a uv
 * and never reads it).  Off by default: a scene with no textured model allocates, launches and
 * computes exactly what it did. ----
 * pt_scene_set_mesh_uv stores nv*2 floats (u, v per vertex) for the mesh's vertices, in
 * pt_scene_add_mesh's vertex order; `built`, the grid and the BLAS are left alone.  Refused:
 * "setMeshUv: bad mesh index", "setMeshUv: nv is not the mesh's vertex count", "setMeshUv:
 * non-finite uv".  pt_scene_export_uv writes nv_total*2 floats, (0, 0) for the vertices of a mesh
 * without uv (uv_out may be null), and returns the vertex count.  pt_scene_mesh_has_uv: 0 or 1.
 * Where uvs come from otherwise: pt_scene_load_obj reads `vt u v` and the middle index of the
 * v/vt/vn and v/vt corner forms, with negative indices as for v, and stores (u, 1.0f - v), which
 * is what the reference's one import flag, aiProcess_FlipUVs, does.  A corner without vt gets
 * (0, 0), and the mesh has uv when any corner named one.  A bad vt index is refused like a bad vn
 * index.  One exception: a face that comes before the file's first vt line has its middle
 * indices ignored, as the loader always ignored them.  A generated SPHERE gives vertex (j, i) the uv ((float)((double)i / 48),
 * (float)((double)j / 24)); a generated BOX gives each face's four corners (0,0), (1,0), (1,1),
 * (0,1) in the order it emits them.
 * pt_scene_add_texture copies w*h*3 floats, texel (row y, column x) at rgb[3*(y*w + x)], and
 * returns the texture's index.  Refused: "addTexture: width and height must be in [1,4096]",
 * "addTexture: non-finite texel".  pt_scene_texture reads one back (w, h, rgb_out may be null);
 * pt_scene_texture_count is the number of textures.
 * pt_scene_set_model_texture binds texture (-1: none) to model (-1: every model added so far),
 * before or after pt_scene_build.  Refused: "setModelTexture: bad model index", "setModelTexture:
 * bad texture index", "setModelTexture: mesh has no uv".  pt_scene_model_texture returns the
 * binding, -1 for none; -2: error ("pt_scene_model_texture: bad model index").
 * pt_renderer_allocate_on_gpu snapshots the bindings: a change made afterwards applies to the next
 * allocation.  When some model is textured the allocation also uploads every texture's texels
 * (16 bytes each), the shading table of pt_scene_set_model_smooth with the vertex uvs in its
 * spare lanes, and a 16-byte-per-pixel plane of the primary hits' albedos.
 * Definition.  The albedo mc of a hit of the world ray (o, d) at world distance dist on scene
 * triangle T of model M, when M has texture X of w x h texels; float32 IEEE in exactly this
 * order, no fused multiply-add.  b0, b1, b2 are those of pt_scene_set_model_smooth's definition
 * above, bit for bit (the same ip, pm, q, den, the same two clamps, b0 = (1.0f - b1) - b2);
 * uv0, uv1, uv2 the triangle's three stored vertex uvs:
 *   uv_k = (uv0_k*b0 + uv1_k*b1) + uv2_k*b2                 k = u, v
 *   per axis (a = uv_u with n = w gives x0, x1, tx;  a = uv_v with n = h gives y0, y1, ty):
 *     fr = a - floorf(a)                                    repeat wrap
 *     f  = fr * (float)n - 0.5f
 *     f  = fminf(fmaxf(f, -0.5f), (float)n - 0.5f)          a NaN gives way: f = -0.5
 *     fl = floorf(f);  t = f - fl
 *     i0 = (int)fl;  if (i0 < 0) i0 += n;  i1 = i0 + 1;  if (i1 >= n) i1 -= n
 *   per channel:
 *     top = X[y0][x0] + (X[y0][x1] - X[y0][x0]) * tx
 *     bot = X[y1][x0] + (X[y1][x1] - X[y1][x0]) * tx
 *     v   = top + (bot - top) * ty
 *   mc  = color_M * v                                       the model's own colour tints the texture
 * mc takes the place of the model colour wherever the shading reads it: the r.c = r.c * mc of
 * DIFFUSE, METAL, COAT, EMISSIVE and REFLECTIVE hits with bounces left (a textured EMISSIVE
 * model is a textured light).  No random draw, slot, compaction order or segment count changes.
 * mc is a function of (o, d, dist, model, triangle) alone, so every path that shades a hit gets
 * the same bits.  No load leaves the texture: fl lies in [-1, n-1], so i0 and i1 lie in [0, n-1]
 * for every float input, a NaN and fr*n rounding up to n included.
 * Limits.  No mip levels and no ray differentials: minification aliases, and pixel jitter is the
 * remedy.  Texels are linear values; a PPM's bytes are not gamma-decoded.  pt_renderer_denoise
 * filters the image as it stands, so inside one model only its luminance term stops at texture
 * detail; pt_renderer_denoise_ex with PT_DENOISE_DEMODULATE divides the primary hit's albedo out
 * first (see there).
 * Config grammar: a block TEXTURE / <name> / CHECKER / [r,g,b] / [r,g,b] / N makes an N x N
 * texture, 1 <= N <= 4096, whose texel (y, x) is the first colour when x + y is even and the
 * second otherwise; TEXTURE / <name> / PPM / <path> loads a binary P6 file with maxval <= 255
 * (a texel is (float)byte / (float)maxval; the path resolves like an OBJ path; a malformed file
 * is refused with the path in the message).  TEXTURE blocks are collected first, like material
 * blocks.  MESH, SPHERE and BOX blocks take the attribute texture:<name> (an unknown name is
 * refused: "unknown texture ..."). */
int pt_scene_set_mesh_uv(pt_scene *s, int mesh, const float *uv, int nv);
int pt_scene_export_uv(const pt_scene *s, float *uv_out);              /* -> vertex count */
int pt_scene_mesh_has_uv(const pt_scene *s, int mesh);
int pt_scene_add_texture(pt_scene *s, int w, int h, const float *rgb); /* -> texture index */
int pt_scene_texture_count(const pt_scene *s);
int pt_scene_texture(const pt_scene *s, int texture, int *w, int *h, float *rgb_out);
int pt_scene_set_model_texture(pt_scene *s, int model, int texture);
int pt_scene_model_texture(const pt_scene *s, int model);
/* ---- Dielectric material: refraction, Fresnel reflection and total internal reflection (added
 * within ABI 9: one new material value and new functions only; pt_scene_add_model's signature,
 * pt_render_config and PT_ABI_VERSION are unchanged.  No counterpart in the reference, whose
 * shading has no branch for its SPECULAR and REFRACTIVE types: those two keep doing what they
 * did, a hit only loses a bounce).  Off by default: a scene without a PT_MAT_DIELECTRIC model
 * allocates, launches and computes exactly what it did. ----
 * pt_scene_add_model accepts material PT_MAT_DIELECTRIC (7); a value above 7 is refused as before
 * ("addModel: bad material").  pt_scene_set_model_ior stores the index of refraction of one model;
 * model = -1: of every model added so far.  It is stored for every model and read only by a
 * dielectric one; 1.5 by default.  Before or after pt_scene_build: the grid and the BLAS are not
 * touched.  pt_renderer_allocate_on_gpu snapshots the values with the materials: a change made
 * afterwards applies to the next allocation.  Refused: "setModelIor: bad model index",
 * "setModelIor: ior must be finite and in [1, 4]".  pt_scene_model_ior reads it back; a negative
 * value: error ("pt_scene_model_ior: bad model index").
 * Definition.  A hit with bounces > 0 on a dielectric model, with dir = normalize(r.d) and
 * ip = r.o + dir * dist as every shade has them; n the normal this shade uses (flat, or
 * pt_scene_set_model_smooth's); ior the model's; mc the albedo (the model's colour, times its
 * texture where it has one).  float32 IEEE in exactly this order, no fused multiply-add;
 * dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z:
 *   ci  = dot(dir, n)
 *   ent = ci < 0.0f                              the normal faces the ray: entering
 *   nn  = ent ? n : -n;   c = ent ? -ci : ci;   c = fminf(c, 1.0f)
 *   eta = ent ? 1.0f / ior : ior
 *   k   = 1.0f - (eta*eta) * (1.0f - c*c)
 *   a   = (1.0f - ior) / (1.0f + ior);   r0 = a*a
 *   k < 0.0f:   total internal reflection (no draw is made)
 *   otherwise:  sk = sqrtf(k);   x = 1.0f - (ent ? c : sk);   x2 = x*x;   x5 = (x2*x2)*x
 *               Fr = r0 + (1.0f - r0) * x5                   (Schlick, cosine on the thin side)
 *               u  = the first uniform of the engine seeded (iteration, slot, r.bounces)
 *               u < Fr: reflection, else refraction
 *   reflection, total internal reflection:
 *               d' = dir + nn * (2.0f * c);           o' = ip + nn * 0.1f;   colour unchanged
 *   refraction: d' = dir * eta + nn * (eta*c - sk);   o' = ip - nn * 0.1f;   colour = colour * mc when ent
 *   then bounces-- as for every surviving material
 * The mirror direction is the true one; REFLECTIVE, COAT and METAL keep the reference's formula.
 * The two-sided triangle test lets a ray inside a mesh find the far wall, its t >= -0.005 bound
 * keeps an origin moved 0.1 past a surface from finding that surface again, and every shade
 * reseeds its engine, so the one draw disturbs no other stream.  Only the shading computes
 * anything new: every path that shades a hit (the plain loop, masked and generated iterations,
 * graph replay, every accel, pipeline count and block size) computes the same bits.  The
 * sampled first-hit guides and pt_renderer_primary_albedo report mc for a dielectric hit as for
 * every material.
 * Limits.  Glass thinner than a few times the 0.1 origin offset is not resolved.  A mesh whose
 * normals oppose its winding has inside and outside swapped.  A smooth normal near a silhouette
 * can call an entering ray a leaving one.  The colour tints once per entry, whatever the
 * thickness: there is no absorption along the path.  There are no nested media and no priority
 * between overlapping glass models.  Light seen through glass is found by the paths alone, so
 * caustics are noisy.  Under PT_DENOISE_DEMODULATE a dielectric first hit multiplies by its
 * albedo only when the sample refracts in: the caveat given there for SPECULAR and REFRACTIVE.
 * Config grammar: a material block DIELECTRIC / <name> / [r,g,b], like the other material
 * keywords, and the attribute ior:<number> on MESH, SPHERE and BOX blocks (a malformed value or
 * one outside [1, 4] is refused: "bad attribute ..."). */
int pt_scene_set_model_ior(pt_scene *s, int model, float ior);
float pt_scene_model_ior(const pt_scene *s, int model);
/* with_bvh: also build the per-mesh BLAS (needed by PT_ACCEL_GRID_FAST and PT_ACCEL_BVH;
 * pt_renderer_allocate_on_gpu adds it on demand to a scene built without it). */
int pt_scene_build(pt_scene *s, const int grid[3], int with_bvh);
/* counts[9] = nv nt nmesh nmodel ngrid nvox npv nbvh_nodes nbvh_refs */
int pt_scene_counts(const pt_scene *s, int counts[9]);
/* Flat export of Scene.h's vectors (any pointer may be NULL):
 * vpos/vnrm nv*3, tris nt*3, mesh_ranges nmesh*4 (vs ve ts te), mesh_bbox nmesh*6,
 * model_ints nmodel*3 (mesh grid material), m2w/w2m nmodel*16 column-major,
 * color nmodel*3, grid_ints ngrid*4 (vox_start vox_end entity_type entity_index),
 * grid_vw ngrid*3, vox nvox*3 (start end entity_type), per_voxel npv. */
int pt_scene_export(const pt_scene *s, float *vpos, float *vnrm, int *tris, int *mesh_ranges,
                    float *mesh_bbox, int *model_ints, float *m2w, float *w2m, float *color,
                    int *grid_ints, float *grid_vw, int *vox, int *per_voxel);

/* BVH export (ACCEL_BVH builds): nodes nbvh_nodes*16 (the 64-byte BvhNode as
 * 16 floats; int fields bit-cast), refs nbvh_refs, roots nmesh. */
int pt_scene_export_bvh(const pt_scene *s, float *nodes, int *refs, int *roots);
/* The same BLAS collapsed 4-wide (k_trace_gf's node steps): Bvh4Node records,
 * 32 words each (lo x/y/z[4], hi x/y/z[4], link[4], count[4]), and each mesh's
 * 4-wide root (-1: none).  Returns the node count (call with nodes = NULL to
 * size the buffer), < 0 on error. */
int pt_scene_export_bvh4(const pt_scene *s, float *nodes, int *roots);
/* Each mesh's first leaf record (bvh_tri_order entry), nmesh ints: a 4-wide
 * leaf link (1 << 31 | count << 26 | first) holds first relative to it, so
 * the 2^26 limit of the encoding is per mesh (ABI 8).  Returns nmesh. */
int pt_scene_export_bvh4_leaf_base(const pt_scene *s, int *bases);

/* ---- Renderer ---- */
pt_renderer *pt_renderer_create(const pt_render_config *cfg);
/* Use an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
int pt_renderer_set_stream(pt_renderer *r, void *hip_stream);
/* Accumulate into caller-owned device memory (W*H*3 floats) instead of an internal buffer. */
int pt_renderer_bind_image(pt_renderer *r, float *device_rgb);
/* For PT_ACCEL_GRID_FAST / PT_ACCEL_BVH a scene built without the BLAS gets it here (once). */
int pt_renderer_allocate_on_gpu(pt_renderer *r, const pt_scene *s);
/* Zeroes the accumulator and the trace-fault counter (a new render starts). */
int pt_renderer_clear_image(pt_renderer *r);
/* Enqueue iterations [first_iter, first_iter + n_iters) (asynchronous). */
int pt_renderer_render_loop(pt_renderer *r, int first_iter, int n_iters);
int pt_renderer_synchronize(pt_renderer *r);
int pt_renderer_read_image(pt_renderer *r, float *host_rgb);
int pt_renderer_render_image(pt_renderer *r, const char *bmp_path, int iterations_total);
/* Ray segments shaded so far (sum over bounces of live rays). */
long long pt_renderer_segments(pt_renderer *r);
/* Persistent-trace waves that hit their iteration cap and left rays untraced since
 * allocate_on_gpu or the last clear_image (0 in a correct run; -1 on error).  Non-zero
 * makes pt_renderer_synchronize / read_image / render_image fail: the image is invalid. */
long long pt_renderer_trace_faults(pt_renderer *r);
/* out[b] = live rays entering bounce b, summed over the iterations rendered (b < n, n <= 64 useful). */
int pt_renderer_segments_per_bounce(pt_renderer *r, long long *out, int n);
/* HIP-event timing read by kernel_stats: 0 off, 1 around every kernel group on every
 * pipeline, 2 around pipeline 0's trace phases only (light enough for a timed run). */
int pt_renderer_set_profiling(pt_renderer *r, int on);
/* Iterations in flight after allocate_on_gpu (config.pipelines clamped to 1..32, PT_PIPES overrides). */
int pt_renderer_pipelines(pt_renderer *r);
/* stats[0..6] = secondary-bounce ms, scan ms, primary ms, secondary-bounce launches,
 * scan launches, first-bounce ms, first-bounce launches (HIP events; resets). */
int pt_renderer_kernel_stats(pt_renderer *r, double stats[7]);
/* Same, n values: stats[7..8] = persistent-trace ms, launches (grid_fast / bvh split each
 * secondary bounce into a persistent trace + a shading pass; stats[0] is then the shading
 * pass); stats[9..10] = ray-sort ms, sort passes (k_sort_hist + prefix + scatter). */
int pt_renderer_kernel_stats_ex(pt_renderer *r, double *stats, int n);
/* Test hooks: primary-hit cache and batch intersection (host arrays). */
int pt_renderer_primary_hits(pt_renderer *r, float *dist, float *normal, int *model);
int pt_renderer_intersect_rays(pt_renderer *r, int n, const float *orig, const float *dir,
                               float *dist, float *normal, int *model);
/* Test hook (grid_fast): k_trace_gf's walk certificates (walk_certify_fast,
 * walk_certify) against the exact stepped walk on the same hit sets of each ray;
 * out4[4i..4i+3] = fast certificates tried, accepted, accepted-but-wrong,
 * full certificates accepted-but-wrong (no counterpart in the reference: it
 * checks the exactness of Renderer.cpp:238-360's replacement). */
int pt_renderer_certify_check(pt_renderer *r, int n, const float *orig, const float *dir, int *out4);
/* Test hook (PT_ACCEL_BVH / PT_ACCEL_GRID_FAST with the split trace): runs a caller's ray
 * batch through the persistent trace kernels as bounce 1 of an iteration runs them.  The
 * n rays are written as bounce 0's survivors into pipeline 0's ray pool: block b (of `chunk`
 * = config.block positions) holds block_counts[b] rays, ray k at the k-th occupied position
 * in block order; block_counts = NULL: full blocks, then the remainder.  Then the real
 * k_scan, the ray sort (when on) and the trace launches allocate_on_gpu picked (tails and
 * k_trace_deferred included) run on the renderer's stream, and ray k's hit record is read
 * back as the shading pass reads it: world distance (FLT_MAX: miss), world normal, model
 * (-1: miss) and the scene triangle index.  Refused (negative return, message) before any
 * launch: not allocated, another accel, PT_GF_SPLIT=0 / PT_TRACE_SPLIT=0, n outside
 * [0, width*height] (less the dropped tail with tail_drop), a count outside [0, chunk],
 * counts that do not sum to n, n_blocks > ceil(width*height / chunk).  The image, the
 * primary-hit cache and pt_renderer_segments / _segments_per_bounce are unchanged (but the
 * deferred-ray slot and the fault counter, which count this trace too); fails like
 * pt_renderer_synchronize when a trace gave up.  Zero-length and non-finite directions
 * are outside the hook's contract, as they are outside the renderer's (ABI 9). */
int pt_renderer_trace_rays(pt_renderer *r, int n, const float *orig, const float *dir,
                           const int *block_counts, int n_blocks,
                           float *dist, float *normal, int *model, int *tri);

/* ---- Noise estimate and render-until-converged (no counterpart in the reference,
 * which always renders ITER samples).  Off unless pt_renderer_enable_moments is
 * called: a render then launches, allocates and computes exactly what it did. ---- */
#define PT_NOISE_TILE 16
/* Keep, beside the image, the per-pixel sum of squared contributions (W*H*3 floats):
 * one fused pass per iteration adds a contribution c to the image and c*c to the
 * moments, in iteration order, so both are bit-reproducible and the same for every
 * pipeline count; the image is unchanged.  device_m2 = NULL: the renderer allocates
 * the buffer; otherwise the caller owns it, as with pt_renderer_bind_image (16-byte
 * aligned image and moment buffers take the wide-access kernel).  Costs 12 bytes per
 * pixel, plus one contribution buffer of the same size when pipelines == 1.  Must be
 * called before pt_renderer_allocate_on_gpu ("enable_moments must precede
 * allocateOnGPU").  pt_renderer_clear_image zeroes the moments and the sample count
 * (iterations enqueued since allocate_on_gpu or the last clear); pixels dropped by
 * tail_drop keep moment 0.  No counterpart in the reference. */
int pt_renderer_enable_moments(pt_renderer *r, float *device_m2);
/* The moments, ordered and fault-checked like pt_renderer_read_image; fails with
 * "moments not enabled" when they are off.  No counterpart in the reference. */
int pt_renderer_read_moments(pt_renderer *r, float *host_m2);
/* Relative noise of the accumulated image from S = image, Q = moments and
 * nf = (float)samples (samples <= 0: the sample count; fewer than 2 is refused with
 * "need at least 2 samples").  Per pixel, in float32 and in this order:
 *   for k in r,g,b:  m_k = S_k / nf;  q = Q_k / nf;  v = q - m_k*m_k;  v = v > 0 ? v : 0;
 *                    e_k = sqrtf(v / (nf - 1.0f));         (standard error of the mean)
 *   err = ((e_r + e_g) + e_b) / (((m_r + m_g) + m_b) + 0.01f);
 * Tiles are PT_NOISE_TILE x PT_NOISE_TILE pixels, ceil(W/16) x ceil(H/16), row-major,
 * partial in the last tile column and row: tile sum = sum of (double)err over its pixels,
 * tile_err = (float)(tile sum / pixels in the tile), *mean_err = (sum of tile sums) /
 * (W*H) in double, *max_tile_err = the largest tile_err; tile_err_host (may be NULL)
 * receives the tile map.  The reductions use no atomics: a run repeats bit for bit.
 * Runs on the renderer's stream, synchronizes, and fails like pt_renderer_read_image
 * after a trace fault.
 * Limit: the raw-moment variance q - m*m cancels in float32, with a floor of about
 * 1e-7 * m*m; this is an estimate to stop a render by, not a statistic.
 * No counterpart in the reference. */
int pt_renderer_noise(pt_renderer *r, int samples, double *mean_err, float *max_tile_err,
                      float *tile_err_host);
/* Renders iterations first_iter, first_iter + 1, ... in chunks of check_every (<= 0:
 * 32; the last chunk is cut at max_iters); after each chunk that brings this call's
 * count to max(min_iters, 2) or more it evaluates pt_renderer_noise over every sample
 * in the accumulator and stops when mean_err <= target.  Returns 1 converged, 0
 * max_iters reached, < 0 error; *iters_done = iterations this call rendered,
 * *mean_err = the last estimate (-1: fewer than 2 samples).  Each check costs a
 * synchronize and the start/end ramp of a render_loop call: check_every 32 keeps that
 * to a few percent of the chunk.  Moments must be enabled.  No counterpart in the
 * reference. */
int pt_renderer_render_until(pt_renderer *r, int first_iter, int min_iters, int max_iters,
                             int check_every, double target, int *iters_done, double *mean_err);

/* ---- Variance-guided edge-avoiding denoiser of the accumulated image (an a-trous
 * filter in the style of SVGF's spatial pass; no counterpart in the reference, which
 * writes the raw mean).  Needs pt_renderer_enable_moments.  A render that never calls it
 * allocates, launches and computes exactly what it did: the filter's buffers (56 bytes
 * per pixel) are allocated by the first call and freed with the renderer. ---- */
#define PT_DENOISE_MAX_PASSES 6
typedef struct pt_denoise_params {
    int passes;               /* a-trous passes, 1..PT_DENOISE_MAX_PASSES (default 5): pass s has taps 1 << s apart */
    float sigma_l, sigma_z;   /* luminance and depth stopping widths, finite and > 0 (defaults 4.0, 1.0) */
} pt_denoise_params;
void pt_default_denoise_params(pt_denoise_params *p);
/* Filters the mean image S / nf, guided by the variance of the mean from S = image and
 * Q = moments and by the primary-hit cache (depth d, world normal n, model k; the same
 * for every iteration: camera rays carry no jitter).  nf = (float)samples, resolved as in
 * pt_renderer_noise (samples <= 0: the sample count; fewer than 2 is refused with "need
 * at least 2 samples").  All arithmetic is float32 IEEE add, multiply, divide and square
 * root, in exactly this order; pixel index p = y*W + x.
 * Prep, per pixel:
 *   for k in r,g,b:  m_k = S_k / nf;  q = Q_k / nf;  v = q - m_k*m_k;  v = v > 0 ? v : 0;
 *                    v_k = v / (nf - 1.0f);
 *   c = (m_r, m_g, m_b);  V = (v_r + v_g) + v_b;
 *   pixels dropped by tail_drop (index >= the traced count) get k = -1, d = FLT_MAX like a miss;
 *   slope g = max(|d[y][x+] - d[y][x-]| * 0.5f, |d[y+][x] - d[y-][x]| * 0.5f), x+- = clamp(x +- 1,
 *   0, W-1), y+- = clamp(y +- 1, 0, H-1), whatever the neighbours' models.
 * Pass s = 0 .. passes-1, step = 1 << s, reads (c, V) of the previous pass and writes new ones.
 * H5 = {1/16, 1/4, 3/8, 1/4, 1/16}, G3 = {1/4, 1/2, 1/4}.  A pixel with k_p < 0 (miss or
 * dropped) copies its c and V in every pass and contributes to no other pixel.  Otherwise:
 *   Vbar = sum over j = -1..1 (outer), i = -1..1 of (G3[j+1]*G3[i+1]) * V[clamp(y+j)][clamp(x+i)],
 *          from 0.0f, any model;
 *   L_p = (c_r + c_g) + c_b;  den_l = sigma_l * sqrtf(Vbar) + 1e-4f;  sw = sc[3] = sv = 0;
 *   for j = -2..2 (outer), i = -2..2, tap q = (x + i*step, y + j*step), skipped when outside the
 *   frame or k_q != k_p:
 *     centre (i == 0 && j == 0):  w = H5[2]*H5[2];
 *     else  dot = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z;  wn = dot > 0 ? dot : 0;
 *           wn = wn*wn, six times;  r = (float)(step * (|i| + |j|));
 *           a = (d_q - d_p) / (sigma_z * (g_p * r + 1e-3f * d_p));  wz = 1.0f / (1.0f + a*a);
 *           xl = (L_q - L_p) / den_l;  wl = 1.0f / (1.0f + xl*xl);
 *           w = (H5[j+2]*H5[i+2]) * ((wn * wz) * wl);
 *     sw += w;  sc[k] += w * c_q[k];  sv += (w*w) * V_q;
 *   c[k] = sc[k] / sw;  V = sv / (sw*sw).            (sw >= 9/64)
 * The result is the last pass's c (host_rgb, W*H*3 floats, may be NULL; device_rgb_out, W*H*3
 * floats of device memory, NULL: the result stays in the renderer's own buffer) and V (host_var,
 * W*H floats, may be NULL).  p = NULL: the defaults.  The image and the moments are not modified.
 * Runs on the renderer's stream, synchronizes, and fails like pt_renderer_read_image after a
 * trace fault.  No atomics: a call repeats bit for bit.  Passes with step <= PT_DENOISE_LDS
 * (environment, read at every call: 0, 1, 2, 4 or 8; default 4) stage their tile in LDS, the
 * others read their taps from global memory; the results are the same for every value
 * (another value is refused: "PT_DENOISE_LDS must be 0, 1, 2, 4 or 8").
 * Refused before any launch: null renderer, "not allocated", "moments not enabled", "need at
 * least 2 samples", "bad denoise parameters" (passes outside 1..6, a sigma not finite and > 0).
 * Limits: it filters the accumulator's sqrt(color) space; inside one model only the luminance
 * term stops at reflections; silhouette pixels have a large slope and so little depth stopping.
 * No counterpart in the reference. */
int pt_renderer_denoise(pt_renderer *r, int samples, const pt_denoise_params *p,
                        float *device_rgb_out, float *host_rgb, float *host_var);
/* pt_renderer_denoise, then the BMP of the denoised mean D with pt_renderer_render_image's
 * conversion: bytes (int)(D * 255.0f) & 0xFF, rows bottom-up.  No counterpart in the reference. */
int pt_renderer_render_image_denoised(pt_renderer *r, const char *bmp_path, int samples,
                                      const pt_denoise_params *p);
/* HIP-event times in ms of the last pt_renderer_denoise or pt_renderer_denoise_ex made with
 * pt_renderer_set_profiling on: ms[0] prep, ms[1..6] the passes (0: not run), ms[7] the copy into
 * device_rgb_out, ms[8] first kernel to last, ms[9] the remodulation of PT_DENOISE_DEMODULATE (0:
 * not run); n values (0 beyond 10).  No counterpart in the reference. */
int pt_renderer_denoise_times(pt_renderer *r, double *ms, int n);

/* ---- The denoiser with options: albedo demodulation, and per-tile sample counts (added within
 * ABI 9: new functions only; pt_renderer_denoise, pt_denoise_params and PT_ABI_VERSION are
 * unchanged, and a caller who never uses these allocates, launches and computes what it did.  No
 * counterpart in the reference). ----
 * pt_renderer_denoise_ex with flags == 0 is pt_renderer_denoise: the same launches and the same
 * bits.  Otherwise it is pt_renderer_denoise's definition above with the changes below, float32
 * IEEE in exactly this order, no fused multiply-add.
 * PT_DENOISE_DEMODULATE.  The image holds sqrt(color) per channel, and the first shade of a
 * DIFFUSE, METAL, COAT, EMISSIVE or REFLECTIVE hit multiplies the colour by the albedo mc, so a
 * pixel's contribution is sqrt(mc) * sqrt(rest), channel by channel: the albedo divides out
 * exactly.  For pixel p with guide model k_p >= 0 let A be the three floats
 * pt_renderer_primary_albedo reports for p (the albedo plane's value when the allocation has
 * textures, otherwise the colour of model k_p).  Per channel:
 *   t = A > 0 ? A : 0    (a NaN gives 0);   sa = sqrtf(t);   e = sa > 1e-3f ? sa : 1e-3f
 * For k_p < 0 (a miss, or a pixel tail_drop left out) sa = e = 1.0f: such a pixel shows the
 * environment and is not demodulated.  Prep computes m_k and v_k as above, then
 *   c_k = m_k / e_k;   v'_k = v_k / (e_k * e_k)   (the product rounded first);
 *   V = (v'_r + v'_g) + v'_b
 * The passes are unchanged: every guide, weight and the luminance L is taken from the demodulated
 * c.  After the last pass  D_k = c_k * sa_k.  Multiplying by sa, not e, keeps a black texel black
 * when its neighbours bleed irradiance into it.  The result everywhere (the renderer's own
 * buffer, device_rgb_out, host_rgb, the BMP) is D; host_var is the last pass's V, in demodulated
 * units.  The floor 1e-3 is part of the definition, like den_l's 1e-4: a sqrt-space albedo of
 * 1e-3 is below a quarter of one output byte step (D * 255).
 * PT_DENOISE_TILE_COUNTS.  nf of pixel (x, y) is (float)counts[(y/16)*tiles_x + x/16], the counts
 * pt_renderer_sample_counts reports, wherever prep uses nf (nf - 1.0f included); the passes are
 * unchanged.  This is how an image of masked or adaptive iterations is denoised.
 * Refused before any launch: pt_renderer_denoise's refusals with the same text (without
 * PT_DENOISE_TILE_COUNTS, mixed sample counts included); "denoise_ex: unknown flag bits";
 * "denoise_ex: PT_DENOISE_TILE_COUNTS takes every tile's own sample count; samples must be <= 0";
 * "denoise_ex: PT_DENOISE_TILE_COUNTS needs at least 2 samples in every tile";
 * "denoise_ex: PT_DENOISE_DEMODULATE needs max_bounces >= 1 (without a bounce no hit multiplies
 * by its albedo)".
 * Cost: no buffer beyond pt_renderer_denoise's; demodulation reads 16 bytes more per pixel in
 * prep (the albedo plane; without textures the model's colour) and adds one launch that
 * multiplies the result in place; the counts are one int per tile, uploaded per call.  No
 * atomics: a call repeats bit for bit.  PT_DENOISE_LDS keeps its meaning.
 * Limits.  Under pixel jitter or a lens the albedo is the pinhole centre ray's, like the other
 * guides: a defocused or jittered textured region is demodulated with an albedo that its samples
 * did not all see (without PT_DENOISE_SAMPLED_GUIDES; with it the albedo is the mean over the
 * samples' own first hits, see pt_renderer_enable_guides).  Only the first hit's albedo is removed: a texture seen in a mirror is filtered
 * as before.  A first hit on a SPECULAR or REFRACTIVE model, whose shade multiplies by nothing, is
 * divided by an albedo its samples do not contain and multiplied by it again: harmless for a
 * plain colour, a reason to leave the flag off for a textured model of such a material. */
#define PT_DENOISE_DEMODULATE  1   /* filter the image divided by the primary hit's sqrt(albedo) */
#define PT_DENOISE_TILE_COUNTS 2   /* nf per pixel = its 16x16 tile's own sample count */
#define PT_DENOISE_SAMPLED_GUIDES 4 /* guides = means of the samples' first hits (pt_renderer_enable_guides) */
int pt_renderer_denoise_ex(pt_renderer *r, int samples, const pt_denoise_params *p, int flags,
                           float *device_rgb_out, float *host_rgb, float *host_var);
/* pt_renderer_denoise_ex, then the BMP of D as pt_renderer_render_image_denoised writes it. */
int pt_renderer_render_image_denoised_ex(pt_renderer *r, const char *bmp_path, int samples,
                                         const pt_denoise_params *p, int flags);

/* ---- Sampled first-hit guides (added within ABI 9: new functions and one new flag bit only;
 * PT_ABI_VERSION is unchanged.  No counterpart in the reference).  Off unless enabled: a renderer
 * that never calls pt_renderer_enable_guides allocates, launches and computes exactly what it did.
 * Under pixel jitter or a lens the primary-hit cache, the unjittered pinhole ray's hit, is not what
 * a pixel's samples saw.  With guides on, every generated iteration (one whose camera rays
 * k_gen_jitter / k_gen_camera emit: the jitter on, or lens_radius > 0) adds one record g per
 * emitted ray to G, a per-pixel record of 8 floats, 32 bytes, interleaved; for pixel p
 *   G[8p .. 8p+7] = (Nx, Ny, Nz, Z, Ar, Ag, Ab, Hc)
 * float32 IEEE, in this order, no fused multiply-add.  The ray's first hit is pass 1's hit record
 * (distance t, model m, triangle tri):
 *   hit (m >= 0):  n = the world normal pass 1's shade uses (the transformed triangle normal, or
 *                  pt_scene_set_model_smooth's interpolated one); mc = the albedo of
 *                  pt_scene_set_model_texture's definition (the model's colour without a texture);
 *                  pos(a) = a > 0 ? a : 0;
 *                  g = (n.x, n.y, n.z, t, sqrtf(pos(mc.r)), sqrtf(pos(mc.g)), sqrtf(pos(mc.b)), 1.0f)
 *   miss:          g = eight zeros
 * G[p] += g, one add per float, in iteration order: like S and Q the sums do not depend on the
 * pipeline count, and a run repeats bit for bit (no atomics).  A pixel that emitted no ray (a tile
 * a mask switched off, a pixel tail_drop left out) receives nothing.  The square root of the
 * albedo is summed because a sample's contribution is sqrt(mc) * sqrt(rest).  Ordinary iterations
 * (pinhole, jitter off) add nothing; the renderer counts per tile the samples that did
 * (pt_renderer_guide_counts), beside pt_renderer_sample_counts.
 * pt_renderer_enable_guides: before allocate_on_gpu.  device_ptr is a caller-owned device buffer of
 * W*H*8 floats (4-byte alignment suffices; 16-byte alignment takes the faster merge), NULL: the
 * renderer allocates it.  Refused for a null renderer and after allocation.  allocate_on_gpu then
 * refuses guides without pt_renderer_enable_moments, and (a limit) guides without the split trace,
 * whose hit records they read: PT_ACCEL_GRID, PT_GF_SPLIT=0 or PT_TRACE_SPLIT=0.
 * pt_renderer_read_guides copies G to the host (it waits for the renderer's stream);
 * pt_renderer_guide_counts writes tiles_y * tiles_x counts (NULL: none) and returns that number.
 * pt_renderer_clear_image, and every call that does what it does (pt_renderer_set_camera, a new
 * environment), zeroes G and the guide counts too.
 * PT_DENOISE_SAMPLED_GUIDES (pt_renderer_denoise_ex, pt_renderer_render_image_denoised_ex; free to
 * combine with the other two flags) changes prep alone; the passes and PT_DENOISE_LDS are
 * untouched.  With nf the pixel's sample count (per tile under PT_DENOISE_TILE_COUNTS) and h = Hc:
 *   validity, model:  k = h > 0 ? 0 : -1: the passes' model test becomes "both pixels saw a
 *                     surface", and a pixel no sample hit copies through as a miss does
 *   depth:            d = h > 0 ? Z / h : FLT_MAX; the slope g from these d by the same formula
 *   normal:           n = (Nx / h, Ny / h, Nz / h), not renormalised: a pixel that mixes
 *                     orientations has a short normal, its dot^64 weight to every neighbour falls,
 *                     and it is filtered less, never across
 *   demodulation (with PT_DENOISE_DEMODULATE), per channel:
 *                     sa = (A + (nf - h)) / nf  (the sum rounded before the division: a sample
 *                     that missed counts as albedo 1);  e = sa > 1e-3f ? sa : 1e-3f;
 *                     c, v' and D = c * sa as defined above, with this sa also where h = 0
 * Refused before any launch: "guides not enabled" (a renderer without pt_renderer_enable_guides
 * knows the bit no more than it did: the message begins "denoise_ex: unknown flag bits" and names
 * the reason); with samples <= 0, a tile whose guide count
 * differs from its sample count (every sample since the last clear must be a generated iteration);
 * with samples > 0 the caller vouches for that, as for sharded sums.
 * Memory: 32 bytes per pixel for G and 32 per pixel per pipeline for the per-iteration records: at
 * 1280 x 1024 42 MB + 16 x 42 MB = 713 MB when on, 0 when off.
 * Limits.  The model test is hit / no hit: two models that meet at equal depth and normal are
 * separated by the luminance term alone.  Only generated iterations accumulate.  No guides on the
 * fused or list-walking trace paths.  Only the first hit's albedo is removed, as before. */
int pt_renderer_enable_guides(pt_renderer *r, void *device_ptr);
int pt_renderer_read_guides(pt_renderer *r, float *out);
int pt_renderer_guide_counts(pt_renderer *r, int *tiles);

/* ---- Tile-masked sampling and the adaptive render (added within ABI 9: new functions only;
 * pt_render_config and PT_ABI_VERSION are unchanged.  No counterpart in the reference, which
 * gives every pixel ITER samples).  Off unless called: a renderer that never calls them
 * allocates, launches and computes exactly what it did.  Needs pt_renderer_enable_moments.
 * Tiles are the noise estimate's: PT_NOISE_TILE pixels square, tiles_x = ceil(W/16),
 * tiles_y = ceil(H/16), row-major, partial in the last column and row. ---- */
/* Enqueues iterations [first_iter, first_iter + n_iters) that sample only the tiles whose
 * byte in tile_mask_host (tiles_y * tiles_x bytes) is non-zero; NULL: every tile.  The mask
 * is copied before the call returns; the upload is ordered on the renderer's stream, so
 * successive calls with different masks and no synchronize each render under their own.
 * One masked iteration: at bounce 0 a pixel of an active tile does what it does in
 * pt_renderer_render_loop (camera ray, cached primary hit, shading with RNG slot = pixel
 * index, stable compaction); a pixel of an inactive tile emits no ray and contributes 0.0,
 * which leaves its sum S (image) and Q (moments) bit-identical.  From bounce 1 on a
 * survivor's slot, the RNG seed, is its rank among the survivors of the active tiles, so
 * under a partial mask a pixel draws other samples than in a full iteration: equally valid
 * samples of the same estimator, not the same ones.  With an all-ones mask or NULL the
 * result equals pt_renderer_render_loop's bit for bit.  Pixels dropped by tail_drop stay
 * dropped.  A mask with no active tile, or n_iters = 0, enqueues nothing and changes
 * nothing.  Masked iterations are enqueued directly also under PT_GRAPH=1: they are never
 * captured or replayed, and the graphs of pt_renderer_render_loop stay valid.
 * pt_renderer_segments keeps counting the frame's launched pixels as bounce 0's rays of a
 * masked iteration (the scan that counts them is unchanged); bounces >= 1 count the live
 * rays.  The sample count of pt_renderer_noise (iterations enqueued) grows by n_iters;
 * each active tile's count below grows by n_iters.
 * Errors: not allocated, "moments not enabled ...", "bad iteration range". */
int pt_renderer_render_loop_masked(pt_renderer *r, int first_iter, int n_iters,
                                   const unsigned char *tile_mask_host);
/* Samples per tile since allocate_on_gpu or the last clear_image (tiles_y * tiles_x ints,
 * may be NULL): pt_renderer_render_loop adds its n to every tile, a masked call to the
 * active ones.  Returns the tile count.  Once the counts differ between tiles,
 * pt_renderer_noise, pt_renderer_denoise, pt_renderer_render_image_denoised with
 * samples <= 0 and pt_renderer_render_until fail with a message naming the calls below;
 * with samples > 0 they compute what they always did from S, Q and that number. */
int pt_renderer_sample_counts(pt_renderer *r, int *tile_counts_host);
/* pt_renderer_noise with nf = (float)count[tile] for the pixels of each tile: the same
 * per-pixel expression in the same float32 order, the same fixed-order double sums, no
 * atomics (a call repeats bit for bit).  A tile with fewer than 2 samples has tile_err
 * +inf (*max_tile_err is then +inf) and adds nothing to *mean_err's sum, which is still
 * divided by W*H. */
int pt_renderer_adaptive_noise(pt_renderer *r, double *mean_err, float *max_tile_err,
                               float *tile_err_host);
/* The mean image S / (float)count[tile], 0 where the count is 0, W*H*3 floats into
 * device_rgb_out (device memory, may be NULL) and/or host_rgb (may be NULL).  16-byte
 * aligned buffers take the wide-access kernel.  Runs on the renderer's stream and
 * synchronizes. */
int pt_renderer_adaptive_mean(pt_renderer *r, void *device_rgb_out, float *host_rgb);
/* The BMP of that mean M with pt_renderer_render_image's conversion: bytes
 * (int)(M * 255.0f) & 0xFF, rows bottom-up. */
int pt_renderer_render_image_adaptive(pt_renderer *r, const char *bmp_path);
/* Renders masked chunks of check_every iterations (<= 0: 32; the last chunk is cut at
 * max_iters), every tile active at first.  After each chunk that brings this call's count
 * to max(min_iters, 2) or more it evaluates pt_renderer_adaptive_noise over every sample in
 * the accumulator and switches off each active tile with tile_err <= tile_target; a tile
 * switched off stays off for the rest of the call.  Returns 1 when no tile is active, 0 when
 * max_iters is reached first, < 0 on error.  *iters_done = iterations this call rendered,
 * *pixel_samples = sum over chunks of (pixels of the active tiles, dropped ones included)
 * x chunk length, *mean_err = the last estimate's frame mean.  Each check synchronizes and
 * reads the tile map back, as pt_renderer_render_until does.
 * Known bias: a tile is stopped on an estimate made from the very samples it keeps, so
 * tiles that look quiet by chance stop early and stay that way; min_iters is the guard.
 * Like the "Limit" of pt_renderer_noise, this is a budget heuristic, not a statistic. */
int pt_renderer_render_adaptive(pt_renderer *r, int first_iter, int min_iters, int max_iters,
                                int check_every, double tile_target,
                                int *iters_done, long long *pixel_samples, double *mean_err);

/* ---- Pixel-jittered camera rays (anti-aliasing; added within ABI 9: new functions only,
 * pt_render_config and PT_ABI_VERSION are unchanged.  No counterpart in the reference, whose
 * camera rays are the same every iteration, so its silhouettes are stair-stepped at any
 * sample count).  Off by default: a renderer that never turns it on allocates, launches and
 * computes exactly what it did. ---- */
/* Host state: it applies to the iterations enqueued after the call, and may be set before or
 * after allocate_on_gpu and between render calls without a synchronize.  While on,
 * pt_renderer_render_loop, _render_loop_masked, _render_until and _render_adaptive all enqueue
 * jittered iterations.  width is the side of the square, in pixels, the ray's point is drawn
 * from, centred on the point the unjittered ray goes through (1.0: the pixel's own extent).
 * One jittered iteration `it`, for launched pixel p = y*W + x (pixels dropped by tail_drop
 * stay dropped), float32 IEEE in exactly this order, no fused multiply-add:
 *   ux = the first uniform of the reference's engine seeded (it, p, max_bounces + 1)
 *   uy = the first uniform of the engine seeded (it, p, max_bounces + 2)
 *        (depths the shading never seeds with; the index is the pixel, not the pool slot)
 *   fx = (float)x + width * (ux - 0.5f);   fy = (float)y + width * (uy - 0.5f)
 *   wx = (float)(plane_x0 + (double)(fx * step_x));  wy = (float)(plane_y0 + (double)(fy * step_y))
 *   origin = cam;  direction = (wx, wy, plane_z) - cam (not normalised);  color = 1;
 *   bounces = max_bounces
 * The rays, in ascending pixel order, are bounce 0's survivors: the ray of rank k sits at
 * dense slot k.  Nothing is intersected or shaded at bounce 0.  Then come the ordinary passes
 * b = 1 .. max(max_bounces, 1): ray sort (when on), trace, shade, compaction -- so a ray gets
 * as many shades as in pt_renderer_render_loop, and each pixel still contributes exactly once
 * per iteration.  The RNG slot of a ray's first shade is its rank, which with every tile
 * active is its pixel index, as in render_loop.  The generated rays are in pixel order
 * already, so the trace of pass 1 claims them unsorted; PT_JITTER_SORT=1 (environment, read
 * by allocate_on_gpu) sorts them like every later pass's.  The results are the same.
 * Width 0: x + 0 * (u - 0.5f) is x, so on with width 0 reproduces render_loop bit for bit.
 * Masks: under a tile mask (moments required, as ever) a pixel of an inactive tile emits no
 * ray and contributes 0.0.  Sharding: the offset depends on (iteration, pixel) only, so
 * sharding the iterations across ranks stays exact.
 * Unchanged: the primary-hit cache is still built once; pt_renderer_primary_hits, the
 * denoiser's guides and unjittered iterations read it.  Limit: the denoiser's guides are thus
 * the hit of the unjittered ray, so an anti-aliased edge pixel, a mix of two surfaces, is
 * filtered with the guides of one of them (flags without PT_DENOISE_SAMPLED_GUIDES; with
 * pt_renderer_enable_guides and that flag the guides are the means over the jittered samples'
 * own first hits).  pt_renderer_segments counts a jittered iteration's
 * generated rays as bounce 0 (the frame's launched pixels, as for masked iterations) and its
 * traced camera rays as bounce 1: the launched-pixel count more per iteration than
 * render_loop.  Jittered iterations are enqueued directly also under PT_GRAPH=1: never
 * captured or replayed, and the graphs of the unjittered loop stay valid.
 * Refused before any launch: a null renderer; a width that is not finite or is negative;
 * turning it on when max_bounces + 2 > 511 (the seeding word's depth field). */
int pt_renderer_set_pixel_jitter(pt_renderer *r, int on, float width);
/* The current setting (either pointer may be NULL); off and width 1.0 until set. */
int pt_renderer_pixel_jitter(pt_renderer *r, int *on, float *width);

/* ---- Free camera with a thin lens: look-at views and depth of field (added within ABI 9:
 * new functions only, pt_render_config and PT_ABI_VERSION are unchanged.  No counterpart in
 * the reference, whose generateRaysKernel looks down -z through one axis-aligned rectangle).
 * Off by default: a renderer that never sets a camera allocates, launches and computes
 * exactly what it did, through the config's legacy camera. ---- */
typedef struct pt_camera {
    float origin[3];              /* centre of the lens */
    float p0[3];                  /* world point the ray of pixel coordinates (0, 0) goes through */
    float du[3], dv[3];           /* world step per pixel in x and in y; the plane they span is the plane in focus */
    float lens_u[3], lens_v[3];   /* two vectors spanning the lens (unit length for a round lens) */
    float lens_radius;            /* 0: pinhole */
} pt_camera;
/* Sets the view of the iterations enqueued after the call; cam = NULL: back to the config's
 * legacy camera.  The ray through pixel coordinates (fx, fy), for launched pixel p = y*W + x in
 * iteration `it`, float32 IEEE in exactly this order, no fused multiply-add:
 *   t_k = (p0_k + fx*du_k) + fy*dv_k                      k = x, y, z
 *   pinhole:  o = origin
 *   lens:     u1 = the first uniform of the reference's engine seeded (it, p, max_bounces + 3)
 *             u2 = the first uniform of the engine seeded (it, p, max_bounces + 4)
 *                  (two more depths the shading never seeds with; the index is the pixel)
 *             rr = lens_radius * sqrtf(u1);  phi = 6.2831855f * u2
 *             a = rr * cosf(phi);  b = rr * sinf(phi)     (the kernels' sinf / cosf, pt_selftest_math)
 *             o_k = (origin_k + a*lens_u_k) + b*lens_v_k
 *   direction = t - o (not normalised);  color = 1;  bounces = max_bounces
 * (fx, fy) is ((float)x, (float)y) with the pixel jitter off and pt_renderer_set_pixel_jitter's
 * x + width * (ux - 0.5f), y + width * (uy - 0.5f) with it on.
 * Which iterations take which path.  A pinhole with the jitter off renders through the ordinary
 * loop: the camera ray of bounce 0 takes the form above, and the primary-hit cache, tile masks,
 * PT_GRAPH=1 replay and the denoiser's guides work as they do for the legacy camera.  With the
 * jitter on or lens_radius > 0 an iteration is a jittered iteration: its rays are generated as
 * bounce 0's survivors (with a lens and the jitter off the two jitter draws are not made), then
 * come passes 1 .. max(max_bounces, 1); masks, the RNG slots, the segment accounting (the
 * launched-pixel count more per iteration) and the direct enqueue under PT_GRAPH=1 are the
 * jittered iteration's.
 * The legacy-equivalent camera -- origin = cam, p0 = (plane_x0, plane_y0, plane_z),
 * du = ((float)(plane_w / W), 0, 0), dv = (0, (float)(plane_h / H), 0) -- has the legacy camera's
 * rays bit for bit, plain and jittered, whenever cam, plane_x0, plane_y0 and plane_z are
 * float-representable (the default config's are).
 * The primary-hit cache is always the hit of the pinhole ray through the pixel's own point.
 * Limit: the denoiser's guides under a lens are thus the pinhole's, so a defocused pixel, a mix
 * of surfaces, is filtered with the guides of the surface its centre ray hits (flags without
 * PT_DENOISE_SAMPLED_GUIDES; with pt_renderer_enable_guides and that flag the guides are the
 * means over the lens samples' own first hits).
 * May be called before or after allocate_on_gpu.  After it the call is ordered on the renderer's
 * stream after everything enqueued (no synchronize is needed between render calls and view
 * changes; with PT_GRAPH=1 graphs in flight are waited for), invalidates the primary-hit cache,
 * which the next render call rebuilds as the first one does, drops the captured graphs, and does
 * what pt_renderer_clear_image does: a new view is a new render.
 * Refused with a message before anything changes: a null renderer; "set_camera: every field must
 * be finite"; "set_camera: du and dv must not be zero"; "set_camera: lens_radius must be >= 0";
 * lens_radius > 0 when max_bounces + 4 > 511 (the seeding word's depth field). */
int pt_renderer_set_camera(pt_renderer *r, const pt_camera *cam);
/* The current view (out may be NULL): returns 1 when a camera is set, 0 for the legacy camera,
 * for which *out receives the legacy-equivalent camera above. */
int pt_renderer_camera(pt_renderer *r, pt_camera *out);
/* A look-at view for a W x H frame (host only; computed in double, each field rounded once to
 * float):  f = normalize(target - eye);  r = normalize(f x up);  u = r x f;
 * hh = focus_dist * tan(vfov / 2);  hw = hh * W / H;  du = r * 2hw / W;  dv = u * 2hh / H;
 * p0 = eye + f * focus_dist - r * hw - u * hh;  origin = eye;  lens_u = r;  lens_v = u.
 * Pixel y grows along +u, as the legacy camera's grows along +y.  focus_dist places the plane in
 * focus; for a pinhole it only scales du, dv and p0 along their rays.
 * Refused: a null argument, a frame without pixels, a non-finite value, "look_at: eye and target
 * coincide", "look_at: up is parallel to the view", "look_at: vfov_deg must lie in (0, 180)",
 * "look_at: focus_dist must be > 0", "look_at: lens_radius must be >= 0". */
int pt_camera_look_at(const double eye[3], const double target[3], const double up[3], double vfov_deg,
                      double focus_dist, double lens_radius, int W, int H, pt_camera *out);
/* The view the config file's RENDER block set, for a W x H frame: returns 1 and fills *out, or 0
 * when the block set none (< 0: error).  Optional RENDER keys: camera_eye:[x,y,z] and
 * camera_target:[x,y,z] (both or neither), camera_up:[x,y,z] (default [0,1,0]), camera_fov:DEG
 * (vertical, default 45), camera_focus:D (default |target - eye|), camera_lens:R (default 0).
 * pt_render and the command-line renderer apply it. */
int pt_scene_camera(const pt_scene *s, int W, int H, pt_camera *out);

/* ---- Environment lighting: an octahedral sky map for the rays that miss (added within ABI 9:
 * new functions only, pt_render_config and PT_ABI_VERSION are unchanged.  No counterpart in
 * the reference, whose shadeRayKernel gives a missing ray the constant 0.01).  Off by default:
 * a renderer that never sets an environment computes exactly what it did. ---- */
typedef struct pt_environment {
    int n;                        /* the map is n x n texels, 1 <= n <= 2048 */
    const float *texels_rgb;      /* n*n*3 floats, octahedral layout: texel (row y, column x) at 3*(y*n + x) */
    float scale[3];               /* multiplies the interpolated texel, per channel */
    float rotation[9];            /* row-major, world -> environment frame; the frame's +z is the map's centre */
} pt_environment;
/* Sets what a ray that leaves the scene brings back, for the iterations enqueued after the
 * call; env = NULL: back to the constant 0.01.  Only the colour of a ray that has already missed
 * changes: no trace, no random draw, no slot, no compaction order and no segment count does.
 * For a missing ray of direction d (not normalised) and colour c, float32 IEEE in exactly this
 * order, no fused multiply-add; T[y][x] is a texel, |.| clears the sign bit:
 *   u  = d * (1.0f / sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z))
 *   e_k = (rotation[3k]*u.x + rotation[3k+1]*u.y) + rotation[3k+2]*u.z          k = 0, 1, 2
 *   l  = (|e.x| + |e.y|) + |e.z|
 *   px = e.x / l;  py = e.y / l
 *   if (e.z < 0) { qx = (1.0f - |py|) * (px >= 0 ? 1.0f : -1.0f);
 *                  qy = (1.0f - |px|) * (py >= 0 ? 1.0f : -1.0f);  px = qx;  py = qy; }
 *   per axis p:  f = ((p * 0.5f + 0.5f) * (float)n) - 0.5f;  f = fminf(fmaxf(f, 0.0f), (float)(n - 1))
 *                i0 = (int)f;  i1 = min(i0 + 1, n - 1);  t = f - (float)i0
 *   per channel: top = T[y0][x0] + (T[y0][x1] - T[y0][x0]) * tx
 *                bot = T[y1][x0] + (T[y1][x1] - T[y1][x0]) * tx
 *                v   = top + (bot - top) * ty
 *   c = c * (v * scale);  the ray ends (bounces = 0)
 * The upper hemisphere (e.z >= 0) fills the diamond |px| + |py| <= 1 about the map's centre, the
 * lower one the four corners.  fmaxf / fminf drop a NaN, so a NaN coordinate (a zero direction)
 * reads texel (0, 0): no load leaves the map.
 * Limits.  The lookup is clamp-to-edge bilinear: the map's outer edge is a fold line of the lower
 * hemisphere, where the interpolation is off by at most half a texel (there is no octahedral
 * wrap).  The map is sampled by the paths alone (no importance sampling, no shadow rays), so a
 * small bright sun is noisy.  The image accumulates sqrt(colour) as before.
 * May be called before or after allocate_on_gpu.  After it the call waits for the renderer's
 * stream (which every render call has joined its pipelines into), uploads on that stream, drops
 * the captured graphs when the environment changes between NULL and set, and does what
 * pt_renderer_clear_image does: a new environment is a new render.  The segment counters and
 * the primary-hit cache stay.  The texels are copied: the caller's buffer is free after the call.
 * Refused with a message before anything changes: a null renderer; "set_environment: n must be
 * 1 .. 2048"; "set_environment: null texels"; "set_environment: every scale entry must be
 * finite"; "set_environment: every rotation entry must be finite"; "set_environment: every texel
 * must be finite". */
int pt_renderer_set_environment(pt_renderer *r, const pt_environment *env);
/* The current environment: returns 1 when one is set and 0 when none is (< 0: error).  *out (may
 * be NULL) receives n, scale and rotation, with texels_rgb = NULL; texels_out (may be NULL: ask
 * for n first) receives the n*n*3 texels. */
int pt_renderer_environment(pt_renderer *r, pt_environment *out, float *texels_out);
/* Test hook: the lookup above, without the final c * ..., on the device for `count` directions
 * dirs[3*count] -> rgb_out[3*count].  Needs allocate_on_gpu and an environment. */
int pt_renderer_env_lookup(pt_renderer *r, int count, const float *dirs, float *rgb_out);
/* The albedo mc (pt_scene_set_model_texture's definition) of each pixel's cached primary hit:
 * rgb_out[3*width*height], (0, 0, 0) for a miss and for a pixel tail_drop leaves out.  Works
 * without textures too, where it is the hit model's colour.  Needs allocate_on_gpu.  No
 * counterpart in the reference. */
int pt_renderer_primary_albedo(pt_renderer *r, float *rgb_out);
/* Test hook: that definition evaluated on the device for n caller-given hits: orig[3n], dir[3n],
 * and the dist[n], model[n], tri[n] pt_renderer_trace_rays returns -> rgb_out[3n].  An untextured
 * model gives its colour, model < 0 gives (0, 0, 0).  Refused before any launch: "hit_albedo:
 * model index out of range", "hit_albedo: triangle index out of range".  No counterpart in the
 * reference. */
int pt_renderer_hit_albedo(pt_renderer *r, int n, const float *orig, const float *dir, const float *dist,
                           const int *model, const int *tri, float *rgb_out);
/* Fills an n x n octahedral map with a sky (host only): texels_out[3*(y*n + x) + k], k = r, g, b.
 * Texel (y, x)'s centre is decoded to a direction, float32 in exactly this order:
 *   px = (((float)x + 0.5f) / (float)n) * 2.0f - 1.0f;  py likewise from y
 *   ez = (1.0f - |px|) - |py|;  ex = px;  ey = py
 *   if (ez < 0) { ex = (1.0f - |py|) * (px >= 0 ? 1.0f : -1.0f);
 *                 ey = (1.0f - |px|) * (py >= 0 ? 1.0f : -1.0f); }
 *   uz = ez * (1.0f / sqrtf((ex*ex + ey*ey) + ez*ez))
 *   texel_k = ez >= 0 ? horizon_k + (zenith_k - horizon_k) * uz : ground_k
 * The environment frame's +z is the zenith; pt_environment's rotation turns it to the world's up.
 * Refused: a null argument, n outside 1 .. 2048. */
int pt_environment_sky(const float zenith[3], const float horizon[3], const float ground[3], int n,
                       float *texels_out);
void pt_renderer_free(pt_renderer *r);

/* Device math conformance hook: evaluates the kernels' sinf/cosf/powf/sqrtf/div
 * replacements on n inputs (x, y) -> out[n*5] = sin(x) cos(x) pow(x,y) sqrt(x) x/y. */
int pt_selftest_math(int n, const float *x, const float *y, float *out);

/* Device conformance hook of the dielectric material: evaluates the definition above on n inputs,
 * one lane each, without a renderer.  dir (n*3) is normalised first, as the shading does; nrm
 * (n*3) and ior (n) are used as given; u (n) takes the place of the draw.  out_dir (n*3) is d';
 * out_event (n): 0 refraction entering, 1 refraction leaving, 2 Fresnel reflection, 3 total
 * internal reflection. */
int pt_selftest_dielectric(int n, const float *dir, const float *nrm, const float *ior, const float *u,
                           float *out_dir, int *out_event);

/* ---- Direct lighting: light sampling with shadow rays at diffuse hits (added; no counterpart in
 * the reference, whose paths carry light only when the random walk lands on an EMISSIVE triangle).
 * Opt-in: a renderer that never calls pt_renderer_set_direct_light allocates, launches and
 * computes exactly what it did, and so does one with the switch on in a scene without a light.
 *
 * Lights are the triangles of every EMISSIVE model, models in index order, each model's triangles
 * in mesh order.  The table holds per light, in world space: p0, e1, e2 (the first vertex and the
 * two edges), the unit normal nl, the area, the model index and the emission E (the model's
 * colour; two-sided, as the shade has no facing test); and A_total and a float32 cdf (the running
 * area sum over A_total, last entry 1).  Computed in double from the float32 vertices and
 * model_to_world, rounded once.  A zero-area triangle stays in the table and is never chosen.
 *
 * The estimator, float32, no contraction, in this order.  At every hit of a live ray (bounces > 0,
 * the count before the shade decrements it) on a MAT_DIFFUSE model -- COAT, METAL, REFLECTIVE and
 * DIELECTRIC hits sample nothing -- with ip the hit point, n the shading normal, mc the albedo and
 * c the ray's colour, all as the shade of that hit has them, and slot the slot that shade seeds
 * with (the pixel index at a cached primary hit, the dense slot otherwise):
 *   u0, u1, u2 = the first uniform of the engine seeded (iteration, slot, 256 + bounces),
 *                (iteration, slot, 320 + bounces), (iteration, slot, 384 + bounces)
 *   i  = the smallest index with u0 < cdf[i], else the last light
 *   s  = sqrtf(u1);  y = (p0 + e1 * (s * (1 - u2))) + e2 * (s * u2)
 *   x' = ip + n * 0.1f                               (the origin a scattered ray gets)
 *   w  = y - x';  r2 = dot(w, w);  r = sqrtf(r2);  wn = w * (1 / sqrtf(dot(w, w)))
 *   cx = dot(n, wn);  cy = fabsf(dot(nl, wn))
 *   unless (cx > 0 && cy > 0 && r2 > 0): nothing is added, no shadow ray is traced (a NaN fails)
 *   g  = ((cx * cy) / (pi * r2)) * A_total;  Dc = ((c * mc) * E) * g      per channel
 *   the shadow ray runs from x' along wn with tmax = r * 0.999f; it is occluded if and only if
 *   some triangle of some model that the reference's triangle test accepts lies at a world
 *   distance (the closest-hit query's distance of that triangle) below tmax -- PT_ACCEL_BVH's
 *   exact semantics for every accel; the grid's early exit never applies to a shadow ray
 *   unoccluded: D[pixel] += Dc
 * A ray that hits an EMISSIVE model directly after a DIFFUSE vertex contributes nothing for that
 * hit (the vertex before it sampled the lights); emission reached from the camera or through
 * COAT, METAL, REFLECTIVE or DIELECTRIC counts as it did.  Per pixel and iteration, with t the
 * value the path's end writes (sqrtf of the terminal colour) and t' = 0 where that terminal was
 * such a suppressed hit, else t:  sample = (D == 0) ? t' : sqrtf(t' * t' + D)  per channel, which
 * goes into the image and its square into the moments.  A pixel that received no direct light
 * keeps the bits it had.
 * Limits: no multiple importance sampling, so the 1 / r2 term is unbounded close to a light (a
 * diffuse surface next to a lamp shows bright outliers); the environment map is not sampled;
 * COAT and METAL hits do not sample; emission textures are refused.
 *
 * pt_renderer_set_direct_light: before or after allocate_on_gpu; after it, a change clears the
 * accumulators as pt_renderer_set_environment does and drops captured graphs.  Refused with a
 * message, before any launch (here when the renderer is allocated, else at allocate_on_gpu):
 * PT_ACCEL_GRID or a fused trace (PT_TRACE_SPLIT=0 / PT_GF_SPLIT=0); moments not enabled; an
 * EMISSIVE model with a texture; max_bounces > 63 (the depth codes above would meet the shade's
 * and the jitter's).
 * pt_renderer_direct_light: the switch, and the allocation's light count and A_total (0 before).
 * pt_scene_lights / pt_renderer_lights: the table of a scene / of the renderer's allocation, up to
 * max_lights records of PT_LIGHT_FLOATS floats: p0[3], area, e1[3], model (an int's bits), e2[3],
 * cdf, nl[3], 0, E[3], 0; *area_total = A_total; returns the number of lights.
 * pt_scene_direct_light: 1 when the scene file's RENDER block says direct_light: 1.
 * pt_renderer_occluded (test hook): n segments orig -> target (n*3 floats each) as shadow rays,
 * direction the normalised difference and tmax = 0.999f * |target - orig|; out[i] = 1 occluded,
 * 0 not; a segment of zero length reads 0.  Needs a BLAS (not PT_ACCEL_GRID).
 * pt_renderer_direct_sample (test hook): the estimator for n caller-given hits: rays (orig, dir),
 * distance, model, scene triangle, colour c, and ids (iteration, slot, bounces) per hit; the
 * normal and the albedo are the shade's for such a hit.  out_f: 8 floats per hit (y[3], g, Dc[3],
 * 0); out_i: the light's index (-1: the geometry test failed, the rest is 0) and 1 if unoccluded. */
#define PT_LIGHT_FLOATS 20
int pt_renderer_set_direct_light(pt_renderer *r, int on);
int pt_renderer_direct_light(pt_renderer *r, int *on, int *n_lights, float *area);
int pt_scene_lights(const pt_scene *s, int max_lights, float *recs_out, float *area_total);
int pt_renderer_lights(pt_renderer *r, int max_lights, float *recs_out, float *area_total);
int pt_scene_direct_light(const pt_scene *s);
int pt_renderer_occluded(pt_renderer *r, int n, const float *orig, const float *target, int *out);
int pt_renderer_direct_sample(pt_renderer *r, int n, const float *orig, const float *dir, const float *dist,
                              const int *model, const int *tri, const float *color, const int *ids, float *out_f,
                              int *out_i);

/* main.cpp: load scene config, render cfg->iterations, write BMP. */
int pt_render(const char *scene_config, const pt_render_config *cfg, const char *bmp_out);

#ifdef __cplusplus
}
#endif
#endif
