/* winmad_rt.h -- C ABI of the MI355X-native BDPT / PT hot path.
 *
 * Drop-in boundary for winmad/Winmad-s-raytracer-v1.0 (paths below are relative
 * to /root/reference/Winmad-s-raytracer-v1.0/src).  The reference has no FFI;
 * its seam is the C++ class SurfaceIntegrator (surfaceIntegrator/surfaceIntegrator.h:14-34)
 * with Scene::intersect / Scene::occluded below it.  Each entry point names the
 * reference interface it replaces.  INTEGRATION.md shows the C++ / ctypes
 * bindings a maintainer adds on the reference side.
 *
 * Conventions (all functions):
 *   - return 0 on success, a negative WR_E* code on failure; never throw;
 *     the message of the last failure on this thread is wr_last_error();
 *   - plain pointers and sizes only; the caller owns every input / output buffer;
 *   - a wr_context is used by one host thread at a time; it owns its HIP streams
 *     on one device (wr_create) or on several (wr_create_multi).  Multi-GPU is
 *     either one process per GPU (wr_comm_* below) or one context over the
 *     node's GPUs (wr_create_multi); see DESIGN.md section 5.
 */
#ifndef WINMAD_RT_H
#define WINMAD_RT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WR_API_VERSION 8

enum {
  WR_OK = 0,
  WR_E_ARG = -1,      /* bad argument                                  */
  WR_E_IO = -2,       /* scene / obj file unreadable or malformed      */
  WR_E_HIP = -3,      /* HIP runtime error (no device, OOM, launch)    */
  WR_E_SCENE = -4,    /* scene lacks what the call needs (lights, ...) */
  WR_E_NODEVICE = -5  /* the HIP extension found no gfx950 device       */
};

typedef struct wr_scene wr_scene;     /* host-side loaded scene + KD tree */
typedef struct wr_context wr_context; /* scene resident in HBM + stream  */

/* Ray (geometry/ray.h:6-32).  `d` is used as given: callers normalise it as
 * the Ray constructor does (ray.h:14-21).  The reference always has tmin = 0,
 * tmax = INF (1e7). */
typedef struct {
  float o[3];
  float d[3];
  float tmin, tmax;
} wr_ray; /* 32 bytes */

/* Intersection (geometry/intersection.h:6-19) + index of the winning primitive
 * in the reference's `Scene::objs` order (-1 = miss). */
typedef struct {
  float t;
  float p[3];
  float n[3];
  int32_t prim;
  int32_t inside;
  int32_t mat_id;
} wr_hit; /* 40 bytes */

typedef struct {
  int32_t nprims, ntriangles, nspheres, nlights, nmaterials;
  int32_t kd_depth_max;   /* depMax = int(1.2 ln N + 2) (KDtreeAccel.cpp:16) */
  int32_t kd_inner, kd_leaves;
  int64_t kd_refs;
  int32_t kd_max_stack;   /* traversal stack depth bound                    */
  int32_t missing_files;  /* .obj files the reference would silently skip   */
  float camera_xres, camera_yres;
  int64_t device_bytes;   /* bytes this scene occupies in HBM               */
} wr_scene_info;

/* BidirPathTracing knobs (bidirPathTracing.cpp:5-21). */
typedef struct {
  int32_t width, height;     /* Parameters WIDTH / HEIGHT; the film is height x width x 3   */
  int32_t iterations;        /* samples per pixel = iterations (hard-coded 1 in the reference) */
  int32_t iter_begin;        /* global index of the first iteration (RNG key; sharding)     */
  int32_t control_length;    /* 3 = reference filter; <= 0 accumulates every path length     */
  int32_t max_path_length;   /* 10 in the reference                                          */
  uint32_t seed;
  int32_t faithful;          /* 1: trace every ray the reference traces (default);
                                0: skip shadow rays whose contribution is filtered out       */
  int32_t time_kernels;      /* 1: HIP events around every launch -> wr_stats.kernel_ms      */
  int32_t count_work;        /* 1: per-traversal node / ref counters -> wr_stats              */
} wr_bdpt_params;

/* PathIntegrator knobs (pathIntegrator.cpp:3-15, parameters.para). */
typedef struct {
  int32_t width, height;
  int32_t spp;               /* SAMPLES_PER_PIXEL: the stratification grid (surfaceIntegrator.cpp:26-32) */
  int32_t max_depth;         /* MAX_TRACING_DEPTH                                          */
  int32_t sample_begin;      /* first sample index k rendered (RNG key; sharding), >= 0    */
  int32_t sample_count;      /* samples rendered by this call (0: spp - sample_begin);
                                negative, or sample_begin + sample_count > spp: WR_E_ARG    */
  uint32_t seed;
  int32_t time_kernels;
  int32_t count_work;
} wr_path_params;

/* VertexCM knobs (surfaceIntegrator/vertexcm.cpp:3-21, :47-66).  The merge
 * radius of global iteration i is
 *   max(radius_factor * sceneRadius / (i + 1)^(0.5 (1 - radius_alpha)), EPS). */
typedef struct {
  int32_t width, height;
  int32_t iterations;        /* hard-coded 1 in the reference (:7)                   */
  int32_t iter_begin;        /* global index of the first iteration (RNG key, radius) */
  int32_t min_path_length;   /* 0 in the reference                                    */
  int32_t max_path_length;   /* 10 in the reference; at most 10                      */
  float radius_factor;       /* 0.003: baseRadius = factor * sceneSphere.sceneRadius  */
  float radius_alpha;        /* 0.75                                                  */
  uint32_t seed;
  int32_t time_kernels;
  int32_t count_work;
} wr_vcm_params;

enum { WR_K_TRACE = 0, WR_K_SHADE = 1, WR_K_RESOLVE = 2, WR_K_GEN = 3, WR_K_OTHER = 4, WR_K_NUM = 8 };

typedef struct {
  int64_t closest_rays;      /* Scene::intersect traversals                 */
  int64_t shadow_rays;       /* Scene::occluded traversals                  */
  int64_t inner_visits;      /* count_work only                             */
  int64_t leaf_visits;
  int64_t prim_refs;         /* = triangle / sphere tests                   */
  double seconds;            /* host wall time of the call (stream synced)  */
  double kernel_ms[WR_K_NUM];      /* time_kernels only: summed launch durations */
  int64_t kernel_launches[WR_K_NUM];
  double trace_wall_ms;      /* time_kernels only: union of the traversal launch
                                intervals over all pipelines (launches overlap) */
  int64_t vm_queries;        /* VCM: range queries (KdTree::searchInRadius calls)  */
  int64_t vm_found;          /* VCM: light vertices found within the radius       */
  int64_t vm_merged;         /* VCM: RangeQuery::process merges (non-black BSDF)   */
  int64_t prim_tests;        /* count_work only: primitive tests run; < prim_refs
                                by the (ray, primitive) repeats skipped            */
  /* WR_TRACE_BVH only (wr_set_trace_mode), count_work: verified-BVH work.  The
   * KD counters above then cover only the fallback rays.                       */
  int64_t bvh_nodes;         /* BVH nodes visited (64-byte records)             */
  int64_t bvh_tests;         /* triangle tests of the BVH search                */
  int64_t kd_replay_steps;   /* KD path entries replayed (membership checks)    */
  int64_t fallback_rays;     /* rays handed to the faithful KD traversal        */
  /* WR_TRACE_BVH with env WR_BVH_VERIFY=1 (validation, slow): every ray is
   * traced again by the reference's KD walk and the two answers compared.     */
  int64_t verify_rays;
  int64_t verify_mismatches; /* (t, primitive) pairs that differ bit for bit      */
  int64_t pipelines;         /* render calls: the most concurrent pipelines one
                                device ran (API v6)                              */
  int64_t deferred_rays;     /* always 0: the experiment that counted here is
                                removed; the field keeps the
                                struct's layout (API v6)                         */
  int64_t bvh_width;         /* WR_TRACE_BVH: the search tree's width, 2 or 4 (4
                                from 2^18 triangles); 0: KD walk
                                (API v7)                                         */
  int64_t work_bytes;        /* render calls: device bytes of the work buffers the
                                pipelines of this call hold (API v8)              */
  int64_t work_paths;        /* ... and the paths they hold at once (buffer sets x
                                paths per set), so work_bytes / work_paths is the
                                memory per path in flight (API v8)               */
  int64_t redone;            /* BDPT: renders redone with smaller pieces because
                                a vertex pool or shadow queue sized by use filled
                                up (the film is the one of an unbounded render;
                                DESIGN.md 3; API v8)                              */
} wr_stats;

/* The reference's in-memory Scene (scene/scene.h:35-42) as flat host arrays,
 * for callers that build or already hold it instead of a .scene file.  The
 * caller keeps ownership; wr_scene_from_desc copies what it needs and builds
 * the KD tree (KDtreeAccel::init + buildTree, KDtreeAccel.cpp:12-307), so the
 * result is the scene wr_scene_load makes from a file with the same content. */
typedef struct {
  int32_t n_prims;             /* Scene::objs, in order (the KD tree's tie order)          */
  const int32_t* prim_type;    /* 0 Triangle (triangle.h:14-31), 1 Sphere (sphere.h:16-21) */
  const float* prim_data;      /* 9 floats each: triangle p0 p1 p2; sphere centre xyz, radius, 5 unused */
  const int32_t* prim_mat;     /* matId: >= 0 materials[]; < 0 emitter of AreaLight -matId-1
                                  (scene.cpp:412-427); 0 = black, ends paths                  */
  int32_t n_lights;            /* Scene::lights: AreaLight(p0, p1, p2, intensity) (light.h:90-103) */
  const float* light_tri;      /* 9 floats each: p0 p1 p2                                    */
  const float* light_le;       /* 3 floats each: intensity (RGB)                             */
  int32_t n_materials;         /* Scene::materials (material.h:7-31)                          */
  const float* materials;      /* 11 floats each: diffuse rgb, phong rgb, specular rgb, phongExp, refracIndex */
  float cam_pos[3], cam_fwd[3], cam_up[3]; /* Camera::setup (camera.cpp:3-29); fwd / up normalised there */
  float cam_xres, cam_yres;    /* raster size; the reference takes xRes from the XML height (scene.cpp:292-295) */
  float cam_hfov;              /* horizontal field of view, degrees                          */
} wr_scene_desc;

/* ---- scene (Scene::init, scene/scene.cpp:469-489 + loadScene :259-467) ---- */
int wr_scene_load(const char* scene_path, wr_scene** out);
/* Scene::init from the in-memory arrays above (WR_E_ARG on a malformed desc:
 * null arrays, bad type, an emitter matId without its light). */
int wr_scene_from_desc(const wr_scene_desc* desc, wr_scene** out);
int wr_scene_info_get(const wr_scene* scene, wr_scene_info* out);
/* 64-bit FNV-1a of what a render reads from the scene (primitives, lights,
 * materials, camera).  Checkpoints store it (with the integrator's settings)
 * so that a film is never resumed into a render of another scene. */
int wr_scene_fingerprint(const wr_scene* scene, uint64_t* out);
/* Text dump in the format of oracle/ref_driver.cpp `scene` (parity tests). */
int wr_scene_dump(const wr_scene* scene, const char* out_path);
void wr_scene_free(wr_scene* scene);

/* ---- device context ---- */
int wr_device_count(void);
int wr_create(const wr_scene* scene, int hip_device, wr_context** out);
/* Several GPUs of one node behind one context: the scene is uploaded to each
 * of devices[0..n) and every later call is shared out --
 *   wr_render_bdpt: equal contiguous shares of the render's path-iterations
 *     (iteration-major; one iteration still spreads over every device),
 *   wr_render_vcm: contiguous iteration ranges (a merge grid per iteration),
 *   wr_render_path: contiguous sample ranges of the spp grid,
 *   wr_trace_closest / wr_occluded: contiguous ray ranges;
 *   wr_path_radiance runs on devices[0].
 * The devices render concurrently into films of their own, which are summed on
 * devices[0] by one RCCL reduce over xGMI (a device listed twice, or env
 * WR_MULTI_REDUCE=peer: peer copies + an add kernel), then returned like a
 * single-device render (a device film lives on devices[0]).  The reference's
 * render loop over iterations (bidirPathTracing.cpp:25-26) is what is shared
 * out; the result equals one device's up to float summation order. */
int wr_create_multi(const wr_scene* scene, const int* hip_devices, int n_devices, wr_context** out);
/* Devices of a context (devices[0] first); returns their number, writes up to max_n. */
int wr_context_devices(const wr_context* ctx, int* devices, int max_n);
void wr_destroy(wr_context* ctx);

/* ---- one process per GPU: each rank renders its own
 * iterations into a device film; one reduce(sum) of the films over RCCL per
 * sample batch.  Rank 0 calls wr_comm_unique_id and hands the 128 bytes to the
 * other ranks (any channel: MPI, a file, torch.distributed); every rank then
 * calls wr_comm_init on its context. */
int wr_comm_unique_id(uint8_t id[128]);
int wr_comm_init(wr_context* ctx, const uint8_t id[128], int nranks, int rank);
/* Sum the ranks' device films (nfloat floats on the context's device) into
 * rank `root`'s film, in place; collective (every rank calls it).  Ordered
 * after the caller's work on the legacy null stream; returns when done. */
int wr_film_reduce(wr_context* ctx, float* film_dev, int64_t nfloat, int root);
/* The communicator's size and this rank, read back from RCCL (ncclCommCount,
 * ncclCommUserRank): a bench or driver checks the job really spans N ranks. */
int wr_comm_info(const wr_context* ctx, int* nranks, int* rank);
/* Concurrent render pipelines (HIP streams, each with its own work buffers,
 * ~5 GB per pair of iterations at 1080p): iterations / samples are dealt
 * round-robin to them so that one stream's late-bounce traversal tail overlaps
 * another's full launches.  1..16; default = the process's hardware queues
 * (GPU_MAX_HW_QUEUES, read when wr_create runs) up to 16, or env WR_PIPES.
 * GPU-specific scheduling; no reference counterpart. */
int wr_set_pipelines(wr_context* ctx, int n);
/* Ask HIP for n hardware queues (1..32) -- one per render pipeline -- by
 * raising GPU_MAX_HW_QUEUES to n (a larger value already set is kept).  HIP
 * reads the variable once, when it initialises: call this at the top of main(),
 * before the process's first HIP call and before other threads start (it
 * writes the process environment).  Returns the queue count in effect for
 * contexts created later, or WR_E_ARG.  The library never changes the
 * environment otherwise (API v8). */
int wr_request_hw_queues(int n);

/* Allocate now what renders of this integrator and film size on the context
 * will use -- every pipeline's work buffers (each device of a multi-device
 * context) -- instead of inside the first render call.  Optional; the
 * counterpart of the allocations SurfaceIntegrator::init makes before render()
 * (surfaceIntegrator/surfaceIntegrator.h:14-34).  Call after wr_set_pipelines /
 * wr_set_trace_mode (API v6). */
enum { WR_INTEGRATOR_BDPT = 0, WR_INTEGRATOR_VCM = 1, WR_INTEGRATOR_PATH = 2 };
int wr_reserve(wr_context* ctx, int integrator, int32_t width, int32_t height);

/* Traversal mode of every later call on the context.
 *   WR_TRACE_REFERENCE: the reference's KD tree, walked exactly as
 *     KDtreeAccel::traverse (scene/KDtreeAccel.cpp:309-388) walks it.
 *   WR_TRACE_BVH (default): a BVH search over the triangles and spheres for
 *     the smallest hit, accepted only when the winner is provably the
 *     reference's (unique within EPS, in a KD leaf the reference's traversal
 *     reaches, the ray not grazing a tested triangle's plane, its origin inside
 *     the region the sphere boxes are grown for); every other ray is traced in
 *     the reference mode.  Same rays, same (t, primitive) answers; see
 *     DESIGN.md 4b.  (Spheres: API v8.)
 * Env WR_TRACE_BVH=0 / 1 sets the mode at wr_create. */
enum { WR_TRACE_REFERENCE = 0, WR_TRACE_BVH = 1 };
int wr_set_trace_mode(wr_context* ctx, int mode);

/* ---- traversal ---- */
/* Scene::intersect (scene/scene.cpp:21-43) -> KDtreeAccel::traverse
 * (scene/KDtreeAccel.cpp:309-388).  Host arrays of n rays / hits. */
int wr_trace_closest(wr_context* ctx, const wr_ray* rays, int64_t n, wr_hit* hits);
/* Scene::occluded (scene/scene.cpp:55-81): a closest-hit traversal of
 * Ray(o, d) (d re-normalised as the Ray constructor does) whose answer is
 * "not occluded" iff it misses or its hit point equals targets[3k..3k+2]
 * within EPS per component. */
int wr_occluded(wr_context* ctx, const wr_ray* rays, const float* targets, int64_t n, uint8_t* occluded);

/* ---- integrators ---- */
/* BidirPathTracing::render (surfaceIntegrator/bidirPathTracing.cpp:23-27,
 * runIteration :53-265).  film: height*width*3 floats in ImageFilm layout
 * film[x_raster][y_raster] (pre-transpose), accumulated (+=), NOT scaled by
 * 1/iterations.  film_on_device != 0: `film` is a device pointer on the
 * context's device.  The render is ordered after all work submitted before the
 * call on the legacy null stream (torch's default stream); work on another
 * caller stream that writes the film must be synchronized by the caller first.
 * The call returns once the film holds the result (all streams synchronized). */
int wr_render_bdpt(wr_context* ctx, const wr_bdpt_params* p, float* film, int film_on_device, wr_stats* stats);
/* SurfaceIntegrator::render (surfaceIntegrator.cpp:14-46) + PathIntegrator::raytracing
 * (pathIntegrator.cpp:29-148).  film[height][width][3] accumulates the per-sample
 * radiance SUM (the reference's final film->scale(1/spp) is left to the caller). */
int wr_render_path(wr_context* ctx, const wr_path_params* p, float* film, int film_on_device, wr_stats* stats);

/* PathIntegrator::raytracing(const Ray& ray, int dep) (pathIntegrator.cpp:29-148),
 * the per-sample estimator SurfaceIntegrator::render calls, for a batch of
 * caller rays (o and d used as given, like a constructed Ray; tmin / tmax
 * ignored: the reference traces with 0 / INF).  rgb: n*3 floats, overwritten
 * with the radiance of each ray.  Ray k draws from the counter-RNG stream
 * (seed, sample, 2, k) -- the PT render's streams skip that stream's first
 * draw, which stratifies the pixel sample.  `dep` is unused by the reference
 * and has no counterpart. */
int wr_path_radiance(wr_context* ctx, const wr_ray* rays, int64_t n, int32_t max_depth, uint32_t seed,
                     int32_t sample, float* rgb, wr_stats* stats);

/* VertexCM::render (surfaceIntegrator/vertexcm.cpp:23-27, runIteration :47-285):
 * vertex connection + vertex merging.  The reference's point KD tree over the
 * light vertices (scene/KDtree.h) is replaced by a hash grid: searchInRadius
 * reports exactly the vertices with |x - v| < radius, and so does the grid.
 * film as wr_render_bdpt (pre-transpose, accumulated, not scaled). */
int wr_render_vcm(wr_context* ctx, const wr_vcm_params* p, float* film, int film_on_device, wr_stats* stats);

/* ---- second-moment films and the error estimate (no reference
 * counterpart: the reference keeps only the sum).  A *pass* is the unit whose
 * films are independent estimates of the image:
 *   BDPT / VCM: one iteration (global index iter_begin + i), whole frame, with
 *     the light-tracing splats it lands on other pixels;
 *   PT: one sample index k of the spp grid, whole frame, unscaled.
 * With F_i the film of pass i alone, a moments render accumulates
 *   film    += sum_i F_i          (exactly what the plain render adds)
 *   film_sq += sum_i F_i o F_i    (per value, of the complete pass film)
 * into two caller films of height*width*3 floats, same layout, both host or
 * both device (films_on_device).  Both accumulate, so calls over disjoint pass
 * ranges add up: resume, sharding over ranks, wr_film_reduce of film_sq.
 * Otherwise as the plain calls (ordering, stats, the BDPT redo, which puts both
 * films back).  A moments render keeps every piece of an iteration on one
 * pipeline, which holds 2 pass films of the frame's size (allocated by the
 * first moments render, kept on the context); a plain render allocates none.
 * On a wr_create_multi context: WR_E_ARG (it shares one iteration out over
 * its devices).
 * PT: the samples of a pixel are strata of one grid (sampler.cpp:28-42), not
 * i.i.d. passes: film_sq / wr_film_error then give a conservative estimate
 * (stratification only lowers the variance of the mean), and a PT render
 * cannot stop early without leaving part of each pixel unsampled.
 * Callers detect these entry points by their symbols (WR_API_VERSION stays 8). */
int wr_render_bdpt_moments(wr_context* ctx, const wr_bdpt_params* p, float* film, float* film_sq,
                           int films_on_device, wr_stats* stats);
int wr_render_vcm_moments(wr_context* ctx, const wr_vcm_params* p, float* film, float* film_sq,
                          int films_on_device, wr_stats* stats);
int wr_render_path_moments(wr_context* ctx, const wr_path_params* p, float* film, float* film_sq,
                           int films_on_device, wr_stats* stats);

/* Standard error of the mean image from the two films of n_passes passes.  Per
 * value, in double from the float inputs (in float, Q - S^2/n of a value that
 * barely varies cancels to noise):
 *   mu = S / n,  var_of_mean = max(0, (Q - S^2 / n) / (n - 1)) / n,
 *   se = sqrt(var_of_mean)                      (S = film, Q = film_sq). */
typedef struct {
  double sum_stderr;      /* sum of se over all values                            */
  double sum_mean;        /* sum of mu over all values                            */
  double rel_stderr;      /* sum_stderr / sum_mean, 0 if the film is black        */
  double max_rel_stderr;  /* largest se / mu over the values with mu > 0          */
  int64_t values;         /* number of values with mu > 0                         */
} wr_error_info;
/* Host films (films_on_device == 0): a plain loop on the CPU; ctx may be NULL
 * and no device is needed.  Device films: a kernel on the context's device,
 * ordered like a render.  stderr_map (or NULL): height*width*3 floats in the
 * films' memory space, overwritten with se.  WR_E_ARG: n_passes < 2, a null
 * film or `out`, device films without a context. */
int wr_film_error(wr_context* ctx, const float* film, const float* film_sq, int width, int height, int n_passes,
                  int films_on_device, float* stderr_map, wr_error_info* out);

/* ---- first-hit feature films and the film denoiser (no
 * reference counterpart).  Callers detect these entry points by their symbols
 * (WR_API_VERSION stays 8).
 *
 * wr_render_features traces one ray per pixel through the pixel centre -- no
 * RNG, so the films are deterministic -- and writes what the first hit sees.
 * The ray is the PT primary ray (origin cam.pos, no EPS offset,
 * d = normalize(rasterToWorld(rx, ry, 0) - cam.pos)); `layout` says which raster
 * point a value index stands for, so that the films line up with a radiance
 * film of that integrator:
 *   WR_FILM_PT:   index i * width + jj  <-  raster point (jj, i)
 *   WR_FILM_BDPT: index a * width + b   <-  raster point (a + 0.5, b + 0.5)
 *                 (BDPT and VCM films, pre-transpose)
 * With h the wr_hit wr_trace_closest returns for that ray:
 *   normal = h.n, position = h.p (3 floats per pixel), depth = h.t (1 float),
 *   albedo = min(1, diffuse + phong + specular) per channel of material
 *            h.mat_id, (1, 1, 1) for an emitter (mat_id < 0).
 * A miss writes zeros to every film: an all-zero normal is the "no surface"
 * mark wr_film_denoise reads.  Each output may be NULL (not wanted); all NULL:
 * WR_E_ARG.  films_on_device: the outputs are device pointers on the context's
 * device (devices[0] of a wr_create_multi context, which runs the call there).
 * Runs in the context's trace mode, ordered like a render; stats (or NULL):
 * closest_rays and seconds.  WR_E_ARG: width or height < 1, more than 2^28
 * pixels, a layout that is neither. */
enum { WR_FILM_PT = 0, WR_FILM_BDPT = 1 };
int wr_render_features(wr_context* ctx, int32_t width, int32_t height, int layout, float* normal, float* albedo,
                       float* position, float* depth, int films_on_device, wr_stats* stats);

/* wr_film_denoise: an edge-avoiding a-trous wavelet filter over the mean image
 * of a moments render, guided by the variance of the mean per pixel (from
 * film_sq, as wr_film_error computes it) and by the feature films.  `levels`
 * passes of a 5 x 5 B3-spline kernel with holes, step 1, 2, 4, ...; a
 * neighbour's weight falls with
 *   the luminance difference, in standard errors of the pixel (sigma_l),
 *   the angle between the normals (normal_power),
 *   the distance of the neighbour from the pixel's tangent plane, as the sine
 *     of the elevation angle (sigma_p),
 *   the L1 distance of the albedos (sigma_a);
 * surface and no-surface pixels (an all-zero normal) never mix.  DESIGN.md 11
 * has the definition; it uses + - * / sqrt only, in a fixed order, so host
 * films (a plain CPU loop; ctx may be NULL, no device needed) and device films
 * (kernels on the context's device, devices[0] of a multi-device context,
 * ordered like a render) give the same bits.
 * film, film_sq: the two films of n_passes passes (height*width*3 floats); any
 * of normal / position / albedo may be NULL, which sets its weight to 1.  All
 * films live in one memory space (films_on_device).  out: height*width*3
 * floats at the scale of `film` (a sum over n_passes), so it goes wherever
 * `film` goes, e.g. wr_film_write_image(..., scale = 1 / n_passes).  Device
 * films: the first call allocates two (c, v) planes and, with guides, a
 * guide record per pixel (16 + 16 + 48 bytes per pixel) on the context, kept
 * afterwards; a render allocates none of this.
 * WR_E_ARG: n_passes < 2; a null film, film_sq or out; out equal to an input;
 * width or height < 1 or more than 2^28 pixels; parameters out of range or a
 * sigma that is not > 0; device films without a context. */
typedef struct {
  int32_t levels;        /* 1..8, default 5: steps 1,2,4,8,16                       */
  int32_t normal_power;  /* w_n = max(0, Np.Nq)^(2^normal_power), 0..10, default 7   */
  float sigma_l;         /* luminance, in standard errors; default 4                 */
  float sigma_p;         /* plane distance, as a sine; default 0.05                  */
  float sigma_a;         /* albedo L1 distance; default 0.1                          */
} wr_denoise_params;     /* 20 bytes; NULL = the defaults                            */
int wr_film_denoise(wr_context* ctx, const float* film, const float* film_sq, int width, int height, int n_passes,
                    const float* normal, const float* position, const float* albedo, const wr_denoise_params* p,
                    int films_on_device, float* out);

/* ---- ray batches that already live on the GPU (no reference
 * counterpart).  Callers detect these entry points by their symbols
 * (WR_API_VERSION stays 8).
 *
 * The three _dev calls are wr_trace_closest, wr_occluded and wr_path_radiance
 * for arrays in device memory: the same kernels read the caller's rays where
 * they lie and write the caller's outputs directly, so the answers are the host
 * calls' bit for bit and nothing crosses to the host.  Trace mode, the ray
 * limits (2^28; 2^26 for radiance), n == 0 and WR_E_SCENE are as in the host
 * calls.
 *   Ownership: the caller owns every array and keeps it alive and unchanged
 *     until the call returns.  Every pointer is device memory on the context's
 *     device (devices[0] of a wr_create_multi context, which runs the call
 *     there and does not share it out).  Records need only 4-byte alignment
 *     (`occluded`: any), so a slice rays + 1 or hits + 1 is fine.
 *   Streams: the call is ordered after all work submitted before it on the
 *     legacy null stream (torch's default stream); work on another caller
 *     stream that writes an input or output must be synchronized by the caller
 *     first.  The call returns when the outputs are written.
 *   WR_E_ARG: a null pointer with n > 0; n < 0 or over the limit; max_depth out
 *     of range; an output range that overlaps an input range or another output;
 *     a pointer that is not device memory of the context's device (host and
 *     pinned host memory belong to the host calls).
 * wr_path_radiance_dev accumulates (+=) the radiance of each ray into rgb (n*3
 * floats), like a device film: zero it for a plain radiance.  rgb_sq (or NULL):
 * n*3 floats that receive += the square of this call's radiance, per value, so
 * that one call per sample index builds the (film, film_sq) pair of an n x 1
 * film that wr_film_error (n_passes = calls) and wr_film_denoise read.  Ray k
 * draws from stream (seed, sample, 2, k) as in wr_path_radiance.  The first
 * call with rgb_sq allocates a pass film on the context, kept afterwards. */
int wr_trace_closest_dev(wr_context* ctx, const wr_ray* rays, int64_t n, wr_hit* hits);
int wr_occluded_dev(wr_context* ctx, const wr_ray* rays, const float* targets, int64_t n, uint8_t* occluded);
int wr_path_radiance_dev(wr_context* ctx, const wr_ray* rays, int64_t n, int32_t max_depth, uint32_t seed,
                         int32_t sample, float* rgb, float* rgb_sq, wr_stats* stats);
/* The ray wr_render_features traces for every value index of a width x height
 * film in `layout` (origin cam.pos, d = normalize(rasterToWorld(..) - cam.pos),
 * tmin 0, tmax 1e7), as wr_ray records: rays[index].  rays_on_device as
 * films_on_device of wr_render_features; ordered like a render.  A caller
 * perturbs them on the device (a thin lens, a panorama) and hands them to the
 * _dev calls.  WR_E_ARG: as wr_render_features; null rays. */
int wr_camera_rays(wr_context* ctx, int32_t width, int32_t height, int layout, wr_ray* rays, int rays_on_device);

/* ---- shading on device arrays (no reference counterpart).
 * Callers detect these entry points by their symbols (WR_API_VERSION stays 8).
 *
 * What the reference's integrators do at a path vertex, one record per array
 * element: build the BSDF of a hit and evaluate or sample it, pick a point on
 * an area light, read an emitter's radiance, draw from the counter RNG.  The
 * kernels run the device functions the renders run (csrc/wr_devmath.h), so
 * every value is the render's, and the oracle's, bit for bit.  With
 * wr_trace_closest_dev / wr_occluded_dev a caller writes its own integrator
 * over arrays that never leave the GPU.
 *
 * Records are plain structs of 4-byte members and need only 4-byte alignment
 * (a slice out + 1 is fine).  A field the reference leaves unwritten on the
 * branch a record takes (cos_wo when BSDF::f returns early, wo of a black
 * sample, ...) is 0: every record starts from zeros. */
typedef struct {
  int32_t valid;        /* 0: no BSDF here (see below); the whole record and the call's `out` record are zero */
  int32_t is_delta;     /* isDelta                                                  */
  float cos_wi;         /* wiLocal.z                                                */
  float continue_prob;  /* continueProb                                             */
  float fresnel;        /* reflectCoeff                                             */
  float prob[4];        /* diffuse, glossy, reflect, refract                        */
} wr_bsdf_info;         /* 36 bytes: BSDF::init, bsdf.h:66-89                       */
typedef struct {
  float f[3];           /* BSDF::f (bsdf.cpp:102-126)                               */
  float cos_wo;         /* ... its cosWo                                            */
  float dir_pdf;        /* ... its directPdfW                                       */
  float rev_pdf;        /* ... its reversePdfW                                      */
  float pdf;            /* BSDF::pdf forward (:165-181)                             */
  float pdf_rev;        /* BSDF::pdf reverse                                        */
} wr_bsdf_eval;         /* 32 bytes                                                 */
typedef struct {
  float f[3];           /* BSDF::sample (bsdf.cpp:183-334)                          */
  float wo[3];          /* world direction, as sampled (unit up to rounding)        */
  float pdf;
  float cos_wo;
  int32_t type;         /* the T_* bit r3[2] chose: 1 reflect, 2 refract, 4 diffuse, 8 glossy */
} wr_bsdf_sample;       /* 36 bytes                                                 */
typedef struct {
  float le[3];          /* AreaLight::illuminance (light.cpp:4-38)                  */
  float dir[3];         /* dirToLight                                               */
  float dist;
  float direct_pdf;     /* directPdfW                                               */
  float emission_pdf;   /* emissionPdfW                                             */
  float cos_light;      /* cosAtLight                                               */
} wr_light_illum;       /* 40 bytes                                                 */
typedef struct {
  float le_cos[3];      /* AreaLight::emit (light.cpp:40-67): radiance * cos        */
  float pos[3];
  float dir[3];
  float emission_pdf;   /* emissionPdfW                                             */
  float direct_pdf_a;   /* directPdfA                                               */
  float cos_light;      /* cosAtLight                                               */
} wr_light_emission;    /* 48 bytes                                                 */
typedef struct {
  float le[3];          /* AreaLight::getRadiance (light.cpp:69-100)                */
  float direct_pdf_a;
  float emission_pdf;
} wr_light_rad;         /* 20 bytes                                                 */
/* BSDF calls.  hits: records as wr_trace_closest_dev writes them; only n,
 *   mat_id and prim are read.  wi: 3 floats per record, the direction the
 *   integrators hand to the BSDF constructor (-ray.d); it is normalised in
 *   the local frame.  wo (eval): 3 floats, a world direction.  r3 (sample):
 *   3 floats in [0, 1), r3[2] picks the component.  info (or NULL) receives
 *   the BSDF itself.
 *   valid = 0 and all-zero records: a miss (prim < 0), material 0, or wi
 *   within EPS of the tangent plane (bsdf.h:75).  An emitter hit (mat_id < 0)
 *   is valid with the values the renders use: probabilities 0, continue_prob
 *   0, not delta, f = 0.
 * Light calls.  light: an index into Scene::lights (wr_scene_info.nlights).
 *   illuminate: pos = the shaded point, r3 = the triangle sample.  emit:
 *   dir_r3 and pos_r3 as AreaLight::emit's two samples.  radiance: the light
 *   is the hit's (-mat_id - 1), ray_d the direction of the ray that hit it; a
 *   miss or a non-emitter gives zeros.  WR_E_SCENE on a scene without lights.
 * wr_rng_uniform_dev: record k receives draws ctr[k]+1 .. ctr[k]+draws of
 *   stream (seed, iteration, subpath, path[k]) as RNG::randFloat values
 *   (k / 2^24), out[k * draws + j], and ctr[k] advances by draws.  path NULL:
 *   path k = k; ctr NULL: counters start at 0 and are not kept.  draws = 3 is
 *   one RNG::randVector3.  A caller that keeps the counters reproduces the
 *   path tracer's draw order: subpath 2, path = ray index (wr_path_radiance).
 * Caller data never becomes a GPU fault: the arrays are on the device, so the
 *   kernels check them.  A light outside [0, nlights) or a mat_id outside
 *   (-nlights - 1, nmaterials) gives an all-zero record (valid = 0), not an
 *   error return.
 * Ownership, alignment, stream ordering, returning when the outputs are
 *   written, and devices[0] of a multi-device context: as the _dev calls
 *   above.  n == 0 succeeds.  WR_E_ARG: a null pointer with n > 0 (except
 *   the optional ones); n < 0 or n > 2^28; draws outside 1..64; a pointer that
 *   is not device memory of the context's device; an output range that
 *   overlaps an input or another output (ctr is in/out). */
int wr_bsdf_eval_dev(wr_context* ctx, const wr_hit* hits, const float* wi, const float* wo, int64_t n,
                     wr_bsdf_info* info, wr_bsdf_eval* out);
int wr_bsdf_sample_dev(wr_context* ctx, const wr_hit* hits, const float* wi, const float* r3, int64_t n,
                       wr_bsdf_info* info, wr_bsdf_sample* out);
int wr_light_illuminate_dev(wr_context* ctx, const int32_t* light, const float* pos, const float* r3, int64_t n,
                            wr_light_illum* out);
int wr_light_emit_dev(wr_context* ctx, const int32_t* light, const float* dir_r3, const float* pos_r3, int64_t n,
                      wr_light_emission* out);
int wr_light_radiance_dev(wr_context* ctx, const wr_hit* hits, const float* ray_d, int64_t n, wr_light_rad* out);
int wr_rng_uniform_dev(wr_context* ctx, uint32_t seed, uint32_t iteration, uint32_t subpath, const uint32_t* path,
                       uint32_t* ctr, int32_t draws, int64_t n, float* out);

/* ---- point sets on the device: radius and k-nearest queries.
 * Callers detect these entry points by their symbols (WR_API_VERSION stays 8).
 *
 * The reference's point KD tree (scene/KDtree.h) as calls on device arrays:
 * what -vcm, -pr and -mm ask of searchInRadius and -pm of searchKnn
 * (knnPhotons = 50, maxSqrDis = 0.1).  An index is a hashed grid over a copy of
 * the caller's points; the answers are exact and a pure function of the arrays,
 * never of the grid:
 *   d2(q, p) = sqr_len(q - p) in float: per-component subtraction, then
 *     x*x + y*y + z*z, each step rounded, no fused multiply-add
 *     (Vector3::sqrLength).
 *   Radius queries (KdTree::searchInRadius, KDtree.h:141-173) report point i
 *     iff sqrtf(d2) < r, strictly, with the correctly rounded square root;
 *     r = radii[j] when `radii` is given, else `radius`.  count[j] is the
 *     number of points reported for query j.  wr_points_in_radius_dev writes
 *     their indices (into the caller's `pos`) at index[offset[j] ..], at most
 *     offset[j + 1] - offset[j] of them (a list that does not fit is cut
 *     short), and never outside [0, capacity): a query whose offsets decrease,
 *     are negative or pass `capacity` writes nothing.  The order inside one
 *     list is the index's own, not ascending, and deterministic: the same
 *     arrays give the same bytes, run after run and build after build.
 *   k-nearest queries (KdTree::searchKnn, KDtree.h:175-208, with
 *     photonMap.h's ClosePhotonQuery) consider the points with
 *     d2 < max_sqr_dist (strictly) and return the k smallest in the order of
 *     (d2, index), ascending: equal d2 goes to the lower index.  count[j] is
 *     how many were found (<= k); unused slots hold index -1 and sqr_dist 0;
 *     sqr_dist[j * k + count[j] - 1] is the squared gather radius
 *     ClosePhotonQuery keeps in kPhotons[0].sqrDis.
 *   A point with a NaN or infinite coordinate is never reported; a query with
 *     one reports nothing.
 * wr_points_build_dev copies what it needs: `pos` may be freed or changed
 *   afterwards.  The index belongs to the caller (wr_points_free; NULL is a
 *   no-op); wr_destroy frees the indices of the context that are still alive,
 *   after which their handles are dead.  n == 0 builds an empty index.  It
 *   holds 16 bytes per point and 4 per bucket (wr_points_info.device_bytes).
 * Every array is device memory of the context's device (devices[0] of a
 *   wr_create_multi context), 4-byte aligned (`offset`: 8-byte).  Stream
 *   ordering and returning when the outputs are written: as the _dev calls
 *   above.  nq == 0 succeeds.  Array contents never become a GPU fault.
 * WR_E_ARG: a null context, n < 0 or nq < 0 (refused before any HIP call); n
 *   or nq above 2^28; a cell that is not a finite number > 0; k outside 1..64;
 *   a negative or NaN radius (radii NULL) or max_sqr_dist; capacity < 0; a
 *   null pointer with a non-zero size (radii excepted); a misaligned pointer;
 *   a pointer that is not device memory of the context's device; an output
 *   that overlaps an input or another output; an index of another context. */
typedef struct wr_points wr_points;   /* an index over a caller's point set, on the context's device */
typedef struct {
  int64_t n;              /* points indexed                                   */
  float   cell;           /* cell edge                                         */
  float   origin[3];      /* grid origin: the bounding-box minimum of the finite points */
  int64_t buckets;        /* hash buckets                                      */
  int64_t max_bucket;     /* most points in one bucket                         */
  int64_t device_bytes;   /* what the index holds in HBM                       */
} wr_points_info;
int wr_points_build_dev(wr_context* ctx, const float* pos /* n*3, device */, int64_t n, float cell, wr_points** out);
int wr_points_info_get(const wr_points* idx, wr_points_info* out);
void wr_points_free(wr_points* idx);
int wr_points_count_dev(wr_context* ctx, const wr_points* idx, const float* q /* nq*3 */, int64_t nq, float radius,
                        const float* radii /* NULL, or nq radii that replace `radius` */, int32_t* count /* nq */);
int wr_points_in_radius_dev(wr_context* ctx, const wr_points* idx, const float* q, int64_t nq, float radius,
                            const float* radii, const int64_t* offset /* nq+1, the caller's exclusive scan of `count` */,
                            int64_t capacity /* entries `index` holds */, int32_t* index);
int wr_points_knn_dev(wr_context* ctx, const wr_points* idx, const float* q, int64_t nq, int32_t k, float max_sqr_dist,
                      int32_t* index /* nq*k */, float* sqr_dist /* nq*k */, int32_t* count /* nq */);

/* ---- photon mapping (PhotonIntegrator, surfaceIntegrator/photonMap.{h,cpp};
 * DESIGN.md 15).  Callers detect these entry points by their symbols
 * (WR_API_VERSION stays 8).  Single-device: a wr_create_multi context is
 * refused with WR_E_ARG.
 *
 * wr_photon_map_build runs buildPhotonMap: shot s = 0, 1, ... draws from
 *   counter stream (seed, 0, 3, s); the caustic map is the first n_caustic
 *   caustic photons in (shot, bounce) order, the indirect map the first
 *   n_indirect indirect ones; shooting ends after the first shot at which both
 *   maps are full, else after max_shots (a map is then what was found).  The
 *   maps are a pure function of (scene, seed, n_caustic, n_indirect,
 *   max_path_length, max_shots): shot_batch and cell change no byte of them.
 *   A map count of 0 asks for no map of that class.  The map belongs to the
 *   caller (wr_photon_map_free; NULL is a no-op) and must be freed before its
 *   context is destroyed.
 * wr_photon_map_read copies a map's photons out, in map order: pos, wi, alpha
 *   count*3 floats each, shot count int32 (the 0-based shot of each photon);
 *   any pointer may be NULL; on_device: the pointers are device memory of the
 *   context's device.
 * wr_photon_estimate_dev is estimate() for the caller's hits (wr_hit records,
 *   as wr_trace_closest_dev writes them) and directions wo: with k_eff =
 *   min(k, photons with a finite d2), the k_eff photons smallest by
 *   (d2, index); msd = max_sqr_dist * 2^j for the smallest j >= 0 with the
 *   k_eff-th d2 < msd; scale = 1 / (PI * msd * k_eff); the terms
 *   (brdf | alpha) * (cos * scale / pdf) added in ascending (d2, index) order,
 *   a photon below the surface evaluated with its world z negated.  found[j] =
 *   k_eff.  A miss, a non-finite position or an empty map gives found 0, msd 0
 *   and black; an emitter or a hit without a BSDF gives black.
 * wr_render_photon is SurfaceIntegrator::render over PhotonIntegrator::
 *   raytracing: samples, streams, stratification and the film (a sum over
 *   samples, PT layout) as wr_render_path; depths 0..2.  direct_target 0 puts
 *   the direct-light shadow ray's target at the camera ray's hit distance, as
 *   the reference does; 1 at the light's distance.
 * WR_E_ARG: a null pointer the call needs; counts < 0 or above 2^24;
 *   max_path_length outside 1..32; max_shots outside 1..2^31 - 1; shot_batch
 *   < 0 or above 2^22; a cell that is neither 0 nor a finite number > 0; k
 *   outside 1..64; max_sqr_dist not a finite number > 0; `which` not
 *   WR_PHOTON_*; a map of another context; the array checks of the _dev calls
 *   above.  WR_E_SCENE: a scene without lights.  n == 0 succeeds. */
typedef struct {
  int32_t n_caustic, n_indirect;  /* 10000 / 100000 in the reference                 */
  int32_t max_path_length;        /* 5                                                */
  int64_t max_shots;              /* 500000 (the reference never reads its own cap)  */
  int32_t shot_batch;             /* shots per batch; 0: 65536                       */
  float   cell;                   /* the maps' grid cell; 0: derived  */
  uint32_t seed;
} wr_photon_map_params;
typedef struct wr_photon_map wr_photon_map;
typedef struct {
  int64_t shots;                          /* shots run                                           */
  int32_t caustic_count, indirect_count;  /* photons in each map                                 */
  int64_t caustic_paths, indirect_paths;  /* 1-based shot of a full map's last photon, else shots */
  int64_t device_bytes;
  float   caustic_cell, indirect_cell;
} wr_photon_map_info;
enum { WR_PHOTON_CAUSTIC = 0, WR_PHOTON_INDIRECT = 1 };
typedef struct {
  int32_t width, height, spp;
  int32_t sample_begin, sample_count;  /* as wr_path_params                   */
  int32_t knn;                         /* 50 in the reference                 */
  float   max_sqr_dist;                /* 0.1                                 */
  int32_t direct_target;               /* 0: the reference's shadow-ray target */
  uint32_t seed;
  int32_t time_kernels, count_work;    /* accepted, not used                  */
} wr_photon_params;
int wr_photon_map_build(wr_context* ctx, const wr_photon_map_params* p, wr_photon_map** out, wr_stats* stats);
int wr_photon_map_info_get(const wr_photon_map* map, wr_photon_map_info* out);
int wr_photon_map_read(wr_context* ctx, const wr_photon_map* map, int which, float* pos, float* wi, float* alpha,
                       int32_t* shot, int on_device);
void wr_photon_map_free(wr_photon_map* map);
int wr_photon_estimate_dev(wr_context* ctx, const wr_photon_map* map, int which, const wr_hit* hits /* n */,
                           const float* wo /* n*3 */, int64_t n, int32_t k, float max_sqr_dist, float* rgb /* n*3 */,
                           float* msd /* n or NULL */, int32_t* found /* n or NULL */);
int wr_render_photon(wr_context* ctx, const wr_photon_map* map, const wr_photon_params* p, float* film,
                     int film_on_device, wr_stats* stats);

/* ---- output (ImageFilm::outputImage, scene/film.cpp:39-64; BDPT transpose
 * bidirPathTracing.cpp:29-46) ---- scale -> clamp [0,1] -> pow(1/gamma) ->
 * (uchar)(x*255.0); binary PPM (RGB).  transpose != 0 swaps [i][j] <-> [j][i]
 * first (square films only, as the reference). */
int wr_film_write_ppm(const float* film, int height, int width, float scale, float gamma, int transpose,
                      const char* path);
/* The same pipeline into the format the path's extension names, as the
 * reference's cvSaveImage(filename) does (film.cpp:63): .ppm, .bmp (24-bit),
 * .png (8-bit RGB); .pfm writes the scaled linear floats (no clamp / gamma).
 * Other extensions: WR_E_ARG. */
int wr_film_write_image(const float* film, int height, int width, float scale, float gamma, int transpose,
                        const char* path);

/* ---- film checkpoint / resume.  The reference keeps the film in
 * memory only while it loops over iterations (bidirPathTracing.cpp:23-27).
 * Iterations / samples are keyed by their global index, so a render resumes
 * exactly: load the film, render the indices [done, total) (iter_begin /
 * sample_begin = done) into it.  The file carries the accumulated, unscaled
 * film and a checksum; it is replaced atomically (write + rename). */
enum { WR_CKPT_BDPT = 1, WR_CKPT_VCM = 2, WR_CKPT_PT = 3 };
typedef struct {
  int32_t width, height;
  int32_t kind;         /* WR_CKPT_*                                         */
  int32_t done, total;  /* iterations (samples) summed in the film / wanted */
  uint32_t seed;
  uint32_t fingerprint[2]; /* (lo, hi) of a 64-bit hash of the scene
                              (wr_scene_fingerprint) and the integrator's
                              settings, set by the writer; a resume whose
                              own hash differs is refused.  0 = not recorded:
                              the C++ mirror (csrc/integrators.h) refuses such
                              a film too, e.g. one written before API v7 */
} wr_checkpoint_info; /* 32 bytes */
int wr_checkpoint_save(const char* path, const wr_checkpoint_info* info, const float* film);
/* film == NULL reads the header only; else film_floats must be height*width*3.
 * WR_E_IO for a missing, foreign, truncated or corrupt file. */
int wr_checkpoint_load(const char* path, wr_checkpoint_info* info, float* film, int64_t film_floats);

const char* wr_last_error(void);
int wr_api_version(void);

#ifdef __cplusplus
}
#endif
#endif /* WINMAD_RT_H */
