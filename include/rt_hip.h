/*
 * rt_hip.h -- C ABI of the MI355X-native per-pixel ray tracer (librt_hip.so).
 *
 * Drop-in boundary for RichardHancock/OpenCL-Ray-Tracer's GPU trace path.
 * Each entry point names the reference code it replaces (paths relative to
 * /root/reference/RayTrace).  Plain pointers and sizes only; no HIP, torch or
 * glm types cross this boundary.
 *
 * Scene layout is the reference's own flattened layout
 * (MainState.cpp:646-658, MainState.h:99-106):
 *   sphere_origins  float4[num_spheres]     (x, y, z, w)
 *   sphere_radius   float [num_spheres]
 *   sphere_colours  float4[num_spheres]     (r, g, b, a)
 *   cube_vertices   float4[36 * num_cubes]  12 world-space triangles per cube
 *   cube_colours    float4[num_cubes]
 * Output frame (MainState.cpp:952-955, rayTracer.cl:198-201):
 *   RT_FORMAT_I32X4: int32[rows][width][4], truncated (int) r, g, b, a
 *   RT_FORMAT_RGBA8: uint32[rows][width], (uint8)r | (uint8)g<<8 |
 *                    (uint8)b<<16 | 0xFF<<24  (the Texture packing,
 *                    MainState.cpp:984-994, :1023-1037)
 *   RT_FORMAT_HIT:   rt_hit[rows][width], what `collide` found before it
 *                    shades (MainState.cpp:330-394): the float `closest` and
 *                    the winning object (see rt_hit below)
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 1

/* Status codes: 0 = success, negative = failure.  Replaces the reference's
 * print-and-continue cl_int handling (MainState.cpp:1101-1179 getErrorString,
 * :672-674 etc.): the caller decides what to do. */
enum {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = -1,
    RT_ERR_NO_DEVICE = -2,
    RT_ERR_HIP = -3,
    RT_ERR_OUT_OF_MEMORY = -4,
    RT_ERR_UNSUPPORTED = -5
};

/* Output formats.  Value 2 is reserved and stays RT_ERR_INVALID_ARG. */
enum { RT_FORMAT_I32X4 = 0, RT_FORMAT_RGBA8 = 1, RT_FORMAT_HIT = 3 };

/* One pixel of an RT_FORMAT_HIT frame (8 bytes).
 *   t       the reference's `closest` after the whole collide loop
 *           (MainState.cpp:330-394), the exact float: nothing is normalised
 *           or clamped, a negative t or -inf is stored as it is.
 *   object  the colour slot of the winner: cube c gives c, sphere i gives
 *           num_cubes + i (cubes are tested first, MainState.cpp:347-392).
 * A miss is t = 300000.0f (the loop's initial `closest`, MainState.cpp:345)
 * and object = -1.  The comparison is a strict `<`, so no hit carries
 * t == 300000: object == -1 exactly when t == 300000, which is also the
 * miss test of the shade (MainState.cpp:398).  Of several candidates with
 * the same float t the first in the reference's order wins (lower cube,
 * lower triangle, cubes before spheres, lower sphere). */
typedef struct rt_hit {
    float t;
    int32_t object;
} rt_hit;

/* Kernel path selection (rt_render*, `path` field of rt_timing). */
enum {
    RT_PATH_AUTO = 0,    /* binned when its preconditions hold, else generic */
    RT_PATH_BINNED = 1,  /* implicit origins (x,y,0,1), ray_dir = (0,0,D,w) */
    RT_PATH_GENERIC = 2  /* any origins / direction, brute force per pixel */
};

/* The kernel that did a render's per-pixel work (rt_last_kernel). */
enum {
    RT_KERNEL_NONE = 0,         /* no render yet */
    RT_KERNEL_TRACE = 1,        /* prep_kernel -> coarse3_kernel -> trace3_kernel */
    RT_KERNEL_TRACE_SMALL = 2,  /* prep_kernel -> trace_small_kernel (<= 512 primitives) */
    RT_KERNEL_FRAME_SMALL = 3,  /* frame_small_kernel, one launch (<= 128 primitives) */
    RT_KERNEL_GENERIC = 4,      /* generic_kernel: explicit origins / any direction */
    RT_KERNEL_TRACE_SPLIT = 5,  /* prep_kernel -> coarse3_kernel -> trace3_split_kernel
                                   (small frames: several waves per wave tile) */
    RT_KERNEL_TRACE_BIN = 6     /* prep_kernel -> trace_bin_kernel (tiles bin themselves) */
};

typedef struct rt_scene {
    const float* sphere_origins;
    const float* sphere_radius;
    const float* sphere_colours;
    int32_t num_spheres;
    const float* cube_vertices;
    const float* cube_colours;
    int32_t num_cubes;
    /* float4[num_lights]: xyz the position, w reserved.  Renders ignore
     * lights (the reference has no lighting model, its "shade" is a depth
     * ramp, MainState.cpp:396-407); rt_light_hits* read them. */
    const float* lights;
    int32_t num_lights;
} rt_scene;

typedef struct rt_timing {
    double total_us;    /* host wall time of the whole call (the reference's
                           timer scope, MainState.cpp:662-894) */
    double upload_us;   /* HIP events from the stream point after the scene
                           was packed into page-locked staging on the host
                           (that packing, a few us of memcpy, is NOT in it;
                           it is in total_us) to the first render kernel's
                           start: the one H2D scene DMA, the explicit-origin
                           upload, the non-finite flag's reset when its
                           generation wraps, and the gaps before the first
                           kernel.  With explicit origins on the automatic
                           path it also covers their on-device grid check (a
                           small kernel, a 4-byte read-back and a stream sync
                           before the render, so the two are serialised) */
    double kernel_us;   /* first render kernel's start to the last one's end,
                           the kernels' own dispatch-packet timestamps */
    double download_us; /* D2H frame copy, HIP events */
    int32_t path;       /* RT_PATH_BINNED or RT_PATH_GENERIC actually used */
} rt_timing;

typedef struct rt_ctx rt_ctx;

/* Replaces MainState::openCLInit (MainState.cpp:1181-1326): selects HIP
 * device `device_ordinal` and loads every kernel's code object onto it (the
 * counterpart of clBuildProgram / clCreateKernel, :1302-1320) and, once per
 * device and process, sets up the HIP runtime's staging for pageable
 * transfers, so the first render pays no loading.  The stream is created on first use and the
 * workspace grows on demand (or up front with rt_reserve).  One context per
 * device; not re-entrant per context. */
int rt_init(int device_ordinal, rt_ctx** out_ctx);

/* Sizes the context's workspace ahead of the first render of a frame of
 * `rows` x `width` pixels with this many spheres / cubes in `out_format`:
 * the host-API scene copy and frame, the binned path's records and
 * candidate lists, and the context's stream, on which it runs one small
 * pageable upload and download (the stream's first transfers).
 * Synchronous.  openCLInit does its one-time work before any trace
 * (MainState.cpp:1290-1320, outside the trace timer :662-894); after
 * rt_reserve the first rt_render of that size allocates nothing and pays no
 * setup.  Optional: rt_render reserves what it needs itself (before its
 * timed events).  Workspace only grows. */
int rt_reserve(rt_ctx* ctx, int32_t width, int32_t rows, int32_t num_spheres,
               int32_t num_cubes, int32_t out_format);

/* Releases everything rt_init / rt_render allocated (MainState.cpp:73-78). */
void rt_destroy(rt_ctx* ctx);

/* Replaces MainState::getErrorString (MainState.cpp:1101-1179). */
const char* rt_error_string(int status);

/* Replaces the body of MainState::executeRayTracerOpenCL
 * (MainState.cpp:641-934): buffer setup, the six scene/ray uploads, the
 * clEnqueueNDRangeKernel launch of rayTracer.cl::rayTracer and the blocking
 * map/readback.  Synchronous: on return `host_out` holds rows
 * [row_begin, row_end) of the width x height frame.
 *   ray_dir       float4, the reference passes (0,0,-1,-1) (MainState.cpp:37-39)
 *   ray_origins   NULL for the reference's implicit (x, y, 0, 1) grid
 *                 (MainState.cpp:44-50), else float4[width*height] (full
 *                 frame; only rows [row_begin, row_end) are uploaded, and
 *                 origins that are bit for bit that grid are recognised on
 *                 the device and keep the binned path)
 *   host_out      int32[4*width*rows] (I32X4), uint32[width*rows] (RGBA8)
 *                 or rt_hit[width*rows] (HIT)
 *   timing        may be NULL
 * Empty scenes are legal (all pixels (0,0,0,255); HIT: all {300000, -1}). */
int rt_render(rt_ctx* ctx, const rt_scene* scene, const float ray_dir[4],
              const float* ray_origins, int32_t width, int32_t height,
              int32_t row_begin, int32_t row_end, int32_t out_format,
              void* host_out, rt_timing* timing);

/* Same as rt_render with an explicit path (RT_PATH_*).  RT_PATH_BINNED
 * returns RT_ERR_UNSUPPORTED when its preconditions do not hold. */
int rt_render_path(rt_ctx* ctx, const rt_scene* scene, const float ray_dir[4],
                   const float* ray_origins, int32_t width, int32_t height,
                   int32_t row_begin, int32_t row_end, int32_t out_format,
                   int32_t path, void* host_out, rt_timing* timing);

/* In-process multi-GPU render (SURVEY.md §8b/§8e rt_render_multi; the
 * reference is single-device, MainState.cpp:1241-1266).  Rows
 * [row_begin, row_end) are split into num_ctx contiguous bands of whole rows
 * (sizes differ by at most one row); band i is rendered on ctxs[i] (one
 * context per device, e.g. rt_init(i)) from its own host thread, straight
 * into its rows of host_out, so no gather step exists: the bands are
 * disjoint slices of the row-major frame (MainState.cpp:676 `pixels`).
 * Synchronous.  timings, if not NULL, gets one rt_timing per context
 * (zeroed for contexts left idle when num_ctx exceeds the row count).
 * Returns the first failing band's status. */
int rt_render_multi(rt_ctx* const* ctxs, int32_t num_ctx, const rt_scene* scene,
                    const float ray_dir[4], const float* ray_origins, int32_t width,
                    int32_t height, int32_t row_begin, int32_t row_end,
                    int32_t out_format, void* host_out, rt_timing* timings);

/* Device-resident variant (no reference counterpart; used by the multi-GPU
 * row-band driver and the benchmark): every pointer in `device_scene`,
 * `device_ray_origins` and `device_out` is a device pointer on the context's
 * device, `stream` is a hipStream_t (NULL = the context's stream).
 * Asynchronous: work is enqueued on `stream` and the call returns.
 * Renders on one context share its workspace (primitive records, candidate
 * lists): enqueue them on one stream, or synchronise before switching
 * streams.  Concurrent renders need one context each.
 * `device_out` must be aligned to the pixel: 16 bytes for I32X4, 4 for RGBA8,
 * 8 for HIT (one 8-byte store per pixel). */
int rt_render_device(rt_ctx* ctx, const rt_scene* device_scene,
                     const float ray_dir[4], const float* device_ray_origins,
                     int32_t width, int32_t height, int32_t row_begin,
                     int32_t row_end, int32_t out_format, int32_t path,
                     void* device_out, void* stream);

/* ---- multi-rank frame assembly over xGMI ------------- */
/* No reference counterpart (the reference is single-device,
 * MainState.cpp:1241-1266).  One process per GPU: the root allocates the
 * whole frame with rt_shared_alloc and hands the 64-byte handle to the
 * other ranks (any transport, e.g. a broadcast); each rank maps it with
 * rt_shared_open and passes `mapped + its first row` as rt_render_device's
 * device_out, so the trace kernel's framebuffer stores travel over xGMI
 * straight into the root's frame and no separate gather copy exists.
 * rt_shared_close unmaps an opened frame, rt_shared_free releases the
 * root's allocation (after every rank has closed it). */
typedef struct rt_ipc_handle {
    unsigned char bytes[64];
} rt_ipc_handle;
int rt_shared_alloc(rt_ctx* ctx, int64_t bytes, void** device_ptr, rt_ipc_handle* handle);
int rt_shared_open(rt_ctx* ctx, const rt_ipc_handle* handle, void** device_ptr);
int rt_shared_close(rt_ctx* ctx, void* device_ptr);
int rt_shared_free(rt_ctx* ctx, void* device_ptr);

/* Page-lock (and unlock) a caller-owned host buffer, e.g. the app's
 * `pixels` vector (MainState.cpp:215, :676), so that rt_render's frame
 * download is a direct DMA at the PCIe link rate instead of a staged copy.
 * Portable: every context / device may use it.  The reference maps and
 * copies an OpenCL buffer instead (MainState.cpp:876-907). */
int rt_host_register(void* host_ptr, int64_t bytes);
int rt_host_unregister(void* host_ptr);

/* Per-kernel HIP-event profiling of rt_render_device / rt_render launches.
 * rt_profile_enable(ctx, 1) starts recording; rt_profile_read synchronises,
 * returns the summed milliseconds of the prep, bin and trace kernels and the
 * number of renders recorded, then resets the accumulators. */
int rt_profile_enable(rt_ctx* ctx, int enable);
int rt_profile_read(rt_ctx* ctx, double* prep_ms, double* bin_ms,
                    double* trace_ms, int32_t* n_renders);

/* The kernel (RT_KERNEL_*) the last render enqueued on this context did
 * its per-pixel work with (for reports: which path actually ran). */
int rt_last_kernel(rt_ctx* ctx, int32_t* kernel);

/* Device facts for reporting (HBM bytes, CU count, name). */
int rt_device_info(rt_ctx* ctx, char* name, int32_t name_len, int32_t* n_cu,
                   int64_t* total_mem);

/* ---- host-side scene helpers (no GPU needed) ------------------------- */

/* Cube, Cube.cpp:6-83: unit cube, scale, rotate (Rz*Ry*Rx, radians),
 * translate, in place on float4[36]. */
void rt_cube_init(float vertices[144]);
void rt_cube_scale(float vertices[144], float sx, float sy, float sz);
void rt_cube_rotate(float vertices[144], float rx, float ry, float rz);
void rt_cube_translate(float vertices[144], float tx, float ty, float tz);
/* Utility::convertAngleToRadian, Utility.cpp:343-347 */
float rt_deg_to_rad(float degrees);
/* rayDir = perspective(45, 4/3, 0, 100) * (0,0,1,1), MainState.cpp:37-39 */
void rt_primary_ray_dir(float out[4]);

/* MainState::createScene1/2/3 (MainState.cpp:419-639) into caller arrays of
 * capacity 100 spheres / 100 cubes; Random::init(seed) = srand(seed). */
int rt_scene_reference(int32_t scene_id, uint32_t seed, float* sphere_origins,
                       float* sphere_radius, float* sphere_colours,
                       float* cube_vertices, float* cube_colours,
                       int32_t* num_spheres, int32_t* num_cubes);

/* Synthetic N-sphere / M-cube scene (SURVEY.md §8d distributions, seeded
 * splitmix64, object scale k: 1 = sparse, width/640 = dense). */
int rt_scene_synthetic(int32_t width, int32_t height, int32_t num_spheres,
                       int32_t num_cubes, uint64_t seed, float k,
                       float* sphere_origins, float* sphere_radius,
                       float* sphere_colours, float* cube_vertices,
                       float* cube_colours);

/* ---- scene build on the device ---------------- */

/* One Cube method call (Cube.cpp:53-83): scale(vec3), rotate(vec3) with
 * angles in RADIANS (Rz * Ry * Rx, as Cube::rotate), translate(vec3). */
enum { RT_CUBE_SCALE = 1, RT_CUBE_ROTATE = 2, RT_CUBE_TRANSLATE = 3 };
typedef struct rt_cube_op {
    int32_t op;
    float x, y, z;
} rt_cube_op;

/* Replaces building `cubes` on the host (Cube::Cube + its transform calls,
 * MainState.cpp:434-593, :617-638) followed by the vertex upload of
 * executeRayTracerOpenCL (MainState.cpp:646-658, :796-816).  Cube c starts
 * from device_vertices_in[36c .. 36c+35] (float4), or from Cube::Cube's unit
 * cube when device_vertices_in is NULL, and applies
 * device_ops[device_op_offsets[c] .. device_op_offsets[c+1]) in order; the
 * result goes to device_vertices_out (float4[36 * num_cubes], may equal
 * device_vertices_in).  Bit-identical to the rt_cube_* host functions (glibc
 * cosf/sinf restated on the device).  All pointers are device pointers;
 * asynchronous on `stream` (NULL = the context's stream). */
int rt_cube_build_device(rt_ctx* ctx, const rt_cube_op* device_ops,
                         const int32_t* device_op_offsets, int32_t num_cubes,
                         const float* device_vertices_in,
                         float* device_vertices_out, void* stream);

/* rt_scene_synthetic built on the device into device arrays: bit-identical
 * arrays, no host build or upload.  Asynchronous on `stream`. */
int rt_scene_synthetic_device(rt_ctx* ctx, int32_t width, int32_t height,
                              int32_t num_spheres, int32_t num_cubes,
                              uint64_t seed, float k, float* sphere_origins,
                              float* sphere_radius, float* sphere_colours,
                              float* cube_vertices, float* cube_colours,
                              void* stream);

/* Texture conversion (MainState.cpp:1023-1037) on the host. */
void rt_pack_rgba8(const int32_t* frame, int64_t n_pixels, uint32_t* out);

/* Shade a hit buffer exactly as the trace would have (MainState.cpp:396-407,
 * :952-955 / :1023-1037): out_format is RT_FORMAT_I32X4 (out = int32[4 *
 * n_pixels]) or RT_FORMAT_RGBA8 (out = uint32[n_pixels]).  The same float
 * sequence as the trace ((t / 180), 255 - n * 255, scalar * colour) and the
 * reference's x86 (int): NaN and out-of-range values become INT32_MIN.  Only
 * the colour arrays and counts of `scene` are read (host pointers), so a
 * frame can be re-shaded with another colour table without tracing again.
 * Returns RT_ERR_INVALID_ARG for an `object` outside
 * [-1, num_cubes + num_spheres), or any other out_format; `out` may then be
 * partly written. */
int rt_shade_hits(const rt_hit* hits, int64_t n_pixels, const rt_scene* scene,
                  int32_t out_format, void* out);

/* ---- deferred surfaces and diffuse lighting from a hit frame ----------- */
/* No reference counterpart (the reference shades a depth ramp and nothing
 * else).  Input is a band of an RT_FORMAT_HIT frame of implicit origins:
 * hits[(row_end - row_begin) * width], row-major, pixel (x, row_begin + r)
 * with origin ((float)x, (float)y, 0) and direction ray_dir.xyz.  The
 * arithmetic is fp32 with one rounding per operation and is stated in
 * DESIGN.md §3.1a; host and device results are bit-identical.
 *
 * One pixel of rt_hit_surfaces* (16 bytes): the unit normal turned against
 * the ray and, for a cube, which of its twelve triangles was hit (the first
 * in the reference's order whose fp64 test gives the frame's t).  Spheres
 * and misses have triangle = -1; a miss, and a cube pixel whose t none of
 * its triangles reproduces (a hit frame this library did not make), have
 * n = 0. */
typedef struct rt_surface {
    float nx, ny, nz;
    int32_t triangle;
} rt_surface;

/* Host functions, no GPU needed: `hits`, the arrays of `scene` and `out`
 * are host pointers.  rt_light_hits writes rt_shade_hits' pixel with the
 * depth ramp scaled by k = min(1, sum over scene->lights of the positive
 * cosines between the normal and the direction to the light); with
 * num_lights == 0, k = 1 and the frame is rt_shade_hits' frame, and so the
 * trace's, bit for bit.  out_format is RT_FORMAT_I32X4 or RT_FORMAT_RGBA8.
 * RT_ERR_INVALID_ARG: a NULL pointer, width < 1, row_begin < 0, row_end <=
 * row_begin, width or row_end above 2^24, a negative count, an array
 * missing for a non-zero count, another out_format, or an `object` outside
 * [-1, num_cubes + num_spheres) (`out` may then be partly written). */
int rt_hit_surfaces(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                    int32_t width, int32_t row_begin, int32_t row_end, rt_surface* out);
int rt_light_hits(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                  int32_t width, int32_t row_begin, int32_t row_end, int32_t out_format,
                  void* out);

/* The same on the device, one kernel launch: `device_hits`, every pointer in
 * `device_scene` and `device_out` are device pointers on the context's
 * device (the rt_scene struct itself and ray_dir are read on the host
 * during the call).  Asynchronous on `stream` (NULL = the context's stream),
 * so a trace into a hit frame and its lighting can follow each other on one
 * stream with no host synchronisation.  `device_hits` must be 8-byte
 * aligned and `device_out` aligned to its pixel: 16 bytes for surfaces and
 * I32X4, 4 for RGBA8; a misaligned pointer is RT_ERR_INVALID_ARG, as is
 * everything the host functions check except the object ids: a kernel
 * returns no status, so it range-checks `object` before any index and
 * treats an id outside [-1, num_cubes + num_spheres) as -1 (no object:
 * zero surface, k = 1 and the colour (0, 0, 0)).  RT_ERR_UNSUPPORTED for
 * a band of 2^39 pixels or more (one launch's grid). */
int rt_hit_surfaces_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                           const float ray_dir[4], int32_t width, int32_t row_begin,
                           int32_t row_end, rt_surface* device_out, void* stream);
int rt_light_hits_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                         const float ray_dir[4], int32_t width, int32_t row_begin,
                         int32_t row_end, int32_t out_format, void* device_out, void* stream);

/* ---- hard shadows for the light pass ----------------- */
/* For each hit pixel and each light that faces it (the cosine c of
 * rt_light_hits is > 0), an any-hit test of the segment from the hit point
 * to the light against every other object of the scene: all twelve
 * triangles of every other cube (the reference's fp64 test, strictly between
 * the hit point and the light) and every other sphere (fp32).  The pixel's
 * own object is never an occluder: cubes and spheres are convex, so no bias
 * constant exists and none is needed.
 *
 * rt_shadow_hits*: one uint32 per pixel; bit i is set iff light i faces the
 * pixel and is occluded.  Misses give 0.  RT_ERR_UNSUPPORTED for more than
 * 32 lights (these two calls only).
 * rt_light_hits_shadowed*: rt_light_hits* with the occluded lights left out
 * of the sum k; any number of lights.  With num_lights == 0 it is
 * rt_shade_hits' frame; a lit pixel whose lights are all occluded is
 * (0, 0, 0, 255).
 *
 * Arguments, alignment (the mask: 4 bytes), the 2^39-pixel launch limit, the
 * handling of `object` (the host functions refuse an id outside
 * [-1, num_cubes + num_spheres), the kernel treats it as -1) and asynchrony
 * are those of rt_light_hits / rt_light_hits_device.  Host and device
 * results are bit-identical. */
int rt_shadow_hits(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                   int32_t width, int32_t row_begin, int32_t row_end, uint32_t* out);
int rt_light_hits_shadowed(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                           int32_t width, int32_t row_begin, int32_t row_end,
                           int32_t out_format, void* out);
int rt_shadow_hits_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                          const float ray_dir[4], int32_t width, int32_t row_begin,
                          int32_t row_end, uint32_t* device_out, void* stream);
int rt_light_hits_shadowed_device(rt_ctx* ctx, const rt_hit* device_hits,
                                  const rt_scene* device_scene, const float ray_dir[4],
                                  int32_t width, int32_t row_begin, int32_t row_end,
                                  int32_t out_format, void* device_out, void* stream);

/* ---- mirror reflections for the light pass ------------ */
/* For each hit pixel, the closest hit of the ray that leaves the hit point p
 * along the mirrored direction R = d - 2 (n . d) n (n: the faced unit normal
 * of rt_hit_surfaces; R is not normalised), over every other object of the
 * scene: all twelve triangles of every other cube (the reference's fp64 test
 * on p and R, t > 0) and every other sphere (fp32; the far root where p lies
 * inside it).  Cubes first, then spheres, each in slot order; a candidate
 * wins iff it is strictly nearer, so ties go to the first.  The pixel's own
 * object is never a candidate: cubes and spheres are convex and the mirrored
 * ray leaves its surface, so no bias constant exists and none is needed.
 * Renders cast no secondary rays; this is a post-pass over a hit frame.
 *
 * rt_reflect_hits*: one rt_hit per pixel, the bounce: the parameter along R
 * and the colour slot met.  (300000, -1) where the bounce meets nothing, for
 * a primary miss, and for a pixel whose normal is NaN.
 * rt_light_hits_reflected*: rt_light_hits* (no shadows) blended with what
 * each pixel mirrors: per channel a + reflectivity * (b - a), a the pixel's
 * own lit channel and b the lit channel of the bounce's hit point, whose
 * depth ramp runs over t + the bounce's parameter and is clamped at 0 from
 * below (0 where the bounce misses).  reflectivity == 0 gives rt_light_hits'
 * frame word for word, without a walk; misses and pixels with t == 300000
 * are rt_light_hits' pixels for every reflectivity.
 *
 * RT_ERR_INVALID_ARG for a reflectivity outside [0, 1] or NaN.  Arguments,
 * alignment (the bounce frame: 8 bytes), the 2^39-pixel launch limit, the
 * handling of `object` (the host functions refuse an id outside
 * [-1, num_cubes + num_spheres), the kernel treats it as -1) and asynchrony
 * are those of rt_light_hits / rt_light_hits_device.  Host and device
 * results are bit-identical. */
int rt_reflect_hits(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                    int32_t width, int32_t row_begin, int32_t row_end, rt_hit* out);
int rt_light_hits_reflected(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                            int32_t width, int32_t row_begin, int32_t row_end,
                            float reflectivity, int32_t out_format, void* out);
int rt_reflect_hits_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                           const float ray_dir[4], int32_t width, int32_t row_begin,
                           int32_t row_end, rt_hit* device_out, void* stream);
int rt_light_hits_reflected_device(rt_ctx* ctx, const rt_hit* device_hits,
                                   const rt_scene* device_scene, const float ray_dir[4],
                                   int32_t width, int32_t row_begin, int32_t row_end,
                                   float reflectivity, int32_t out_format, void* device_out,
                                   void* stream);

/* ---- shadows and mirror reflections together ---------- */
/* The light pass with all three terms: the shadowed direct light of
 * rt_light_hits_shadowed* at the hit point p, the bounce of rt_reflect_hits*,
 * and the shadowed direct light at the point p2 the bounce meets, blended as
 * rt_light_hits_reflected* blends.
 *
 * rt_light_hits_shadowed_reflected*: rt_light_hits_reflected* with the
 * occluded lights left out of both sums: of k at p (occluders: every object
 * but the pixel's own) and of k2 at p2 (occluders: every object but the one
 * the bounce met).  reflectivity == 0 gives rt_light_hits_shadowed's frame
 * word for word, without the bounce and without the second shadow walk;
 * misses and pixels with t == 300000 are rt_light_hits_shadowed's pixels for
 * every reflectivity; without lights it is rt_light_hits_reflected's frame.
 * rt_shadow_hits_reflected*: one uint32 per pixel, rt_shadow_hits' mask taken
 * at p2: bit i is set iff light i faces p2 (against the bounce's normal there,
 * turned against R) and an object other than the one the bounce met cuts the
 * segment from p2 to the light.  0 for a primary miss, without lights, and
 * where the bounce meets nothing; t == 300000 is not looked at, as in
 * rt_reflect_hits.  RT_ERR_UNSUPPORTED for more than 32 lights (these two
 * calls only).
 *
 * Who is left out at p2: the object the bounce met, always, and only it.  The
 * primary pixel's own object occludes at p2 like any other (a sphere hovering
 * over a face shadows the point of the face that its own flank mirrors).
 * This is exact where the bounce arrives from outside the object it met (the
 * convexity argument of the shadow term).  It is not exact where the bounce
 * arrives from inside it -- the far root of a sphere that holds p, or a
 * triangle of an intersecting cube met from within: there the normal at p2 is
 * turned inward, and the object's own far side could hide a facing light but
 * is left out all the same.
 *
 * RT_ERR_INVALID_ARG for a reflectivity outside [0, 1] or NaN.  Arguments,
 * alignment (the mask: 4 bytes), the 2^39-pixel launch limit, the handling of
 * `object` (the host functions refuse an id outside
 * [-1, num_cubes + num_spheres), the kernel treats it as -1) and asynchrony
 * are those of rt_light_hits / rt_light_hits_device; one launch, no
 * workspace.  Host and device results are bit-identical. */
int rt_shadow_hits_reflected(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                             int32_t width, int32_t row_begin, int32_t row_end, uint32_t* out);
int rt_light_hits_shadowed_reflected(const rt_hit* hits, const rt_scene* scene,
                                     const float ray_dir[4], int32_t width, int32_t row_begin,
                                     int32_t row_end, float reflectivity, int32_t out_format,
                                     void* out);
int rt_shadow_hits_reflected_device(rt_ctx* ctx, const rt_hit* device_hits,
                                    const rt_scene* device_scene, const float ray_dir[4],
                                    int32_t width, int32_t row_begin, int32_t row_end,
                                    uint32_t* device_out, void* stream);
int rt_light_hits_shadowed_reflected_device(rt_ctx* ctx, const rt_hit* device_hits,
                                            const rt_scene* device_scene, const float ray_dir[4],
                                            int32_t width, int32_t row_begin, int32_t row_end,
                                            float reflectivity, int32_t out_format,
                                            void* device_out, void* stream);

/* ---- mirror chains, reflectivity per object ----------- */
/* The bounce of rt_reflect_hits* taken again from the point it meets, up to
 * RT_MAX_BOUNCES times, with one reflectivity per colour slot.
 *
 * Level 0 of a pixel's chain is the pixel itself (object, hit point p_0, faced
 * normal n_0, direction D_0 = ray_dir, depth T_0 = t).  From level j the chain
 * goes on iff j < max_bounces and reflectivity[obj_j] != 0: along
 * R_j = mirror(n_j, D_j), over every object but obj_j alone (the primary
 * object and every earlier one are candidates again), to the closest hit; its
 * object, point, faced normal, R_j and T_j + the bounce's parameter are level
 * j + 1.  A level's own colour is a_j = (ramp(T_j) * k_j) * colour_j, the ramp
 * clamped at 0 from below for j >= 1, k_j the direct light at p_j (shadowed
 * with `shadows`: occluders are every object but obj_j; 1 without lights).
 * Where the chain ends at a level its colour is that level's own; where it
 * ends in a miss, black.  Backwards from there,
 * C_j = a_j + reflectivity[obj_j] * (C_{j+1} - a_j), and the pixel is
 * (int)C_0, alpha 255.
 *
 * rt_light_hits_mirrored*: that frame.  reflectivity: num_cubes + num_spheres
 * floats by colour slot (cubes, then spheres).  max_bounces == 1 with one
 * value r everywhere is rt_light_hits_reflected's frame word for word (with
 * `shadows`, rt_light_hits_shadowed_reflected's); max_bounces == 0, or an
 * all-zero array, is rt_light_hits' (rt_light_hits_shadowed's), without a
 * walk.  Misses and pixels with t == 300000 are those functions' pixels for
 * every array and depth.
 * rt_bounce_hits*: one rt_hit per pixel, the geometry of bounce number
 * `bounce` (1-based) of that chain, followed without regard to reflectivity,
 * lights or t: the parameter along R_{bounce-1} and the colour slot met.
 * (300000, -1) for a primary miss, where this bounce or an earlier one meets
 * nothing, and where a normal is NaN.  bounce == 1 is rt_reflect_hits' frame.
 *
 * Leaving only the current object out is exact where a bounce arrives from
 * outside the object it meets, and has the inexactness stated above for
 * rt_shadow_hits_reflected where it arrives from inside: the next bounce and
 * the shadow walk there leave that object out all the same.
 *
 * RT_ERR_INVALID_ARG for max_bounces outside [0, RT_MAX_BOUNCES], bounce
 * outside [1, RT_MAX_BOUNCES], shadows other than 0 or 1, a NULL reflectivity
 * while max_bounces > 0 and the scene has objects, and (host) any
 * reflectivity[i] outside [0, 1] or NaN.  The device calls check what the host
 * can see, the 4-byte alignment of device_reflectivity included; the kernel
 * reads a value outside [0, 1], NaN included, as 0.  Arguments, alignment (the
 * bounce frame: 8 bytes), the 2^39-pixel launch limit, the handling of
 * `object` and asynchrony are those of rt_light_hits / rt_light_hits_device;
 * one launch, no workspace.  Host and device results are bit-identical. */
#define RT_MAX_BOUNCES 8
int rt_bounce_hits(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                   int32_t width, int32_t row_begin, int32_t row_end, int32_t bounce,
                   rt_hit* out);
int rt_bounce_hits_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                          const float ray_dir[4], int32_t width, int32_t row_begin,
                          int32_t row_end, int32_t bounce, rt_hit* device_out, void* stream);
int rt_light_hits_mirrored(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                           int32_t width, int32_t row_begin, int32_t row_end,
                           const float* reflectivity, int32_t max_bounces, int32_t shadows,
                           int32_t out_format, void* out);
int rt_light_hits_mirrored_device(rt_ctx* ctx, const rt_hit* device_hits,
                                  const rt_scene* device_scene, const float ray_dir[4],
                                  int32_t width, int32_t row_begin, int32_t row_end,
                                  const float* device_reflectivity, int32_t max_bounces,
                                  int32_t shadows, int32_t out_format, void* device_out,
                                  void* stream);

/* ---- ray queries: the caller's own rays, and a camera --- */
/* No reference counterpart (the reference traces its own orthographic grid
 * and nothing else).  The two walks of the light pass, over rays the caller
 * chose: a picking ray, a perspective view, ambient-occlusion or probe rays.
 *
 * rt_cast_rays*: per ray the closest hit from the origin o along the direction
 * d (not normalised: the parameter is in units of |d|), over every object but
 * `skip`: all twelve triangles of every cube (the reference's fp64 test on the
 * doubles of o and d, a candidate iff it hits with td > 0, at (float)td), then
 * every sphere (fp32, the quadratic of §3.1b: the near root where it is > 0,
 * else the far one where that is > 0, so an origin inside a sphere gives its
 * far side).  A candidate is taken iff it is strictly nearer than 300000 and
 * everything before it, so ties go to the first in that order.  out_hits[i] is
 * the parameter and the colour slot met, (300000, -1) for a miss;
 * out_triangle, where it is not NULL, gets the cube triangle met (0..11), -1
 * on a sphere or a miss.  This is rt_light::bounce_walk as it is: the bounce
 * of rt_reflect_hits from a point and along a direction of the caller's.
 * rt_occlude_rays*: one byte per ray, 1 iff some object other than `skip`
 * cuts the open segment (o, o + d): a triangle at 0 < td < 1, a sphere with a
 * root in (0, 1).  The segment's end is at parameter 1, so the caller scales
 * d.  This is rt_light::light_occluded, the any-hit test of rt_shadow_hits.
 *
 * These are the secondary-ray tests: forward only, and the quadratic sphere.
 * They are not the render's `collide`, which also takes triangles behind the
 * origin (t < 0) and tests spheres through dot4 with w and tca: a cast of the
 * library's own primary rays (rt_camera_reference) is NOT claimed to equal an
 * RT_FORMAT_HIT frame.
 *
 * `skip` is compared and never used as an index.  The host functions refuse
 * (RT_ERR_INVALID_ARG; the outputs may then be partly written) a skip outside
 * [-1, num_cubes + num_spheres); a kernel returns no status and treats such an
 * id as -1.  Nothing else about a ray is special: NaN, infinite or zero
 * origins and directions fall out of the comparisons as "no candidate" and
 * "not occluded", the same on host and device.
 *
 * A camera is affine in the pixel: pixel (x, y) has the origin
 * (o0 + x * ou) + y * ov and the direction (d0 + x * du) + y * dv, per
 * component in fp32 with x and y as floats (exact: width and rows are at most
 * 2^24), and with `normalise` the direction divided by its length
 * sqrtf((dx * dx + dy * dy) + dz * dz), three divisions.  That covers the
 * orthographic grid and the pinhole.
 * rt_camera_rays*: rows [row_begin, row_end) of a frame `width` wide as rays,
 * row-major: ray i is pixel (i % width, row_begin + i / width), skip = -1,
 * reserved = 0.
 * rt_cast_camera*: word for word what rt_cast_rays* gives on those rays; on
 * the device in one launch and without the ray buffer (32 bytes per pixel).
 * rt_camera_reference: the library's own primary rays, origin (x, y, 0) and
 * direction ray_dir.xyz, not normalised (a -0 component comes out of the
 * camera's sum as +0).
 * rt_camera_pinhole: a pinhole at `eye` looking at `target`, `fov_y_degrees`
 * over the frame's height, square pixels; the direction goes through the
 * CENTRE of pixel (x, y), row 0 at the top (towards `up`), x growing along
 * cross(target - eye, up) (a right-handed view); normalise = 1.  Computed in double and rounded to float once; a convenience in front of
 * the exact part, with no bit-exactness claim of its own.  RT_ERR_INVALID_ARG
 * for NULL, a non-finite input, fov outside (0, 180), width or height < 1,
 * eye == target, or `up` zero or parallel to the view.
 *
 * RT_ERR_INVALID_ARG: a NULL rays, scene, camera or output (out_triangle may
 * be NULL), n < 0, normalise other than 0 or 1, the scene and band checks of
 * rt_light_hits, a misaligned pointer (rays 16 bytes, hits 8, triangles 4).
 * n == 0 is RT_OK and does nothing.  RT_ERR_UNSUPPORTED above 2^39 - 256 rays
 * (one launch's grid, as in the light pass).  The outputs must not overlap
 * `rays`; that is not checked.  Device calls: every array pointer is a device
 * pointer (the rt_scene and rt_camera structs are read on the host during the
 * call); everything above is checked before any HIP call; asynchronous on
 * `stream` (NULL = the context's stream); one launch, no workspace, no
 * allocation.  Host and device results are bit-identical. */
typedef struct rt_ray {      /* 32 bytes; arrays of them 16-byte aligned */
    float ox, oy, oz;        /* origin */
    int32_t skip;            /* colour slot left out of the walk (cubes, then spheres), or -1 */
    float dx, dy, dz;        /* direction, not normalised by the queries */
    float reserved;          /* written 0 by rt_camera_rays*, never read */
} rt_ray;

typedef struct rt_camera {
    float o0[3], ou[3], ov[3];   /* origin of pixel (x, y):    (o0 + x*ou) + y*ov */
    float d0[3], du[3], dv[3];   /* direction of pixel (x, y): (d0 + x*du) + y*dv */
    int32_t normalise;           /* 1: d = d / |d|, 0: as computed */
} rt_camera;

int rt_cast_rays(const rt_ray* rays, int64_t n, const rt_scene* scene, rt_hit* out_hits,
                 int32_t* out_triangle);
int rt_occlude_rays(const rt_ray* rays, int64_t n, const rt_scene* scene, uint8_t* out_occluded);
int rt_camera_rays(const rt_camera* camera, int32_t width, int32_t row_begin, int32_t row_end,
                   rt_ray* out_rays);
int rt_cast_camera(const rt_camera* camera, const rt_scene* scene, int32_t width,
                   int32_t row_begin, int32_t row_end, rt_hit* out_hits, int32_t* out_triangle);
int rt_cast_rays_device(rt_ctx* ctx, const rt_ray* device_rays, int64_t n,
                        const rt_scene* device_scene, rt_hit* device_out_hits,
                        int32_t* device_out_triangle, void* stream);
int rt_occlude_rays_device(rt_ctx* ctx, const rt_ray* device_rays, int64_t n,
                           const rt_scene* device_scene, uint8_t* device_out_occluded,
                           void* stream);
int rt_camera_rays_device(rt_ctx* ctx, const rt_camera* camera, int32_t width, int32_t row_begin,
                          int32_t row_end, rt_ray* device_out_rays, void* stream);
int rt_cast_camera_device(rt_ctx* ctx, const rt_camera* camera, const rt_scene* device_scene,
                          int32_t width, int32_t row_begin, int32_t row_end,
                          rt_hit* device_out_hits, int32_t* device_out_triangle, void* stream);
int rt_camera_pinhole(const float eye[3], const float target[3], const float up[3],
                      float fov_y_degrees, int32_t width, int32_t height, rt_camera* out);
int rt_camera_reference(const float ray_dir[4], rt_camera* out);

/* ---- culled ray queries from prebuilt cube bounds ------- */
/* The ray queries above test every ray against all twelve triangles of every
 * cube.  A caller may build one small record per cube once per scene and pass
 * it to the *_accel forms of the three queries: a cube whose record proves
 * that none of its triangles can be accepted for a ray is left out for that
 * ray.  The results are the unculled calls' results word for word, on every
 * input: the keep test (rt_light::cube_kept) allows for the
 * rounding of the exact fp64 triangle test and keeps a cube whenever a miss is
 * not proven, always for a non-finite ray, for a cube with a non-finite
 * vertex, and for a ray within rounding of grazing one of the cube's
 * triangles.  Spheres are not culled.
 *
 * rt_cube_bound: lo / hi are the exact minimum / maximum of the cube's 36
 * vertices' x, y, z (w ignored); emax2 is the largest squared length of the 24
 * edges v1 - v0 and v2 - v0 of its twelve triangles, computed in double and
 * rounded up to float; normal[k] is e1 x e2 of triangle k in double.  A cube
 * with a non-finite vertex coordinate has lo = -inf, hi = +inf, emax2 = +inf
 * and zero normals.  A record is a function of its cube's vertices alone.
 * rt_accel_build*: out[j] for every cube j of the scene.  Host and device
 * records are bit-identical.  Rebuild after any change of cube_vertices.
 * rt_*_accel*: the unculled call's arguments and contract, plus `accel`:
 * num_cubes records as rt_accel_build* wrote them for THIS scene's vertices.
 * A stale or foreign accel is not detectable and gives wrong results.
 * rt_accel_kept: per ray the number of cubes other than its `skip` that the
 * keep test keeps (segment = 0: the cast's test, 1: the occlusion test's).
 *
 * RT_ERR_INVALID_ARG: what the unculled call refuses; a NULL scene or, with
 * num_cubes > 0, a NULL or misaligned (16 bytes) accel / out; segment other
 * than 0 or 1; a NULL out_count.  num_cubes == 0: RT_OK, accel and out may be
 * NULL, the build launches nothing.  Device calls: checked before any HIP
 * call; asynchronous on `stream`; one launch, no workspace, no allocation. */
typedef struct rt_cube_bound { /* 320 bytes; arrays of them 16-byte aligned */
    float lo[3];
    float emax2;
    float hi[3];
    float reserved;            /* 0 */
    double normal[12][3];
} rt_cube_bound;

int rt_accel_build(const rt_scene* scene, rt_cube_bound* out);
int rt_accel_build_device(rt_ctx* ctx, const rt_scene* device_scene, rt_cube_bound* device_out,
                          void* stream);
int rt_accel_kept(const rt_ray* rays, int64_t n, const rt_scene* scene,
                  const rt_cube_bound* accel, int32_t segment, int32_t* out_count);
int rt_cast_rays_accel(const rt_ray* rays, int64_t n, const rt_scene* scene,
                       const rt_cube_bound* accel, rt_hit* out_hits, int32_t* out_triangle);
int rt_occlude_rays_accel(const rt_ray* rays, int64_t n, const rt_scene* scene,
                          const rt_cube_bound* accel, uint8_t* out_occluded);
int rt_cast_camera_accel(const rt_camera* camera, const rt_scene* scene,
                         const rt_cube_bound* accel, int32_t width, int32_t row_begin,
                         int32_t row_end, rt_hit* out_hits, int32_t* out_triangle);
int rt_cast_rays_accel_device(rt_ctx* ctx, const rt_ray* device_rays, int64_t n,
                              const rt_scene* device_scene, const rt_cube_bound* device_accel,
                              rt_hit* device_out_hits, int32_t* device_out_triangle,
                              void* stream);
int rt_occlude_rays_accel_device(rt_ctx* ctx, const rt_ray* device_rays, int64_t n,
                                 const rt_scene* device_scene, const rt_cube_bound* device_accel,
                                 uint8_t* device_out_occluded, void* stream);
int rt_cast_camera_accel_device(rt_ctx* ctx, const rt_camera* camera, const rt_scene* device_scene,
                                const rt_cube_bound* device_accel, int32_t width,
                                int32_t row_begin, int32_t row_end, rt_hit* device_out_hits,
                                int32_t* device_out_triangle, void* stream);

/* ---- the light pass over the same records ---------------- */
/* The walks of the deferred light pass, culled by the records above: each call
 * is the call of the same name without `_accel`, with `accel` directly after
 * the scene, and returns that call's output word for word on every input.  A
 * pixel tests cube j only where j is not its own and the keep test keeps j for
 * its shadow segment (the occlusion test's form) or its bounce (the cast's).
 * Order, tie rule, early-outs, the sphere loops, the level loop and the
 * backward blend are the unculled calls'.
 *
 * rt_shadow_hits_accel*: rt_shadow_hits*' uint32 mask per pixel.
 * rt_bounce_hits_accel*: rt_bounce_hits*' hit frame of bounce 1 ..
 * RT_MAX_BOUNCES (bounce 1 is rt_reflect_hits*' frame).
 * rt_light_hits_mirrored_accel*: rt_light_hits_mirrored*' lit frame; with
 * max_bounces 0 and shadows 1 that is rt_light_hits_shadowed*' frame, with
 * max_bounces 1 and one reflectivity everywhere rt_light_hits_reflected*' and
 * rt_light_hits_shadowed_reflected*', so the three calls cover every lit frame.
 *
 * The unculled call's contract, and RT_ERR_INVALID_ARG for a NULL or
 * misaligned (16 bytes) accel with num_cubes > 0; with num_cubes == 0 accel
 * may be NULL.  A stale or foreign accel is not detectable.  Device calls:
 * checked before any HIP call; asynchronous on `stream`; one launch, no
 * workspace. */
int rt_shadow_hits_accel(const rt_hit* hits, const rt_scene* scene, const rt_cube_bound* accel,
                         const float ray_dir[4], int32_t width, int32_t row_begin,
                         int32_t row_end, uint32_t* out);
int rt_shadow_hits_accel_device(rt_ctx* ctx, const rt_hit* device_hits,
                                const rt_scene* device_scene, const rt_cube_bound* device_accel,
                                const float ray_dir[4], int32_t width, int32_t row_begin,
                                int32_t row_end, uint32_t* device_out, void* stream);
int rt_bounce_hits_accel(const rt_hit* hits, const rt_scene* scene, const rt_cube_bound* accel,
                         const float ray_dir[4], int32_t width, int32_t row_begin,
                         int32_t row_end, int32_t bounce, rt_hit* out);
int rt_bounce_hits_accel_device(rt_ctx* ctx, const rt_hit* device_hits,
                                const rt_scene* device_scene, const rt_cube_bound* device_accel,
                                const float ray_dir[4], int32_t width, int32_t row_begin,
                                int32_t row_end, int32_t bounce, rt_hit* device_out,
                                void* stream);
int rt_light_hits_mirrored_accel(const rt_hit* hits, const rt_scene* scene,
                                 const rt_cube_bound* accel, const float ray_dir[4],
                                 int32_t width, int32_t row_begin, int32_t row_end,
                                 const float* reflectivity, int32_t max_bounces, int32_t shadows,
                                 int32_t out_format, void* out);
int rt_light_hits_mirrored_accel_device(rt_ctx* ctx, const rt_hit* device_hits,
                                        const rt_scene* device_scene,
                                        const rt_cube_bound* device_accel, const float ray_dir[4],
                                        int32_t width, int32_t row_begin, int32_t row_end,
                                        const float* device_reflectivity, int32_t max_bounces,
                                        int32_t shadows, int32_t out_format, void* device_out,
                                        void* stream);

/* ---- the light pass of a camera view --------------------- */
/* A camera's view, lit: diffuse light, hard shadows and mirror chains for the
 * rays of an rt_camera, in one call and without a hit frame.  Pixel (x, y) of
 * the band has the ray of rt_camera_rays*.  Level 0 of its chain is what
 * rt_cast_camera* finds along that ray (closest hit over every object, ties to
 * the first in cube / triangle / sphere order); a pixel whose ray meets nothing
 * is rt_shade_hits' miss pixel (0, 0, 0, 255).  From level 0 on the pixel is
 * rt_light_hits_mirrored*'s: per level the ramp of the summed depth T (level
 * 0's unclamped, later ones clamped at 0) times the lighting factor (with
 * `shadows` the occluded lights left out) times the slot's colour; the chain
 * goes on from level j iff j < max_bounces and reflectivity[obj_j] != 0, by a
 * bounce with obj_j alone left out, and ends at a matte object, at max_bounces
 * or at a miss; the levels are blended backwards, a + r * (C - a).
 *
 * rt_light_camera*: the lit frame, RT_FORMAT_I32X4 or RT_FORMAT_RGBA8.
 * rt_bounce_camera*: the hit frame of `bounce`: 0 is rt_cast_camera*'s frame;
 * 1 .. RT_MAX_BOUNCES the hit of that bounce of the chain, followed without
 * regard to reflectivity, (300000, -1) where it or an earlier level met
 * nothing.
 * For rt_camera_reference(d) without a -0 component in d these are
 * rt_light_hits_mirrored* / rt_bounce_hits* on rt_cast_camera*'s frame, word
 * for word.
 *
 * `accel`: NULL, every walk tests every cube; or the scene's records
 * (rt_accel_build*), every walk is the culled one (the level-0 cast and the
 * bounces by the cast's keep test, the shadow segments by the occlusion
 * test's).  The output is the same word for word.
 *
 * Known limit, as for every bounce: a level reached from inside an object (the
 * eye inside a sphere, whose far root the cast takes) still leaves that object
 * out of the next bounce and of the shadow walks there.
 *
 * RT_ERR_INVALID_ARG: what rt_cast_camera* refuses (a NULL camera, scene or
 * out, normalise other than 0 or 1, the band and scene checks: the band must
 * not be empty, width >= 1 and row_begin < row_end); max_bounces
 * outside [0, RT_MAX_BOUNCES]; bounce outside [0, RT_MAX_BOUNCES]; shadows
 * other than 0 or 1; a format other than the two; a NULL reflectivity with
 * max_bounces > 0 on a scene with objects (otherwise it may be NULL); on the
 * host a reflectivity outside [0, 1] (a kernel reads such a value as 0); an
 * `out` not aligned to 16 (int32x4), 4 (RGBA8) or 8 (rt_hit) bytes; a non-NULL
 * accel not aligned to 16 bytes.  More than 32 lights are served.  Device
 * calls: every array pointer is a device pointer (rt_camera and rt_scene are
 * read on the host during the call); everything is checked before any HIP
 * call; asynchronous on `stream` (NULL = the context's stream); one launch, no
 * workspace, no allocation.  Host and device results are bit-identical. */
int rt_light_camera(const rt_camera* camera, const rt_scene* scene, const rt_cube_bound* accel,
                    int32_t width, int32_t row_begin, int32_t row_end, const float* reflectivity,
                    int32_t max_bounces, int32_t shadows, int32_t out_format, void* out);
int rt_light_camera_device(rt_ctx* ctx, const rt_camera* camera, const rt_scene* device_scene,
                           const rt_cube_bound* device_accel, int32_t width, int32_t row_begin,
                           int32_t row_end, const float* device_reflectivity, int32_t max_bounces,
                           int32_t shadows, int32_t out_format, void* device_out, void* stream);
int rt_bounce_camera(const rt_camera* camera, const rt_scene* scene, const rt_cube_bound* accel,
                     int32_t width, int32_t row_begin, int32_t row_end, int32_t bounce,
                     rt_hit* out);
int rt_bounce_camera_device(rt_ctx* ctx, const rt_camera* camera, const rt_scene* device_scene,
                            const rt_cube_bound* device_accel, int32_t width, int32_t row_begin,
                            int32_t row_end, int32_t bounce, rt_hit* device_out, void* stream);

/* ---- ray queries culled by spatially grouped sphere bounds - */
/* The *_accel queries above still test every ray against every sphere.  A
 * caller may also build one 64-byte record per group of up to 8 nearby spheres
 * and pass the records to the *_grouped forms of the three queries: a group
 * whose record proves that none of its members can be accepted for a ray is
 * left out for that ray.  The results are the unculled and the *_accel calls'
 * results word for word, on every input: a group is kept
 * whenever a miss is not proven, always for a non-finite ray, for a group with
 * a non-finite member, and outside the magnitudes stated there.
 *
 * rt_sphere_group: the spheres are ordered by (Morton key of the centre, index)
 * and cut into runs of `group_size`; a record holds the box of its members
 * (lo = min of centre - |r| rounded down, hi = max of centre + |r| rounded up),
 * the largest |r|, and the members' indices in ascending order (unused slots
 * -1).  A group with a non-finite centre or radius has lo = -inf, hi = +inf,
 * rmax = +inf.  The build is written operation by operation in §3.1j; host and
 * device records are bit-identical.  Rebuild after any change of the spheres.
 * rt_sphere_groups_count: ceil(num_spheres / group_size) records, or -1 for
 * num_spheres < 0 or group_size outside 1..8.
 * rt_sphere_groups_workspace_bytes: the device build's workspace for
 * num_spheres spheres (16 + 8 * num_spheres, rounded up to 16; -1 for
 * num_spheres < 0).
 * rt_sphere_groups_build_device: four launches on `stream`, in order (the
 * bounds of the centres, the keys, the ranks, the records); the ranks count
 * over all keys, num_spheres^2 compares (16 M at 4096 spheres).  No allocation:
 * `device_workspace` is the caller's, 16-byte aligned, at least
 * rt_sphere_groups_workspace_bytes(num_spheres) bytes, and may be reused once
 * the work on `stream` in front of that reuse is ordered behind the build.
 * rt_*_grouped*: the *_accel call's arguments and contract, plus `groups`,
 * `num_groups` directly after `accel`: the records rt_sphere_groups_build*
 * wrote for THIS scene's spheres.  A stale or foreign record is not detectable
 * and gives wrong results (a member index outside the scene is skipped).
 * rt_sphere_groups_kept: per ray the number of groups the keep test keeps
 * (segment = 0: the cast's test, 1: the occlusion test's); host only.
 *
 * RT_ERR_INVALID_ARG: what the *_accel call refuses; group_size outside 1..8;
 * with num_spheres > 0 a NULL or misaligned (16 bytes) groups / out /
 * workspace, a workspace too small, or num_groups that is not
 * rt_sphere_groups_count(num_spheres, g) for any g in 1..8; num_groups != 0
 * with num_spheres == 0; segment other than 0 or 1.  num_spheres == 0: RT_OK,
 * groups / out / workspace may be NULL, the build launches nothing.  Device
 * calls: checked before any HIP call; asynchronous on `stream`; the queries
 * are one launch, no workspace, no allocation. */
typedef struct rt_sphere_group { /* 64 bytes; arrays of them 16-byte aligned */
    float lo[3];
    float rmax;
    float hi[3];
    int32_t count;             /* members, 1..8 */
    int32_t member[8];         /* ascending sphere indices, then -1 */
} rt_sphere_group;

int32_t rt_sphere_groups_count(int32_t num_spheres, int32_t group_size);
int64_t rt_sphere_groups_workspace_bytes(int32_t num_spheres);
int rt_sphere_groups_build(const rt_scene* scene, int32_t group_size, rt_sphere_group* out);
int rt_sphere_groups_build_device(rt_ctx* ctx, const rt_scene* device_scene, int32_t group_size,
                                  rt_sphere_group* device_out, void* device_workspace,
                                  int64_t workspace_bytes, void* stream);
int rt_sphere_groups_kept(const rt_ray* rays, int64_t n, const rt_scene* scene,
                          const rt_sphere_group* groups, int32_t num_groups, int32_t segment,
                          int32_t* out_count);
int rt_cast_rays_grouped(const rt_ray* rays, int64_t n, const rt_scene* scene,
                         const rt_cube_bound* accel, const rt_sphere_group* groups,
                         int32_t num_groups, rt_hit* out_hits, int32_t* out_triangle);
int rt_occlude_rays_grouped(const rt_ray* rays, int64_t n, const rt_scene* scene,
                            const rt_cube_bound* accel, const rt_sphere_group* groups,
                            int32_t num_groups, uint8_t* out_occluded);
int rt_cast_camera_grouped(const rt_camera* camera, const rt_scene* scene,
                           const rt_cube_bound* accel, const rt_sphere_group* groups,
                           int32_t num_groups, int32_t width, int32_t row_begin, int32_t row_end,
                           rt_hit* out_hits, int32_t* out_triangle);
int rt_cast_rays_grouped_device(rt_ctx* ctx, const rt_ray* device_rays, int64_t n,
                                const rt_scene* device_scene, const rt_cube_bound* device_accel,
                                const rt_sphere_group* device_groups, int32_t num_groups,
                                rt_hit* device_out_hits, int32_t* device_out_triangle,
                                void* stream);
int rt_occlude_rays_grouped_device(rt_ctx* ctx, const rt_ray* device_rays, int64_t n,
                                   const rt_scene* device_scene, const rt_cube_bound* device_accel,
                                   const rt_sphere_group* device_groups, int32_t num_groups,
                                   uint8_t* device_out_occluded, void* stream);
int rt_cast_camera_grouped_device(rt_ctx* ctx, const rt_camera* camera,
                                  const rt_scene* device_scene, const rt_cube_bound* device_accel,
                                  const rt_sphere_group* device_groups, int32_t num_groups,
                                  int32_t width, int32_t row_begin, int32_t row_end,
                                  rt_hit* device_out_hits, int32_t* device_out_triangle,
                                  void* stream);

/* Known-answer checksum of a frame: FNV-1a-64 over its 32-bit words in
 * memory order (`h ^= w; h *= 0x100000001b3`), starting from `basis`
 * (RT_FNV1A64_BASIS; the survey's probe of the reference's CPU frames,
 * SURVEY.md §8c, started from 1469598103934665603).  No reference
 * counterpart: the app never checks its frame.  Used by the headless driver,
 * the benchmark's frame check against the committed fixtures and the tests. */
#define RT_FNV1A64_BASIS 0xcbf29ce484222325ull
uint64_t rt_fnv1a64(const void* words, int64_t n_words, uint64_t basis);

/* Library / ABI version. */
int rt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_HIP_H */
