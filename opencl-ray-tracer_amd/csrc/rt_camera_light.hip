// rt_camera_light.hip -- rt_light_camera_device / rt_bounce_camera_device: the
// light pass of a camera view on the device.  The mirror
// chain of rt_light_accel.hip / rt_mirror.hip with level 0 found by a cast of
// the pixel's own ray (cast_kernel<kFromCamera>'s, by camera_ray_at of
// rt_rays_device.inc) instead of read from a hit frame: one launch, no hit
// frame, no workspace, and no fp64 re-identification of the level-0 triangle.
//
// One kernel template over the output (int32x4, RGBA8, bounce frame) and over
// the cull policy of the walks of rt_light_device.inc (KeepAll, or CubeCull of
// rt_accel_impl.h on the prebuilt records).  One pixel per lane in 256-thread
// workgroups.  The level a bounce reaches, the chain's pixel and the entry
// points' preamble are rt_chain_device.inc's and rt_light_impl.h's.  The level
// loop, with the level step, the LDS blend stack (depth * 4 KiB of dynamic
// shared memory; none for the bounce frame) and the unwind, is written here a
// second time, beside hit_chain_kernel's: its shape differs, and with the level
// step and the unwind as functions of both kernels the culled instances were
// up to 1.4 % slower (profiles/chain_shared/README.md).  The shape:
// the level loop is entered one step early: the camera ray is the "bounce"
// that reaches level 0, from own object -1, so the kernel has the two walk
// sites of light_accel_kernel (one closest-hit walk, one shadow walk) and not a
// third copy of the walk in front of the loop.  These kernels are short of
// scalar registers (profiles/light_accel/kernel_resources.md); how this one
// stands is profiles/camera_light/kernel_resources.md: no scratch, no spill.
//
// The scene and the records come through scalar loads (indexed by loop
// counters alone); the per-lane loads are bounce_normal's gathers, the colour
// slot and reflectivity[obj]; one store per pixel.  The lanes of a partial last
// workgroup beyond the band stay in uniform control flow through every ballot:
// they cast nothing, reach no level and store nothing.
//
// rt_init does not load this translation unit's code object: the runtime
// loads it at the first launch of one of its kernels.
#include "rt_light_device.inc"
#ifndef RT_ACCEL_NORMALS_LOOP
#define RT_ACCEL_NORMALS_LOOP _Pragma("clang loop unroll(disable)")
#endif
#include "rt_accel_impl.h"
#include "rt_chain_device.inc"
#include "rt_rays_device.inc"  // camera_ray_at, launch_rays
#include "rt_camera_light_impl.h"

namespace {

using rt_light::CubeCull;

// The policy of an instance over the kernel's `accel` argument.
template <typename Cull>
__device__ __forceinline__ Cull policy(const rt_cube_bound* accel) {
    if constexpr (std::is_same_v<Cull, CubeCull>)
        return CubeCull{accel};
    else
        return KeepAll{};
}

// `s` holds device pointers, `accel` its s.num_cubes records (CubeCull only).
// `depth`: max_bounces of the lit forms (0 .. RT_MAX_BOUNCES; the launch passes
// depth * 4 KiB of shared memory), the bounce's number of the bounce form
// (0 .. RT_MAX_BOUNCES).  `refl`: the lit forms' reflectivity by colour slot.
// (uniform: depth, shadows)
template <int kOut, typename Cull>
__global__ void __launch_bounds__(256)
camera_light_kernel(rt_camera cam, int64_t n, int32_t width, int32_t row_begin,
                    const rt_cube_bound* __restrict__ accel, const float* __restrict__ refl,
                    int32_t depth, int32_t shadows, rt_scene s, void* __restrict__ out) {
    using rt_light::Vec3;
    const int64_t i = pixel_index();
    // The lane's pixel of `out`, NULL for a lane beyond the band.  Formed here
    // and held in two vector registers, which the lane's index would take
    // anyway: `out`, `n` and a lane mask of the band are then scalar registers
    // the level loop does not have to keep for the store behind it.
    constexpr int64_t kPixelBytes = kOut == kOutI32x4 ? 16 : kOut == kOutRgba8 ? 4 : 8;
    char* const dst = i < n ? static_cast<char*>(out) + kPixelBytes * i : nullptr;
    const bool in = dst != nullptr;
    // (every lane: no memory is touched, and the camera stays in scalar registers)
    rt_light::Ray ray = camera_ray_at(cam, i, n, width, row_begin);
    // the ray is six opaque registers from here on, as in rt_rays.hip
    asm("" : "+v"(ray.o.x), "+v"(ray.o.y), "+v"(ray.o.z), "+v"(ray.d.x), "+v"(ray.d.y),
             "+v"(ray.d.z));
    // the walk that reaches level j leaves p along R from the object `cur`:
    // for level 0 the camera ray, from no object
    Vec3 p = ray.o, R = ray.d, nrm{0.0f, 0.0f, 0.0f};
    int32_t cur = -1;
    const Cull cull = policy<Cull>(accel);

    if constexpr (kOut == kOutBounce) {
        rt_light::Bounce b{rt_light::kFar, -1, -1};
        bool live = in;  // the lane casts the next walk
#pragma clang loop unroll(disable)
        for (int32_t j = 0;; ++j) {  // (uniform)
            b = wave_bounce_walk(s, p, R, cur, live, cull);  // (kFar, -1) for the others
            if (j >= depth) break;                           // (uniform)
            live = b.obj2 >= 0;
            if (__ballot(live) == 0) break;  // (uniform)
            if (live) rt_light::next_level(s, b, R, p, nrm, cur);
            R = rt_light::mirror_dir(nrm, R);
        }
        if (dst) *reinterpret_cast<int2*>(dst) = make_int2(__float_as_int(b.best), b.obj2);
    } else {
        const bool lights = s.num_lights > 0;  // (uniform)
        Vec3 C{0.0f, 0.0f, 0.0f};              // a miss at level 0 stays (0, 0, 0)
        float T = 0.0f;
        // (a_j.xyz, r_j) per lane and level; the dynamic region is all the LDS
        // there is, so its base is 16-byte aligned
        extern __shared__ __attribute__((aligned(16))) float4 mirror_stack[];
        float4* const mine = mirror_stack + threadIdx.x;
        bool goes = in;       // the lane casts the walk that reaches the next level
        int32_t pushed = 0;  // the levels this lane went on from
        // (uniform) the level; behind the loop, the levels any lane of the wave
        // went on from: both breaks leave at the level whose walk or push no
        // lane took
        int32_t j = 0;
#pragma clang loop unroll(disable)
        for (;; ++j) {
            const rt_light::Bounce b = wave_bounce_walk(s, p, R, cur, goes, cull);
            const bool live = goes && b.obj2 >= 0;  // a miss leaves C = (0, 0, 0)
            if (__ballot(live) == 0) break;         // (uniform)
            if (live) {
                T = j == 0 ? b.best : T + b.best;
                rt_light::next_level(s, b, R, p, nrm, cur);
            }
            // the own colour of level j, for the lanes that reached it
            float k = 1.0f;
            if (lights) {       // (uniform)
                if (shadows) {  // (uniform)
                    uint32_t unused = 0;
                    k = light_walk<false>(s, p, nrm, cur, live, unused, cull);
                } else if (live) {
                    k = rt_light::light_factor(nrm, p, s.lights, s.num_lights);
                }
            }
            Vec3 a{0.0f, 0.0f, 0.0f};
            float r = 0.0f;
            if (live) {
                a = rt_light::chain_colour(rt_light::chain_scalar(T, j >= 1), k,
                                           rt_light::slot_colour(s, cur));
                if (j < depth) r = rt_light::slot_reflectivity(refl, cur);
            }
            goes = live && r != 0.0f;
            if (live && !goes) C = a;        // ended here by depth or by a matte object
            if (__ballot(goes) == 0) break;  // (uniform) at j == depth at the latest
            // j < depth here, so the push stays inside depth * 4 KiB
            if (goes) {
                mine[256 * pushed] = make_float4(a.x, a.y, a.z, r);
                ++pushed;
            }
            R = rt_light::mirror_dir(nrm, R);
        }
        // the backward blend, from the wave's deepest level down
#pragma clang loop unroll(disable)
        for (int32_t l = j - 1; l >= 0; --l) {  // (uniform)
            if (l < pushed) {
                const float4 e = mine[256 * l];
                C = rt_light::chain_blend(Vec3{e.x, e.y, e.z}, e.w, C);
            }
        }
        if (dst) {
            int32_t lit[4];
            chain_lit(C, lit);
            store_lit<kOut>(dst, 0, lit);
        }
    }
}

// The launch of both entry points.  `align`: of `out`, in bytes.  Every check
// runs before any HIP call.
template <typename Kernel>
int launch_camera(Kernel unculled, Kernel culled, uintptr_t align, rt_ctx* ctx,
                  const rt_camera* camera, const rt_scene* scene, const rt_cube_bound* accel,
                  int32_t width, int32_t row_begin, int32_t row_end, const float* refl,
                  int32_t depth, int32_t shadows, size_t shared, void* out, void* stream) {
    if (!ctx || reinterpret_cast<uintptr_t>(refl) % sizeof(float)) return RT_ERR_INVALID_ARG;
    const int rc = rt_light::check_camera_light(camera, scene, accel, width, row_begin, row_end,
                                                out, align);
    if (rc) return rc;
    // (n >= 1: the checks refuse an empty band; blocks <= INT32_MAX: and more pixels than that)
    const int64_t n = (int64_t)(row_end - row_begin) * width;
    const Kernel kernel = accel ? culled : unculled;  // NULL accel: every walk unculled
    return launch_rays(ctx, n, 256, stream, [&](dim3 grid, hipStream_t st) {
        kernel<<<grid, dim3(256), shared, st>>>(*camera, n, width, row_begin, accel, refl, depth,
                                                shadows, *scene, out);
    });
}

}  // namespace

extern "C" {

int rt_bounce_camera_device(rt_ctx* ctx, const rt_camera* camera, const rt_scene* device_scene,
                            const rt_cube_bound* device_accel, int32_t width, int32_t row_begin,
                            int32_t row_end, int32_t bounce, rt_hit* device_out, void* stream) {
    if (bounce < 0 || bounce > RT_MAX_BOUNCES) return RT_ERR_INVALID_ARG;
    return launch_camera(camera_light_kernel<kOutBounce, KeepAll>,
                         camera_light_kernel<kOutBounce, CubeCull>, 8, ctx, camera, device_scene,
                         device_accel, width, row_begin, row_end, nullptr, bounce, 0, 0,
                         device_out, stream);
}

int rt_light_camera_device(rt_ctx* ctx, const rt_camera* camera, const rt_scene* device_scene,
                           const rt_cube_bound* device_accel, int32_t width, int32_t row_begin,
                           int32_t row_end, const float* device_reflectivity, int32_t max_bounces,
                           int32_t shadows, int32_t out_format, void* device_out, void* stream) {
    int32_t depth;
    size_t shared;
    const int rc = chain_settings(device_scene, device_reflectivity, max_bounces, shadows,
                                  out_format, depth, shared);
    if (rc) return rc;
    if (out_format == RT_FORMAT_I32X4)
        return launch_camera(camera_light_kernel<kOutI32x4, KeepAll>,
                             camera_light_kernel<kOutI32x4, CubeCull>, 16, ctx, camera,
                             device_scene, device_accel, width, row_begin, row_end,
                             device_reflectivity, depth, shadows, shared, device_out, stream);
    return launch_camera(camera_light_kernel<kOutRgba8, KeepAll>,
                         camera_light_kernel<kOutRgba8, CubeCull>, 4, ctx, camera, device_scene,
                         device_accel, width, row_begin, row_end, device_reflectivity, depth,
                         shadows, shared, device_out, stream);
}

}  // extern "C"
