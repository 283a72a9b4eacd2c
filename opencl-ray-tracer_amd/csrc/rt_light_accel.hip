// rt_light_accel.hip -- rt_bounce_hits_accel_device /
// rt_light_hits_mirrored_accel_device: the mirror chain of the deferred light
// pass over the prebuilt cube records, on the device.
// mirror_kernel (rt_mirror.hip) with the walks of rt_light_device.inc culled by
// CubeCull of rt_accel_impl.h: a lane tests a cube only where it is not its own
// and the keep test of include/rt_accel_impl.h keeps it for the lane's shadow
// segment or bounce.  What each call stores is its unculled call's output word
// for word.  The mask, rt_shadow_hits_accel_device, is
// rt_shadow_accel.hip.
//
// One kernel template over the output (int32x4, RGBA8, bounce frame).  The
// level loop, its ballots, the LDS blend stack (depth * 4 KiB of dynamic shared
// memory; none for the bounce frame) and the unwind are rt_mirror.hip's,
// restated so that that file and its kernels stay as they are.  The record
// comes through scalar loads: accel[j] is indexed by the walks' loop counters
// alone.  No workspace, one launch.
//
// Scalar registers are what the lit forms are short of.  The level loop keeps
// the scene's pointers, the record's, the reflectivity's and its own counters
// live across both walks, and the keep test wants the record's twelve normals
// (72 dwords) in flight at once: together that is past the 102 a wave has, and
// the compiler spills 35 of them to lanes of a VGPR.  So the keep test's loop
// over the normals stays a loop here (one normal's six dwords per trip), and
// `out`, which is read once at the end, is the last kernel argument, behind
// the ones that arrive preloaded in registers: no spill, and about 17 VGPRs
// fewer (profiles/light_accel/kernel_resources.md).
//
// rt_init does not load this translation unit's code object: the runtime
// loads it at the first launch of one of its kernels.
#include "rt_light_device.inc"
#ifndef RT_ACCEL_NORMALS_LOOP
#define RT_ACCEL_NORMALS_LOOP _Pragma("clang loop unroll(disable)")
#endif
#include "rt_accel_impl.h"

namespace {

using rt_light::CubeCull;

enum { kOutBounce = 2 };

// The level the bounce `b` met, in place: its point, faced normal, object and
// direction.
__device__ __forceinline__ void next_level(const rt_scene& s, rt_light::Bounce b,
                                           rt_light::Vec3 R, rt_light::Vec3& p,
                                           rt_light::Vec3& nrm, rt_light::Vec3& D, int32_t& cur) {
    const rt_light::Vec3 p2 = rt_light::bounce_point(p, R, b.best);
    nrm = rt_light::bounce_normal(s, b.obj2, b.tri2, p2, R);
    p = p2;
    cur = b.obj2;
    D = R;
}

// `s` holds device pointers, `accel` its s.num_cubes records.  `depth`:
// max_bounces of the lit forms (0 .. RT_MAX_BOUNCES; the launch passes
// depth * 4 KiB of shared memory), the bounce's number of the bounce form
// (1 .. RT_MAX_BOUNCES).  `refl`: the lit forms' reflectivity by colour slot.
// (uniform: depth, shadows)
template <int kOut>
__global__ void __launch_bounds__(256)
light_accel_kernel(const rt_hit* __restrict__ hits, const rt_cube_bound* __restrict__ accel,
                   int64_t n, int32_t width, int32_t row_begin, float dx, float dy, float dz,
                   const float* __restrict__ refl, int32_t depth, int32_t shadows, rt_scene s,
                   void* __restrict__ out) {
    using rt_light::Vec3;
    const int64_t i = pixel_index();
    if (i >= n) return;
    const Vec3 d{dx, dy, dz};
    float ox, oy;
    int32_t obj;
    const float t = load_pixel(hits, i, n, width, row_begin, s, ox, oy, obj);
    const bool hit = obj >= 0;

    if constexpr (kOut == kOutBounce) {
        rt_light::Bounce b{rt_light::kFar, -1, -1};
        Vec3 p{0.0f, 0.0f, 0.0f}, nrm{0.0f, 0.0f, 0.0f}, D = d;
        int32_t cur = obj;
        if (hit) {
            p = rt_light::hit_point(ox, oy, d, t);
            nrm = surface_step(s, obj, ox, oy, d, t, p);
        }
        bool live = hit;  // the lane's chain reaches the current level
#pragma clang loop unroll(disable)
        for (int32_t j = 1; __ballot(live) != 0; ++j) {  // (uniform)
            const Vec3 R = rt_light::mirror_dir(nrm, D);
            // (kFar, -1) for the others
            b = wave_bounce_walk(s, p, R, cur, live, CubeCull{accel});
            if (j >= depth) break;  // (uniform)
            live = b.obj2 >= 0;
            if (live) next_level(s, b, R, p, nrm, D, cur);
        }
        reinterpret_cast<int2*>(out)[i] = make_int2(__float_as_int(b.best), b.obj2);
    } else {
        // the lanes with a chain: the others are lit_pixel's, black or a miss
        const bool chained = hit && !(t == rt_light::kFar);
        const bool lights = s.num_lights > 0;  // (uniform)
        Vec3 C{0.0f, 0.0f, 0.0f};
        if (__ballot(chained) != 0) {  // (uniform)
            Vec3 p{0.0f, 0.0f, 0.0f}, nrm{0.0f, 0.0f, 0.0f}, D = d;
            float T = t;
            int32_t cur = obj;
            if (chained && (lights || depth > 0)) {
                p = rt_light::hit_point(ox, oy, d, t);
                nrm = surface_step(s, obj, ox, oy, d, t, p);
            }
            // (a_j.xyz, r_j) per lane and level; the dynamic region is all the
            // LDS there is, so its base is 16-byte aligned
            extern __shared__ __attribute__((aligned(16))) float4 mirror_stack[];
            float4* const mine = mirror_stack + threadIdx.x;
            bool live = chained;  // the lane's chain reaches the current level
            int32_t pushed = 0;   // the levels this lane went on from
            int32_t deepest = 0;  // (uniform) the levels any lane of the wave went on from
#pragma clang loop unroll(disable)
            for (int32_t j = 0;; ++j) {  // (uniform)
                // the own colour of level j, for the lanes that reached it
                float k = 1.0f;
                if (lights) {  // (uniform)
                    if (shadows) {  // (uniform)
                        uint32_t unused = 0;
                        k = light_walk<false>(s, p, nrm, cur, live, unused, CubeCull{accel});
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
                const bool goes = live && r != 0.0f;
                if (live && !goes) C = a;  // ended here by depth or by a matte object
                if (__ballot(goes) == 0) break;  // (uniform) at j == depth at the latest
                // j < depth here, so the push stays inside depth * 4 KiB
                if (goes) {
                    mine[256 * pushed] = make_float4(a.x, a.y, a.z, r);
                    ++pushed;
                }
                deepest = j + 1;
                const Vec3 R = rt_light::mirror_dir(nrm, D);
                const rt_light::Bounce b = wave_bounce_walk(s, p, R, cur, goes, CubeCull{accel});
                live = goes && b.obj2 >= 0;  // a miss leaves C = (0, 0, 0)
                if (live) {
                    T = T + b.best;
                    next_level(s, b, R, p, nrm, D, cur);
                }
            }
            // the backward blend, from the wave's deepest level down
#pragma clang loop unroll(disable)
            for (int32_t l = deepest - 1; l >= 0; --l) {  // (uniform)
                if (l < pushed) {
                    const float4 e = mine[256 * l];
                    C = rt_light::chain_blend(Vec3{e.x, e.y, e.z}, e.w, C);
                }
            }
        }
        int32_t lit[4];
        if (chained) {
            lit[0] = rt_light::cvt_i32(C.x);
            lit[1] = rt_light::cvt_i32(C.y);
            lit[2] = rt_light::cvt_i32(C.z);
            lit[3] = 255;
        } else {
            rt_light::shade_lit(t, 1.0f, rt_light::slot_colour(s, obj), lit);
        }
        store_lit<kOut>(out, i, lit);
    }
}

// The launch of both entry points: launch_mirror of rt_mirror.hip with the
// record and its check.  `align`: of `out`, in bytes.  Every check runs before
// any HIP call.
template <typename Kernel>
int launch_accel(Kernel kernel, uintptr_t align, rt_ctx* ctx, const rt_hit* hits,
                 const rt_scene* scene, const rt_cube_bound* accel, const float* ray_dir,
                 int32_t width, int32_t row_begin, int32_t row_end, const float* refl,
                 int32_t depth, int32_t shadows, size_t shared, void* out, void* stream) {
    if (!ctx || rt_light::check(hits, scene, ray_dir, width, row_begin, row_end, out) ||
        reinterpret_cast<uintptr_t>(hits) % sizeof(rt_hit) ||
        reinterpret_cast<uintptr_t>(out) % align ||
        reinterpret_cast<uintptr_t>(refl) % sizeof(float))
        return RT_ERR_INVALID_ARG;
    const int64_t n = (int64_t)(row_end - row_begin) * width;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > INT32_MAX) return RT_ERR_UNSUPPORTED;
    if (rt_light::check_accel(scene, accel)) return RT_ERR_INVALID_ARG;
    if (hipSetDevice(rt_internal::ctx_device(ctx)) != hipSuccess) return RT_ERR_HIP;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : rt_internal::ctx_stream(ctx);
    if (!st) return RT_ERR_HIP;
    kernel<<<dim3((unsigned)blocks), dim3(256), shared, st>>>(
        hits, accel, n, width, row_begin, ray_dir[0], ray_dir[1], ray_dir[2], refl, depth,
        shadows, *scene, out);
    return hipGetLastError() == hipSuccess ? RT_OK : RT_ERR_HIP;
}

}  // namespace

extern "C" {

int rt_bounce_hits_accel_device(rt_ctx* ctx, const rt_hit* device_hits,
                                const rt_scene* device_scene, const rt_cube_bound* device_accel,
                                const float ray_dir[4], int32_t width, int32_t row_begin,
                                int32_t row_end, int32_t bounce, rt_hit* device_out,
                                void* stream) {
    if (bounce < 1 || bounce > RT_MAX_BOUNCES) return RT_ERR_INVALID_ARG;
    return launch_accel(light_accel_kernel<kOutBounce>, 8, ctx, device_hits, device_scene,
                        device_accel, ray_dir, width, row_begin, row_end, nullptr, bounce, 0, 0,
                        device_out, stream);
}

int rt_light_hits_mirrored_accel_device(rt_ctx* ctx, const rt_hit* device_hits,
                                        const rt_scene* device_scene,
                                        const rt_cube_bound* device_accel, const float ray_dir[4],
                                        int32_t width, int32_t row_begin, int32_t row_end,
                                        const float* device_reflectivity, int32_t max_bounces,
                                        int32_t shadows, int32_t out_format, void* device_out,
                                        void* stream) {
    if (max_bounces < 0 || max_bounces > RT_MAX_BOUNCES || (shadows != 0 && shadows != 1))
        return RT_ERR_INVALID_ARG;
    // (the counts are checked by the launch; a scene it refuses is never read)
    if (!device_reflectivity && max_bounces > 0 && device_scene &&
        (int64_t)device_scene->num_cubes + device_scene->num_spheres > 0)
        return RT_ERR_INVALID_ARG;
    // without an array no slot can be read: the kernel then runs at depth 0
    const int32_t depth = device_reflectivity ? max_bounces : 0;
    const size_t shared = 256 * sizeof(float4) * (size_t)depth;
    if (out_format == RT_FORMAT_I32X4)
        return launch_accel(light_accel_kernel<kOutI32x4>, 16, ctx, device_hits,
                            device_scene, device_accel, ray_dir, width, row_begin, row_end,
                            device_reflectivity, depth, shadows, shared, device_out, stream);
    if (out_format == RT_FORMAT_RGBA8)
        return launch_accel(light_accel_kernel<kOutRgba8>, 4, ctx, device_hits,
                            device_scene, device_accel, ray_dir, width, row_begin, row_end,
                            device_reflectivity, depth, shadows, shared, device_out, stream);
    return RT_ERR_INVALID_ARG;
}

}  // extern "C"
