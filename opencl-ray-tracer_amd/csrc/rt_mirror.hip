// rt_mirror.hip -- rt_bounce_hits_device / rt_light_hits_mirrored_device: the
// mirror chain of the deferred light pass, on the device:
// the bounce of rt_reflect.hip taken again from the point it meets, up to
// RT_MAX_BOUNCES times, with one reflectivity per colour slot and, on request,
// the shadow term at every level.
//
// One kernel template over the output (bounce frame, int32x4, RGBA8): the
// pixel prologue, the surface step, the level loop, the unwind, one 8-, 16- or
// 4-byte store.  No workspace, one launch.
//
// The level loop is a loop: one copy of the shadow walk and one of the bounce
// walk, whatever the depth.  Its trip count is wave-uniform: a level is
// entered while a lane of the wave is still on its chain, and a ballot ends
// it, so a wave whose chains all end after level 1 pays one bounce walk.  At
// a level, the lanes that reached it take their direct light (light_walk with
// `shadows`, light_factor without; neither without lights), then the lanes
// whose chain goes on push (a_j, r_j) and walk.  Every walk index is a loop
// counter; a lane indexes per lane only its own pixel, reflectivity[obj_j],
// colour slot obj_j and the triangle or centre of (obj_j, tri_j): values the
// range check passed or loop counters held.
//
// The backward blend needs (a_j, r_j) of every level the chain went on from.
// A register array indexed by the level would go to scratch, so the stack is
// LDS: one float4 per lane and level, lane-contiguous (level l of thread x at
// [256 * l + x]), max_bounces * 4 KiB of dynamic shared memory.  A lane reads
// only what it wrote itself, so there is no barrier.  The unwind is a
// wave-uniform loop from the wave's deepest level down.
//
// rt_init does not load this translation unit's code object: the runtime
// loads it at the first launch of one of its kernels.
#include "rt_light_device.inc"

namespace {

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

// `s` holds device pointers.  `depth`: max_bounces of the lit forms (0 ..
// RT_MAX_BOUNCES; the launch passes depth * 4 KiB of shared memory), the
// bounce's number of the bounce form (1 .. RT_MAX_BOUNCES).  `refl`: the lit
// forms' reflectivity by colour slot.  (uniform: depth, shadows)
template <int kOut>
__global__ void __launch_bounds__(256)
mirror_kernel(const rt_hit* __restrict__ hits, void* __restrict__ out, int64_t n, int32_t width,
              int32_t row_begin, float dx, float dy, float dz, const float* __restrict__ refl,
              int32_t depth, int32_t shadows, rt_scene s) {
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
            b = wave_bounce_walk(s, p, R, cur, live);  // (kFar, -1) for the others
            if (j >= depth) break;                     // (uniform)
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
                        k = light_walk<false>(s, p, nrm, cur, live, unused);
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
                const rt_light::Bounce b = wave_bounce_walk(s, p, R, cur, goes);
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

// The launch of both entry points: launch() of rt_light_device.inc with the
// chain's arguments and its shared memory.  `align`: of `out`, in bytes.
template <typename Kernel>
int launch_mirror(Kernel kernel, uintptr_t align, rt_ctx* ctx, const rt_hit* hits,
                  const rt_scene* scene, const float* ray_dir, int32_t width, int32_t row_begin,
                  int32_t row_end, const float* refl, int32_t depth, int32_t shadows,
                  size_t shared, void* out, void* stream) {
    if (!ctx || rt_light::check(hits, scene, ray_dir, width, row_begin, row_end, out) ||
        reinterpret_cast<uintptr_t>(hits) % sizeof(rt_hit) ||
        reinterpret_cast<uintptr_t>(out) % align ||
        reinterpret_cast<uintptr_t>(refl) % sizeof(float))
        return RT_ERR_INVALID_ARG;
    const int64_t n = (int64_t)(row_end - row_begin) * width;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > INT32_MAX) return RT_ERR_UNSUPPORTED;
    if (hipSetDevice(rt_internal::ctx_device(ctx)) != hipSuccess) return RT_ERR_HIP;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : rt_internal::ctx_stream(ctx);
    if (!st) return RT_ERR_HIP;
    kernel<<<dim3((unsigned)blocks), dim3(256), shared, st>>>(
        hits, out, n, width, row_begin, ray_dir[0], ray_dir[1], ray_dir[2], refl, depth, shadows,
        *scene);
    return hipGetLastError() == hipSuccess ? RT_OK : RT_ERR_HIP;
}

}  // namespace

extern "C" {

int rt_bounce_hits_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                          const float ray_dir[4], int32_t width, int32_t row_begin,
                          int32_t row_end, int32_t bounce, rt_hit* device_out, void* stream) {
    if (bounce < 1 || bounce > RT_MAX_BOUNCES) return RT_ERR_INVALID_ARG;
    return launch_mirror(mirror_kernel<kOutBounce>, 8, ctx, device_hits, device_scene, ray_dir,
                         width, row_begin, row_end, nullptr, bounce, 0, 0, device_out, stream);
}

int rt_light_hits_mirrored_device(rt_ctx* ctx, const rt_hit* device_hits,
                                  const rt_scene* device_scene, const float ray_dir[4],
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
        return launch_mirror(mirror_kernel<kOutI32x4>, 16, ctx, device_hits, device_scene, ray_dir,
                             width, row_begin, row_end, device_reflectivity, depth, shadows,
                             shared, device_out, stream);
    if (out_format == RT_FORMAT_RGBA8)
        return launch_mirror(mirror_kernel<kOutRgba8>, 4, ctx, device_hits, device_scene, ray_dir,
                             width, row_begin, row_end, device_reflectivity, depth, shadows,
                             shared, device_out, stream);
    return RT_ERR_INVALID_ARG;
}

}  // extern "C"
