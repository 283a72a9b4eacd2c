// rt_chain_device.inc -- the mirror chain of a hit frame on the device
// (DESIGN.md §3.1e, §3.1h), written once: one kernel template over the output
// (bounce frame, int32x4, RGBA8) and over what the walks cull by (nothing, or
// the prebuilt cube records through CubeCull of rt_accel_impl.h), which
// rt_mirror.hip and rt_light_accel.hip instantiate; and what the camera view's
// kernel (rt_camera_light.hip, §3.1i) shares with it.  Included behind
// rt_light_device.inc (and, where the file culls, behind rt_accel_impl.h); not
// a standalone translation unit.  The level an accepted bounce reaches is
// next_level of rt_light_impl.h, the host's too.
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

namespace {

enum { kOutBounce = 2 };

// The int32x4 pixel of a chain's colour.
__device__ __forceinline__ void chain_lit(rt_light::Vec3 C, int32_t lit[4]) {
    lit[0] = rt_light::cvt_i32(C.x);
    lit[1] = rt_light::cvt_i32(C.y);
    lit[2] = rt_light::cvt_i32(C.z);
    lit[3] = 255;
}

// The policy and the output of hit_chain_kernel's (second, last...).
__device__ __forceinline__ KeepAll chain_cull(void*) { return KeepAll{}; }
__device__ __forceinline__ void* chain_out(void* out) { return out; }
template <typename Accel>
__device__ __forceinline__ auto chain_cull(Accel accel, void*) {
    return rt_light::cull_of(accel);
}
template <typename Accel>
__device__ __forceinline__ void* chain_out(Accel, void* out) {
    return out;
}

// The chain of one pixel of a hit frame: mirror_kernel (rt_mirror.hip) and
// light_accel_kernel (rt_light_accel.hip) are this kernel.  `s` holds device
// pointers.  `depth`: max_bounces of the lit forms (0 .. RT_MAX_BOUNCES; the
// launch passes depth * 4 KiB of shared memory), the bounce's number of the
// bounce form (1 .. RT_MAX_BOUNCES).  `refl`: the lit forms' reflectivity by
// colour slot.  (uniform: depth, shadows)
//
// The two differ in two arguments, which stay where they were, so that the
// same dwords arrive preloaded: the unculled kernel takes `out` second and
// nothing last; the culled one takes the s.num_cubes records second and `out`,
// which is read once at the end, last (rt_light_accel.hip).  (One kernel text
// and not a function both kernels call: with that, the compiler orders two
// instructions of the push differently, profiles/chain_shared/.)
template <int kOut, typename Second, typename... Last>
__global__ void __launch_bounds__(256)
hit_chain_kernel(const rt_hit* __restrict__ hits, Second __restrict__ second, int64_t n,
                 int32_t width, int32_t row_begin, float dx, float dy, float dz,
                 const float* __restrict__ refl, int32_t depth, int32_t shadows, rt_scene s,
                 Last __restrict__... last) {
    const auto cull = chain_cull(second, last...);
    void* const out = chain_out(second, last...);
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
            b = wave_bounce_walk(s, p, R, cur, live, cull);  // (kFar, -1) for the others
            if (j >= depth) break;                           // (uniform)
            live = b.obj2 >= 0;
            if (live) rt_light::next_level(s, b, R, p, nrm, D, cur);
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
                const bool goes = live && r != 0.0f;
                if (live && !goes) C = a;        // ended here by depth or by a matte object
                if (__ballot(goes) == 0) break;  // (uniform) at j == depth at the latest
                // j < depth here, so the push stays inside depth * 4 KiB
                if (goes) {
                    mine[256 * pushed] = make_float4(a.x, a.y, a.z, r);
                    ++pushed;
                }
                deepest = j + 1;
                const Vec3 R = rt_light::mirror_dir(nrm, D);
                const rt_light::Bounce b = wave_bounce_walk(s, p, R, cur, goes, cull);
                live = goes && b.obj2 >= 0;  // a miss leaves C = (0, 0, 0)
                if (live) {
                    T = T + b.best;
                    rt_light::next_level(s, b, R, p, nrm, D, cur);
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
        if (chained)
            chain_lit(C, lit);
        else
            rt_light::shade_lit(t, 1.0f, rt_light::slot_colour(s, obj), lit);
        store_lit<kOut>(out, i, lit);
    }
}

// The preamble of the lit chain entry points: the host's check of the settings
// (the counts are checked by the launch; a scene it refuses is never read),
// then the kernel's `depth` and the bytes of its blend stack.
inline int chain_settings(const rt_scene* scene, const float* refl, int32_t max_bounces,
                          int32_t shadows, int32_t out_format, int32_t& depth, size_t& shared) {
    const int rc = rt_light::check_chain_settings(scene, refl, max_bounces, shadows, out_format);
    // without an array no slot can be read: the kernel then runs at depth 0
    depth = refl ? max_bounces : 0;
    shared = 256 * sizeof(float4) * (size_t)depth;
    return rc;
}

}  // namespace
