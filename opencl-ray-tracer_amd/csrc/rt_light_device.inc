// rt_light_device.inc -- what the kernels of the deferred light pass share
// (DESIGN.md §3.1a-d): the pixel prologue, the wave-uniform surface step, the
// shadow walk, the bounce walk, the lit store, and on the host the one launch
// function of every entry point over a hit frame, culled ones included, and
// the preload helper.  Included once by every translation unit of
// the light pass and of the ray queries, in front of its kernels; not a
// standalone translation unit.
//
// Each walk is written once, over a cull policy passed by value: whether a
// lane has to test a cube.  The policies are the host walks': KeepAll of
// rt_light_impl.h, the unculled one and the default, and CubeCull of
// rt_accel_impl.h, which asks the prebuilt cube records (DESIGN.md §3.1g,
// §3.1h); WaveGroupCull of rt_sphere_groups.hip adds the shadow walk's loop
// over the sphere groups (§3.1j; a policy with kGroups walks the spheres
// itself).  A translation unit that culls includes rt_accel_impl.h itself,
// behind this file (some set RT_ACCEL_NORMALS_LOOP first).
//
// The per-pixel arithmetic is include/rt_light_impl.h, the text the host
// functions of rt_light.cpp compile, so the two agree bit for bit.  What is
// here is how a wave goes through it: every walk's loops are wave-uniform
// (cube, triangle, sphere and light are indexed by loop counters alone, so
// vertices, centres, radii and lights come through scalar loads, once per
// wave), a lane's own object is only compared there, and a ballot skips what
// no lane of the wave needs.
//
// rt_trace.inc is not included: its shade / (int) helpers are restated in
// rt_light_impl.h, and including it would instantiate every trace kernel a
// second time.
//
// Build: -ffp-contract=off, IEEE '/' and sqrtf (the Makefile's HIPFLAGS).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <type_traits>

#define RT_LIGHT_FN __host__ __device__ inline
#include "rt_hip.h"
#include "rt_internal.h"
#include "rt_light_impl.h"

#pragma clang fp contract(off)  // (file scope: holds for the including file too)

namespace {

using rt_light::KeepAll;

// The two lit outputs of every kernel template; each file's third kind
// (surface, mask, bounce, mask2) is 2 under its own name.
enum { kOutI32x4 = 0, kOutRgba8 = 1 };

// One pixel per thread in 256-thread workgroups (launch() below).
__device__ __forceinline__ int64_t pixel_index() {
    return (int64_t)blockIdx.x * 256 + threadIdx.x;
}

// The prologue of every kernel: n = rows * width pixels; pixel i < n is
// (ox, oy) = (i % width, row_begin + i / width).  One 8-byte load of the
// pixel's rt_hit gives its t, which is returned, and its object id `obj`,
// which is range-checked here.  (ox, oy and obj through references, t as the
// result: the wording that leaves every kernel's instruction stream as it
// was with this text inline, profiles/light_shared/.)
__device__ __forceinline__ float load_pixel(const rt_hit* __restrict__ hits, int64_t i, int64_t n,
                                            int32_t width, int32_t row_begin, const rt_scene& s,
                                            float& ox, float& oy, int32_t& obj) {
    int32_t x, r;
    if (n <= (int64_t)UINT32_MAX) {  // (uniform) the 32-bit division is several times cheaper
        const uint32_t q = (uint32_t)i / (uint32_t)width;
        r = (int32_t)q;
        x = (int32_t)((uint32_t)i - q * (uint32_t)width);
    } else {
        const int64_t q = i / width;
        r = (int32_t)q;
        x = (int32_t)(i - q * width);
    }
    ox = (float)x, oy = (float)(row_begin + r);  // exact: both <= 2^24
    const int2 h = reinterpret_cast<const int2*>(hits)[i];
    const float t = __int_as_float(h.x);
    obj = h.y;
    // the range check in front of every index and comparison: a foreign id is no object
    if (obj < -1 || (int64_t)obj >= (int64_t)s.num_cubes + s.num_spheres) obj = -1;
    return t;
}

// The surface step of a lane that holds a hit pixel: its faced normal at the
// hit point p.  Neighbouring pixels mostly share their cube: where all cube
// lanes of the wave hold one cube, its vertices come through a wave-uniform
// pointer (scalar loads, once for the wave) and not as 64 equal gathers per
// vertex.  This and the lane's own colour slot are all a lane indexes by a
// per-lane value outside its own hit pixel.  (light_kernel has its own form.)
__device__ __forceinline__ rt_light::Vec3 surface_step(const rt_scene& s, int32_t obj, float ox,
                                                       float oy, rt_light::Vec3 d, float t,
                                                       rt_light::Vec3 p) {
    const float* verts = rt_light::cube_verts(s, obj);
    if (verts) {
        const int c0 = __builtin_amdgcn_readfirstlane(obj);
        if (__ballot(obj != c0) == 0) verts = s.cube_vertices + 144 * (int64_t)c0;
    }
    const rt_surface sf = rt_light::surface(s, obj, verts, ox, oy, d, t, p);
    return rt_light::Vec3{sf.nx, sf.ny, sf.nz};
}

// The shadow walk of one light: over every object but `own` (a colour slot of
// `s`, or -1; compared, never an index) from `p` towards p + L, for the lanes
// that are `pending`.  Returns whether the lane is still pending: not
// occluded.  "Any occluder" does not depend on the order of the tests
// (§3.1b), so the walk ends as soon as no lane of the wave is pending.
template <typename Cull = KeepAll>
__device__ __forceinline__ bool occluder_walk(const rt_scene& s, const double* pd,
                                              rt_light::Vec3 p, rt_light::Vec3 L, int32_t own,
                                              bool pending, Cull cull = Cull{}) {
    if (__ballot(pending) == 0) return pending;  // (uniform) no walk for this light
    const double Ld[3] = {L.x, L.y, L.z};
    for (int32_t j = 0; j < s.num_cubes; ++j) {
        // the lane's own cube and a cube its policy drops are skipped whole; a
        // cube no pending lane has to test is skipped by the wave
        const bool mine = pending && own != j && cull.cube(pd, Ld, j, true);
        if (__ballot(mine) == 0) continue;
        const float* v = s.cube_vertices + 144 * (int64_t)j;
        for (int tri = 0; tri < 12; ++tri) {
            if (mine && pending && rt_light::occluded_by_tri(pd, Ld, v + 12 * tri))
                pending = false;
            if (__ballot(mine && pending) == 0) break;
        }
        if (__ballot(pending) == 0) break;
    }
    if (__ballot(pending) != 0) {
        if constexpr (Cull::kGroups) {
            pending = cull.occluder_spheres(s, pd, Ld, p, L, own, pending);
        } else {
            // (sphere sp is object num_cubes + sp; own < 2^31 so the sum fits)
            for (int32_t sp = 0; sp < s.num_spheres; ++sp) {
                if (pending && own - s.num_cubes != sp &&
                    rt_light::occluded_by_sphere(p, L, s.sphere_origins + 4 * (int64_t)sp,
                                                 s.sphere_radius[sp]))
                    pending = false;
                if (__ballot(pending) == 0) break;
            }
        }
    }
    return pending;
}

// shadowed_factor (and, with kMask, shadow_mask into `mask`) at the point `p`
// with the faced normal `nrm` and own object `own`, for the lanes that are
// `active`; 1 for the others.  s.num_lights > 0.
template <bool kMask, typename Cull = KeepAll>
__device__ __forceinline__ float light_walk(const rt_scene& s, rt_light::Vec3 p,
                                            rt_light::Vec3 nrm, int32_t own, bool active,
                                            uint32_t& mask, Cull cull = Cull{}) {
    using rt_light::Vec3;
    float k = 0.0f;
    const double pd[3] = {p.x, p.y, p.z};
    for (int32_t li = 0; li < s.num_lights; ++li) {
        const float* l = s.lights + 4 * (int64_t)li;
        const Vec3 L{l[0] - p.x, l[1] - p.y, l[2] - p.z};
        const float ll = sqrtf((L.x * L.x + L.y * L.y) + L.z * L.z);
        const float c = ((nrm.x * L.x + nrm.y * L.y) + nrm.z * L.z) / ll;
        const bool faces = active && c > 0.0f;
        const bool pending = occluder_walk(s, pd, p, L, own, faces, cull);
        if (faces) {
            if (pending)
                k = k + c;  // not occluded
            else if (kMask)
                mask |= 1u << (li & 31);  // (li < 32: the launch refuses more lights)
        }
    }
    if (k > 1.0f) k = 1.0f;
    return active ? k : 1.0f;
}

// The bounce walk (rt_light::bounce_walk, for a wave): the closest hit from
// `p` along `R` over every object but `own`, for the lanes that cast one;
// (kFar, -1, -1) for the others.  Unlike the shadow walk this one cannot stop
// early: the closest hit needs every candidate.  obj2 / tri2 are -1 or values
// the loop counters held, so they index the scene in range by construction.
// reflect_kernel's walk; phase 2 of shadow_reflect_kernel keeps the same text
// inline (measured: profiles/light_shared/README.md).
template <typename Cull = KeepAll>
__device__ __forceinline__ rt_light::Bounce wave_bounce_walk(const rt_scene& s, rt_light::Vec3 p,
                                                             rt_light::Vec3 R, int32_t own,
                                                             bool casts, Cull cull = Cull{}) {
    rt_light::Bounce b{rt_light::kFar, -1, -1};
    const double pd[3] = {p.x, p.y, p.z};
    const double Rd[3] = {R.x, R.y, R.z};
    float sf;
    for (int32_t j = 0; j < s.num_cubes; ++j) {
        // the lane's own cube and a cube its policy drops are skipped whole; a
        // cube no lane has to test is skipped by the wave
        const bool mine = casts && own != j && cull.cube(pd, Rd, j, false);
        if (__ballot(mine) == 0) continue;
        const float* v = s.cube_vertices + 144 * (int64_t)j;
        for (int tri = 0; tri < 12; ++tri)
            if (mine && rt_light::bounce_tri(pd, Rd, v + 12 * tri, &sf) && sf < b.best)
                b = rt_light::Bounce{sf, j, tri};
    }
    // (sphere sp is object num_cubes + sp; own < 2^31 so the sum fits)
    for (int32_t sp = 0; sp < s.num_spheres; ++sp)
        if (casts && own - s.num_cubes != sp &&
            rt_light::bounce_sphere(p, R, s.sphere_origins + 4 * (int64_t)sp, s.sphere_radius[sp],
                                    &sf) &&
            sf < b.best)
            b = rt_light::Bounce{sf, s.num_cubes + sp, -1};
    return b;
}

// The lit store: pixel i of an int32x4 (16 bytes) or RGBA8 (4 bytes) frame.
template <int kOut>
__device__ __forceinline__ void store_lit(void* __restrict__ out, int64_t i, const int32_t px[4]) {
    static_assert(kOut == kOutI32x4 || kOut == kOutRgba8, "a lit output");
    if constexpr (kOut == kOutI32x4)
        reinterpret_cast<int4*>(out)[i] = make_int4(px[0], px[1], px[2], px[3]);
    else
        reinterpret_cast<uint32_t*>(out)[i] = rt_light::pack_rgba8(px);
}

// What launch() refuses of a kernel's own arguments: a reflectivity outside
// [0, 1] (NaN too), a misaligned reflectivity array.
inline bool refused(float refl) { return !(refl >= 0.0f && refl <= 1.0f); }
inline bool refused(const float* refl) { return reinterpret_cast<uintptr_t>(refl) % sizeof(float); }
inline bool refused(int32_t) { return false; }

// The launch of every entry point of a hit frame.  `cull`: KeepAll, for a
// kernel that takes `out` second, or CubeCull{accel}, for one that takes the
// records there and `out` last; `shared`: bytes of dynamic shared memory;
// `align`: of `out`, in bytes; `mask`: the output holds one bit per light, so
// at most 32; `own`: the kernel's own arguments between the ray direction and
// the scene: nothing, one reflectivity, or the chain's array, depth and
// shadows.  Every check runs before any HIP call.
template <typename Cull, typename Kernel, typename... Own>
int launch(Cull cull, size_t shared, Kernel kernel, uintptr_t align, bool mask, rt_ctx* ctx,
           const rt_hit* hits, const rt_scene* scene, const float* ray_dir, int32_t width,
           int32_t row_begin, int32_t row_end, void* out, void* stream, Own... own) {
    constexpr bool kCulled = !std::is_same_v<Cull, KeepAll>;
    if (!ctx || rt_light::check(hits, scene, ray_dir, width, row_begin, row_end, out) ||
        reinterpret_cast<uintptr_t>(hits) % sizeof(rt_hit) ||
        reinterpret_cast<uintptr_t>(out) % align)
        return RT_ERR_INVALID_ARG;
    if ((refused(own) || ...)) return RT_ERR_INVALID_ARG;
    if (mask && scene->num_lights > 32) return RT_ERR_UNSUPPORTED;
    const int64_t n = (int64_t)(row_end - row_begin) * width;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > INT32_MAX) return RT_ERR_UNSUPPORTED;
    if (check_cull(scene, cull)) return RT_ERR_INVALID_ARG;
    if (hipSetDevice(rt_internal::ctx_device(ctx)) != hipSuccess) return RT_ERR_HIP;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : rt_internal::ctx_stream(ctx);
    if (!st) return RT_ERR_HIP;
    const auto enqueue = [&](auto second, auto... last) {
        kernel<<<dim3((unsigned)blocks), dim3(256), shared, st>>>(
            hits, second, n, width, row_begin, ray_dir[0], ray_dir[1], ray_dir[2], own..., *scene,
            last...);
    };
    if constexpr (kCulled)
        enqueue(cull.accel, out);
    else
        enqueue(out);
    return hipGetLastError() == hipSuccess ? RT_OK : RT_ERR_HIP;
}

// The lit entry points: the int32x4 or the RGBA8 instance by `out_format`.
template <typename Cull, typename Kernel, typename... Own>
int launch_lit(Cull cull, size_t shared, Kernel i32x4, Kernel rgba8, int32_t out_format,
               rt_ctx* ctx, const rt_hit* hits, const rt_scene* scene, const float* ray_dir,
               int32_t width, int32_t row_begin, int32_t row_end, void* out, void* stream,
               Own... own) {
    if (out_format == RT_FORMAT_I32X4)
        return launch(cull, shared, i32x4, 16, false, ctx, hits, scene, ray_dir, width, row_begin,
                      row_end, out, stream, own...);
    if (out_format == RT_FORMAT_RGBA8)
        return launch(cull, shared, rgba8, 4, false, ctx, hits, scene, ray_dir, width, row_begin,
                      row_end, out, stream, own...);
    return RT_ERR_INVALID_ARG;
}

// rt_init: load the including translation unit's code object now
inline int preload(std::initializer_list<const void*> kernels) {
    hipFuncAttributes a;
    for (const void* k : kernels)
        if (hipFuncGetAttributes(&a, k) != hipSuccess) return RT_ERR_HIP;
    return RT_OK;
}

}  // namespace
