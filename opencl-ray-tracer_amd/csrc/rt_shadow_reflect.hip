// rt_shadow_reflect.hip -- rt_shadow_hits_reflected_device /
// rt_light_hits_shadowed_reflected_device: the deferred light pass with all of
// its terms, on the device: shadowed direct light at the hit
// point p, the mirror bounce, shadowed direct light at the point p2 the bounce
// meets, blended.
//
// One kernel template over the output (mask at p2, int32x4, RGBA8), one pixel
// per thread in 256-thread workgroups, shadow_kernel's index arithmetic: an
// 8-byte load of the pixel's rt_hit, the surface step of rt_light.hip, then
// three phases with the tests of include/rt_light_impl.h (the text the host
// functions of rt_light.cpp compile, so the two agree bit for bit), one 4- or
// 16-byte store.  No workspace, one launch.
//
// Every phase sits behind a wave-uniform guard; a wave that has nothing to do
// in a phase never enters it:
//   1. the shadow walk at p (lit instances with lights): shadow_kernel's walk,
//      per light a pending set (lanes that cast, c > 0, not yet occluded), the
//      lane's own cube skipped whole, a ballot that ends the light's walk;
//   2. the bounce walk (the mask instance, or reflectivity != 0):
//      reflect_kernel's walk, no early exit, the closest hit needs every
//      candidate;
//   3. the shadow walk at p2 (lights, and a lane of the wave whose bounce met
//      something): n2 and p2 are gathered by obj2 / tri2 first, then the walk
//      of phase 1 runs with own object obj2 over the lanes whose bounce met
//      something.
// Phases 1 and 3 are one text: light_walk() over the lights, occluder_walk()
// over the occluders of one light.
//
// Inside every walk cube, triangle, sphere and light are indexed by loop
// counters alone, so vertices, centres, radii and lights come through scalar
// loads, once per wave; obj and obj2 are only compared there.  Before the
// walks no lane indexes anything by a per-lane value but its own hit pixel and
// its own cube's vertices or sphere's centre (the surface step).  Between
// phases 2 and 3, and in the shade, a lane reads the bounce's triangle or
// centre and its colour by obj2 / tri2: values the kernel took from its own
// loop counters, in range by construction.
//
// rt_init does not load this translation unit's code object: the runtime
// loads it at the first launch of one of its kernels.
//
// Build: -ffp-contract=off, IEEE '/' and sqrtf (the Makefile's HIPFLAGS).
#include <hip/hip_runtime.h>

#include <cstdint>

#define RT_LIGHT_FN __host__ __device__ inline
#include "rt_hip.h"
#include "rt_internal.h"
#include "rt_light_impl.h"

#pragma clang fp contract(off)

namespace {

enum { kOutI32x4 = 0, kOutRgba8 = 1, kOutMask2 = 2 };

// One light's walk over every object but `own` (a colour slot of `s`, or -1;
// compared, never an index) from `p` towards p + L, for the lanes that are
// `pending`.  Returns whether the lane is still pending: not occluded.  "Any
// occluder" does not depend on the order of the tests (§3.1b), so the walk
// ends as soon as no lane of the wave is pending.
__device__ __forceinline__ bool occluder_walk(const rt_scene& s, const double* pd,
                                              rt_light::Vec3 p, rt_light::Vec3 L, int32_t own,
                                              bool pending) {
    if (__ballot(pending) == 0) return pending;  // (uniform) no walk for this light
    const double Ld[3] = {L.x, L.y, L.z};
    for (int32_t j = 0; j < s.num_cubes; ++j) {
        // the lane's own cube is skipped whole; a cube no pending lane has to
        // test is skipped by the wave
        const bool mine = pending && own != j;
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
        // (sphere sp is object num_cubes + sp; own < 2^31 so the sum fits)
        for (int32_t sp = 0; sp < s.num_spheres; ++sp) {
            if (pending && own - s.num_cubes != sp &&
                rt_light::occluded_by_sphere(p, L, s.sphere_origins + 4 * (int64_t)sp,
                                             s.sphere_radius[sp]))
                pending = false;
            if (__ballot(pending) == 0) break;
        }
    }
    return pending;
}

// shadowed_factor (and, with kMask, shadow_mask into `mask`) at the point `p`
// with the faced normal `nrm` and own object `own`, for the lanes that are
// `active`; 1 for the others.  s.num_lights > 0.
template <bool kMask>
__device__ __forceinline__ float light_walk(const rt_scene& s, rt_light::Vec3 p,
                                            rt_light::Vec3 nrm, int32_t own, bool active,
                                            uint32_t& mask) {
    using rt_light::Vec3;
    float k = 0.0f;
    const double pd[3] = {p.x, p.y, p.z};
    for (int32_t li = 0; li < s.num_lights; ++li) {
        const float* l = s.lights + 4 * (int64_t)li;
        const Vec3 L{l[0] - p.x, l[1] - p.y, l[2] - p.z};
        const float ll = sqrtf((L.x * L.x + L.y * L.y) + L.z * L.z);
        const float c = ((nrm.x * L.x + nrm.y * L.y) + nrm.z * L.z) / ll;
        const bool faces = active && c > 0.0f;
        const bool pending = occluder_walk(s, pd, p, L, own, faces);
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

// `s` holds device pointers.  n = rows * width pixels; pixel i is
// (i % width, row_begin + i / width).  `refl`: the lit forms' reflectivity.
template <int kOut>
__global__ void __launch_bounds__(256)
shadow_reflect_kernel(const rt_hit* __restrict__ hits, void* __restrict__ out, int64_t n,
                      int32_t width, int32_t row_begin, float dx, float dy, float dz, float refl,
                      rt_scene s) {
    using rt_light::Vec3;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
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
    const float ox = (float)x, oy = (float)(row_begin + r);  // exact: both <= 2^24
    const Vec3 d{dx, dy, dz};
    const int2 h = reinterpret_cast<const int2*>(hits)[i];
    const float t = __int_as_float(h.x);
    int32_t obj = h.y;
    // the range check in front of every index and comparison: a foreign id is no object
    if (obj < -1 || (int64_t)obj >= (int64_t)s.num_cubes + s.num_spheres) obj = -1;
    const bool hit = obj >= 0;
    constexpr bool kMask = kOut == kOutMask2;
    // the lanes that take part: the lit forms leave t == kFar to shade_lit,
    // which writes black whatever the factor
    const bool casts = kMask ? hit : hit && !(t == rt_light::kFar);
    const bool lights = s.num_lights > 0;             // (uniform)
    const bool mirrors = kMask || refl != 0.0f;       // (uniform) a kernel argument
    const bool work = kMask ? lights : (mirrors || lights);  // (uniform) the mask is 0 without lights

    float k = 1.0f, k2 = 1.0f;
    uint32_t mask = 0, unused = 0;
    rt_light::Bounce b{rt_light::kFar, -1, -1};
    if (work && __ballot(casts) != 0) {  // (uniform)
        Vec3 p{0.0f, 0.0f, 0.0f}, nrm{0.0f, 0.0f, 0.0f};
        if (casts) {
            p = rt_light::hit_point(ox, oy, d, t);
            // the surface step of light_kernel: a wave-uniform pointer where
            // all cube lanes of the wave hold one cube
            const float* verts = rt_light::cube_verts(s, obj);
            if (verts) {
                const int c0 = __builtin_amdgcn_readfirstlane(obj);
                if (__ballot(obj != c0) == 0) verts = s.cube_vertices + 144 * (int64_t)c0;
            }
            const rt_surface sf = rt_light::surface(s, obj, verts, ox, oy, d, t, p);
            nrm = Vec3{sf.nx, sf.ny, sf.nz};
        }
        // phase 1: the shadowed factor at p
        if (!kMask && lights) k = light_walk<false>(s, p, nrm, obj, casts, unused);  // (uniform)
        if (mirrors) {  // (uniform)
            // phase 2: the bounce walk
            const Vec3 R = rt_light::mirror_dir(nrm, d);
            const double pd[3] = {p.x, p.y, p.z};
            const double Rd[3] = {R.x, R.y, R.z};
            float sf;
            for (int32_t j = 0; j < s.num_cubes; ++j) {
                // the lane's own cube is skipped whole; a cube no lane has to
                // test is skipped by the wave
                const bool mine = casts && obj != j;
                if (__ballot(mine) == 0) continue;
                const float* v = s.cube_vertices + 144 * (int64_t)j;
                for (int tri = 0; tri < 12; ++tri)
                    if (mine && rt_light::bounce_tri(pd, Rd, v + 12 * tri, &sf) && sf < b.best)
                        b = rt_light::Bounce{sf, j, tri};
            }
            // (sphere sp is object num_cubes + sp; obj < 2^31 so the sum fits)
            for (int32_t sp = 0; sp < s.num_spheres; ++sp)
                if (casts && obj - s.num_cubes != sp &&
                    rt_light::bounce_sphere(p, R, s.sphere_origins + 4 * (int64_t)sp,
                                            s.sphere_radius[sp], &sf) &&
                    sf < b.best)
                    b = rt_light::Bounce{sf, s.num_cubes + sp, -1};
            // phase 3: the shadowed factor (the mask) at p2
            const bool met = b.obj2 >= 0;
            if (lights && __ballot(met) != 0) {  // (uniform)
                Vec3 p2{0.0f, 0.0f, 0.0f}, n2{0.0f, 0.0f, 0.0f};
                if (met) {
                    // b.obj2 / b.tri2 index the scene here: values the loop
                    // counters above held (j < num_cubes, tri < 12, num_cubes
                    // + sp with sp < num_spheres), in range by construction
                    p2 = rt_light::bounce_point(p, R, b.best);
                    n2 = rt_light::bounce_normal(s, b.obj2, b.tri2, p2, R);
                }
                k2 = light_walk<kMask>(s, p2, n2, b.obj2, met, mask);
            }
        }
    }
    if constexpr (kMask) {
        reinterpret_cast<uint32_t*>(out)[i] = mask;
    } else {
        int32_t px[4];
        if (mirrors && casts)
            // (b.obj2 indexes the colours: -1 or in range, as above)
            rt_light::shade_mirrored_factors(s, obj, t, k, b, k2, refl, px);
        else
            rt_light::shade_lit(t, k, rt_light::slot_colour(s, obj), px);
        if constexpr (kOut == kOutI32x4)
            reinterpret_cast<int4*>(out)[i] = make_int4(px[0], px[1], px[2], px[3]);
        else
            reinterpret_cast<uint32_t*>(out)[i] = rt_light::pack_rgba8(px);
    }
}

template <int kOut>
int launch(rt_ctx* ctx, const rt_hit* hits, const rt_scene* scene, const float* ray_dir,
           int32_t width, int32_t row_begin, int32_t row_end, float refl, void* out,
           void* stream) {
    constexpr uintptr_t kAlign = kOut == kOutI32x4 ? 16 : 4;
    if (!ctx || rt_light::check(hits, scene, ray_dir, width, row_begin, row_end, out) ||
        reinterpret_cast<uintptr_t>(hits) % sizeof(rt_hit) ||
        reinterpret_cast<uintptr_t>(out) % kAlign)
        return RT_ERR_INVALID_ARG;
    if (!(refl >= 0.0f && refl <= 1.0f)) return RT_ERR_INVALID_ARG;  // NaN too
    if (kOut == kOutMask2 && scene->num_lights > 32) return RT_ERR_UNSUPPORTED;
    const int64_t n = (int64_t)(row_end - row_begin) * width;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > INT32_MAX) return RT_ERR_UNSUPPORTED;
    if (hipSetDevice(rt_internal::ctx_device(ctx)) != hipSuccess) return RT_ERR_HIP;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : rt_internal::ctx_stream(ctx);
    if (!st) return RT_ERR_HIP;
    shadow_reflect_kernel<kOut><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(
        hits, out, n, width, row_begin, ray_dir[0], ray_dir[1], ray_dir[2], refl, *scene);
    return hipGetLastError() == hipSuccess ? RT_OK : RT_ERR_HIP;
}

}  // namespace

extern "C" {

int rt_shadow_hits_reflected_device(rt_ctx* ctx, const rt_hit* device_hits,
                                    const rt_scene* device_scene, const float ray_dir[4],
                                    int32_t width, int32_t row_begin, int32_t row_end,
                                    uint32_t* device_out, void* stream) {
    return launch<kOutMask2>(ctx, device_hits, device_scene, ray_dir, width, row_begin, row_end,
                             0.0f, device_out, stream);
}

int rt_light_hits_shadowed_reflected_device(rt_ctx* ctx, const rt_hit* device_hits,
                                            const rt_scene* device_scene, const float ray_dir[4],
                                            int32_t width, int32_t row_begin, int32_t row_end,
                                            float reflectivity, int32_t out_format,
                                            void* device_out, void* stream) {
    if (out_format == RT_FORMAT_I32X4)
        return launch<kOutI32x4>(ctx, device_hits, device_scene, ray_dir, width, row_begin,
                                 row_end, reflectivity, device_out, stream);
    if (out_format == RT_FORMAT_RGBA8)
        return launch<kOutRgba8>(ctx, device_hits, device_scene, ray_dir, width, row_begin,
                                 row_end, reflectivity, device_out, stream);
    return RT_ERR_INVALID_ARG;
}

}  // extern "C"
