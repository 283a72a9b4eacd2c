// rt_reflect.hip -- rt_reflect_hits_device / rt_light_hits_reflected_device: the
// mirror bounce of the deferred light pass, on the device.
//
// One kernel template over the output (bounce frame, int32x4, RGBA8), one
// pixel per thread in 256-thread workgroups, shadow_kernel's index arithmetic:
// an 8-byte load of the pixel's rt_hit, the surface step of rt_light.hip, the
// mirrored direction, then one closest-hit walk over every other object of
// the scene with the tests of include/rt_light_impl.h (the text the host
// functions of rt_light.cpp compile, so the two agree bit for bit), one 8-,
// 16- or 4-byte store.  No workspace, one launch.
//
// The walk is what the kernel costs: 12 * cubes + spheres tests per hit pixel,
// each triangle test in fp64.  Its loops are wave-uniform: cube, triangle and
// sphere are indexed by loop counters alone, so vertices, centres and radii
// come through scalar loads, once per wave.  A lane takes part where it holds
// a hit pixel and the cube or sphere is not its own (compared, a whole cube at
// once); a cube no lane has to test is skipped by a ballot.  Unlike the shadow
// walk this one cannot stop early: the closest hit needs every candidate.  A
// wave without a hit lane never enters it, nor does a lit launch with
// reflectivity 0 (a uniform branch on the kernel argument).
//
// Before the walk no lane indexes anything by a per-lane value but its own
// hit pixel, its own colour slot and its own cube's vertices (the surface
// step).  After it the lit forms read the bounce's triangle or centre and its
// colour by obj2 / tri2, which the kernel took from its own loop counters.
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

enum { kOutI32x4 = 0, kOutRgba8 = 1, kOutBounce = 2 };

// `s` holds device pointers.  n = rows * width pixels; pixel i is
// (i % width, row_begin + i / width).  `refl`: the lit forms' reflectivity.
template <int kOut>
__global__ void __launch_bounds__(256)
reflect_kernel(const rt_hit* __restrict__ hits, void* __restrict__ out, int64_t n, int32_t width,
               int32_t row_begin, float dx, float dy, float dz, float refl, rt_scene s) {
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
    // the lanes that cast a bounce: the lit forms leave t == kFar to lit_pixel
    const bool casts = kOut == kOutBounce ? hit : hit && !(t == rt_light::kFar);
    const bool mirrors = kOut == kOutBounce || refl != 0.0f;  // (uniform) a kernel argument

    float k = 1.0f;
    Vec3 p{0.0f, 0.0f, 0.0f}, R{0.0f, 0.0f, 0.0f};
    rt_light::Bounce b{rt_light::kFar, -1, -1};
    if ((mirrors || s.num_lights > 0) && __ballot(hit) != 0) {  // (uniform)
        if (hit) {
            p = rt_light::hit_point(ox, oy, d, t);
            // the surface step of light_kernel: a wave-uniform pointer where
            // all cube lanes of the wave hold one cube
            const float* verts = rt_light::cube_verts(s, obj);
            if (verts) {
                const int c0 = __builtin_amdgcn_readfirstlane(obj);
                if (__ballot(obj != c0) == 0) verts = s.cube_vertices + 144 * (int64_t)c0;
            }
            const rt_surface sf = rt_light::surface(s, obj, verts, ox, oy, d, t, p);
            const Vec3 nrm{sf.nx, sf.ny, sf.nz};
            if (kOut != kOutBounce && s.num_lights > 0)
                k = rt_light::light_factor(nrm, p, s.lights, s.num_lights);
            R = rt_light::mirror_dir(nrm, d);
        }
        if (mirrors && __ballot(casts) != 0) {  // (uniform) the walk
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
        }
    }
    if constexpr (kOut == kOutBounce) {
        reinterpret_cast<int2*>(out)[i] = make_int2(__float_as_int(b.best), b.obj2);
    } else {
        int32_t px[4];
        if (mirrors && casts)
            // b.obj2 / b.tri2 index the scene here: they are -1 or values the
            // loop counters above held (j < num_cubes, tri < 12, num_cubes + sp
            // with sp < num_spheres), so they are in range by construction
            rt_light::shade_mirrored(s, obj, t, k, p, R, b, refl, px);
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
    constexpr uintptr_t kAlign = kOut == kOutI32x4 ? 16 : kOut == kOutBounce ? 8 : 4;
    if (!ctx || rt_light::check(hits, scene, ray_dir, width, row_begin, row_end, out) ||
        reinterpret_cast<uintptr_t>(hits) % sizeof(rt_hit) ||
        reinterpret_cast<uintptr_t>(out) % kAlign)
        return RT_ERR_INVALID_ARG;
    if (!(refl >= 0.0f && refl <= 1.0f)) return RT_ERR_INVALID_ARG;  // NaN too
    const int64_t n = (int64_t)(row_end - row_begin) * width;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > INT32_MAX) return RT_ERR_UNSUPPORTED;
    if (hipSetDevice(rt_internal::ctx_device(ctx)) != hipSuccess) return RT_ERR_HIP;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : rt_internal::ctx_stream(ctx);
    if (!st) return RT_ERR_HIP;
    reflect_kernel<kOut><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(
        hits, out, n, width, row_begin, ray_dir[0], ray_dir[1], ray_dir[2], refl, *scene);
    return hipGetLastError() == hipSuccess ? RT_OK : RT_ERR_HIP;
}

}  // namespace

namespace rt_internal {
// rt_init: load this translation unit's code object now
int preload_reflect_kernels() {
    hipFuncAttributes a;
    for (const void* k : {reinterpret_cast<const void*>(reflect_kernel<kOutI32x4>),
                          reinterpret_cast<const void*>(reflect_kernel<kOutRgba8>),
                          reinterpret_cast<const void*>(reflect_kernel<kOutBounce>)})
        if (hipFuncGetAttributes(&a, k) != hipSuccess) return RT_ERR_HIP;
    return RT_OK;
}
}  // namespace rt_internal

extern "C" {

int rt_reflect_hits_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                           const float ray_dir[4], int32_t width, int32_t row_begin,
                           int32_t row_end, rt_hit* device_out, void* stream) {
    return launch<kOutBounce>(ctx, device_hits, device_scene, ray_dir, width, row_begin, row_end,
                              0.0f, device_out, stream);
}

int rt_light_hits_reflected_device(rt_ctx* ctx, const rt_hit* device_hits,
                                   const rt_scene* device_scene, const float ray_dir[4],
                                   int32_t width, int32_t row_begin, int32_t row_end,
                                   float reflectivity, int32_t out_format, void* device_out,
                                   void* stream) {
    if (out_format == RT_FORMAT_I32X4)
        return launch<kOutI32x4>(ctx, device_hits, device_scene, ray_dir, width, row_begin,
                                 row_end, reflectivity, device_out, stream);
    if (out_format == RT_FORMAT_RGBA8)
        return launch<kOutRgba8>(ctx, device_hits, device_scene, ray_dir, width, row_begin,
                                 row_end, reflectivity, device_out, stream);
    return RT_ERR_INVALID_ARG;
}

}  // extern "C"
