// rt_shadow.hip -- rt_shadow_hits_device / rt_light_hits_shadowed_device: the
// shadow term of the deferred light pass, on the device.
//
// One kernel template over the output (mask, int32x4, RGBA8), one pixel per
// thread in 256-thread workgroups, light_kernel's index arithmetic: an 8-byte
// load of the pixel's rt_hit, the surface step of rt_light.hip, then per
// light that faces the pixel a walk over every other object of the scene
// with the tests of include/rt_light_impl.h (the text the host functions of
// rt_light.cpp compile, so the two agree bit for bit), one 4- or 16-byte
// store.  No workspace, one launch.
//
// The walk is what the kernel costs: lights x (12 * cubes + spheres) tests
// per pixel, each triangle test in fp64.  Its loops are wave-uniform: the
// light and the occluder are indexed by loop counters alone, so vertices,
// centres and radii come through scalar loads, once per wave.  A lane takes
// part only while it is pending (hit pixel, c > 0, not yet occluded for this
// light); its own object is skipped by comparison, a whole cube at once.
// "Any occluder" does not depend on the order of the tests (§3.1b), so a
// ballot ends a light's walk as soon as no lane of the wave is pending, and
// a wave without a hit lane, or a launch without lights, never enters it.
//
// No lane indexes anything by a per-lane value but its own hit pixel, its
// own colour slot and its own cube's vertices (the surface step).
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

enum { kOutI32x4 = 0, kOutRgba8 = 1, kOutMask = 2 };

// `s` holds device pointers.  n = rows * width pixels; pixel i is
// (i % width, row_begin + i / width).
template <int kOut>
__global__ void __launch_bounds__(256)
shadow_kernel(const rt_hit* __restrict__ hits, void* __restrict__ out, int64_t n, int32_t width,
              int32_t row_begin, float dx, float dy, float dz, rt_scene s) {
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

    float k = 1.0f;
    uint32_t mask = 0;
    if (s.num_lights > 0 && __ballot(hit) != 0) {  // (uniform) else: no walk at all
        Vec3 p{0.0f, 0.0f, 0.0f}, nrm{0.0f, 0.0f, 0.0f};
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
            nrm = Vec3{sf.nx, sf.ny, sf.nz};
            k = 0.0f;
        }
        const double pd[3] = {p.x, p.y, p.z};
        for (int32_t li = 0; li < s.num_lights; ++li) {
            const float* l = s.lights + 4 * (int64_t)li;
            const Vec3 L{l[0] - p.x, l[1] - p.y, l[2] - p.z};
            const float ll = sqrtf((L.x * L.x + L.y * L.y) + L.z * L.z);
            const float c = ((nrm.x * L.x + nrm.y * L.y) + nrm.z * L.z) / ll;
            const bool faces = hit && c > 0.0f;
            bool pending = faces;
            if (__ballot(pending) != 0) {  // (uniform) this light's walk
                const double Ld[3] = {L.x, L.y, L.z};
                for (int32_t j = 0; j < s.num_cubes; ++j) {
                    // the lane's own cube is skipped whole; a cube no pending
                    // lane has to test is skipped by the wave
                    const bool mine = pending && obj != j;
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
                    // (sphere sp is object num_cubes + sp; obj < 2^31 so the sum fits)
                    for (int32_t sp = 0; sp < s.num_spheres; ++sp) {
                        if (pending && obj - s.num_cubes != sp &&
                            rt_light::occluded_by_sphere(p, L, s.sphere_origins + 4 * (int64_t)sp,
                                                         s.sphere_radius[sp]))
                            pending = false;
                        if (__ballot(pending) == 0) break;
                    }
                }
            }
            if (faces) {
                if (pending)
                    k = k + c;  // not occluded
                else if (kOut == kOutMask)
                    mask |= 1u << (li & 31);  // (li < 32: the launch refuses more lights)
            }
        }
        if (hit && k > 1.0f) k = 1.0f;
    }
    if constexpr (kOut == kOutMask) {
        reinterpret_cast<uint32_t*>(out)[i] = mask;
    } else {
        int32_t px[4];
        rt_light::shade_lit(t, k, rt_light::slot_colour(s, obj), px);
        if constexpr (kOut == kOutI32x4)
            reinterpret_cast<int4*>(out)[i] = make_int4(px[0], px[1], px[2], px[3]);
        else
            reinterpret_cast<uint32_t*>(out)[i] = rt_light::pack_rgba8(px);
    }
}

template <int kOut>
int launch(rt_ctx* ctx, const rt_hit* hits, const rt_scene* scene, const float* ray_dir,
           int32_t width, int32_t row_begin, int32_t row_end, void* out, void* stream) {
    constexpr uintptr_t kAlign = kOut == kOutI32x4 ? 16 : 4;
    if (!ctx || rt_light::check(hits, scene, ray_dir, width, row_begin, row_end, out) ||
        reinterpret_cast<uintptr_t>(hits) % sizeof(rt_hit) ||
        reinterpret_cast<uintptr_t>(out) % kAlign)
        return RT_ERR_INVALID_ARG;
    if (kOut == kOutMask && scene->num_lights > 32) return RT_ERR_UNSUPPORTED;
    const int64_t n = (int64_t)(row_end - row_begin) * width;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > INT32_MAX) return RT_ERR_UNSUPPORTED;
    if (hipSetDevice(rt_internal::ctx_device(ctx)) != hipSuccess) return RT_ERR_HIP;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : rt_internal::ctx_stream(ctx);
    if (!st) return RT_ERR_HIP;
    shadow_kernel<kOut><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(
        hits, out, n, width, row_begin, ray_dir[0], ray_dir[1], ray_dir[2], *scene);
    return hipGetLastError() == hipSuccess ? RT_OK : RT_ERR_HIP;
}

}  // namespace

namespace rt_internal {
// rt_init: load this translation unit's code object now
int preload_shadow_kernels() {
    hipFuncAttributes a;
    for (const void* k : {reinterpret_cast<const void*>(shadow_kernel<kOutI32x4>),
                          reinterpret_cast<const void*>(shadow_kernel<kOutRgba8>),
                          reinterpret_cast<const void*>(shadow_kernel<kOutMask>)})
        if (hipFuncGetAttributes(&a, k) != hipSuccess) return RT_ERR_HIP;
    return RT_OK;
}
}  // namespace rt_internal

extern "C" {

int rt_shadow_hits_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                          const float ray_dir[4], int32_t width, int32_t row_begin,
                          int32_t row_end, uint32_t* device_out, void* stream) {
    return launch<kOutMask>(ctx, device_hits, device_scene, ray_dir, width, row_begin, row_end,
                            device_out, stream);
}

int rt_light_hits_shadowed_device(rt_ctx* ctx, const rt_hit* device_hits,
                                  const rt_scene* device_scene, const float ray_dir[4],
                                  int32_t width, int32_t row_begin, int32_t row_end,
                                  int32_t out_format, void* device_out, void* stream) {
    if (out_format == RT_FORMAT_I32X4)
        return launch<kOutI32x4>(ctx, device_hits, device_scene, ray_dir, width, row_begin,
                                 row_end, device_out, stream);
    if (out_format == RT_FORMAT_RGBA8)
        return launch<kOutRgba8>(ctx, device_hits, device_scene, ray_dir, width, row_begin,
                                 row_end, device_out, stream);
    return RT_ERR_INVALID_ARG;
}

}  // extern "C"
