// rt_light.hip -- rt_hit_surfaces_device / rt_light_hits_device: surface
// normals, triangle ids and diffuse lighting from an RT_FORMAT_HIT frame, on
// the device.
//
// One kernel template over the output (rt_surface, int32x4, RGBA8), one
// pixel per thread in 256-thread workgroups: an 8-byte load of the pixel's
// rt_hit, the arithmetic of include/rt_light_impl.h (the text the host
// functions of rt_light.cpp compile, so the two agree bit for bit), one
// 16-byte or 4-byte store.  A cube pixel runs up to twelve fp64 triangle
// tests to find which triangle gave its t (what bounds the kernel: it is
// compute-bound on them); a sphere pixel needs one
// normalisation.  The lights are indexed by the loop counter alone, so every
// lane reads the same address (scalar loads).
//
// rt_trace.inc is not included: its shade / (int) helpers are restated in
// rt_light_impl.h, and including it would instantiate every trace kernel a
// second time.
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

enum { kOutI32x4 = 0, kOutRgba8 = 1, kOutSurface = 2 };

// `s` holds device pointers.  n = rows * width pixels; pixel i is
// (i % width, row_begin + i / width).
template <int kOut>
__global__ void __launch_bounds__(256)
light_kernel(const rt_hit* __restrict__ hits, void* __restrict__ out, int64_t n, int32_t width,
             int32_t row_begin, float dx, float dy, float dz, rt_scene s) {
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
    const rt_light::Vec3 d{dx, dy, dz};
    const int2 h = reinterpret_cast<const int2*>(hits)[i];
    const float t = __int_as_float(h.x);
    int32_t obj = h.y;
    // the range check in front of every index: a foreign id is no object
    if (obj < -1 || (int64_t)obj >= (int64_t)s.num_cubes + s.num_spheres) obj = -1;
    const auto pixel = [&](const float* verts) {
        if constexpr (kOut == kOutSurface) {
            const rt_surface v = rt_light::surface(s, obj, verts, ox, oy, d, t,
                                                   rt_light::hit_point(ox, oy, d, t));
            reinterpret_cast<float4*>(out)[i] =
                make_float4(v.nx, v.ny, v.nz, __uint_as_float((uint32_t)v.triangle));
        } else {
            int32_t p[4];
            rt_light::lit_pixel(s, obj, verts, ox, oy, d, t, p);
            if constexpr (kOut == kOutI32x4)
                reinterpret_cast<int4*>(out)[i] = make_int4(p[0], p[1], p[2], p[3]);
            else
                reinterpret_cast<uint32_t*>(out)[i] = rt_light::pack_rgba8(p);
        }
    };
    const float* verts = rt_light::cube_verts(s, obj);
    // Neighbouring pixels mostly share their cube.  Where all cube lanes of
    // the wave hold one cube, its vertices come through a wave-uniform
    // pointer (scalar loads, once for the wave) and not as 64 equal gathers
    // per vertex: 11-17 % off the kernel at config 3 (profiles/light/).  Any
    // other wave takes the per-lane pointer; the arithmetic is the same.
    int c0 = 0;
    bool one = false;
    if (verts && (kOut == kOutSurface || s.num_lights > 0)) {  // the cube lanes that test triangles
        c0 = __builtin_amdgcn_readfirstlane(obj);
        one = __ballot(obj != c0) == 0;
    }
    if (one)
        pixel(s.cube_vertices + 144 * (int64_t)c0);
    else
        pixel(verts);
}

template <int kOut>
int launch(rt_ctx* ctx, const rt_hit* hits, const rt_scene* scene, const float* ray_dir,
           int32_t width, int32_t row_begin, int32_t row_end, void* out, void* stream) {
    constexpr uintptr_t kAlign = kOut == kOutRgba8 ? 4 : 16;
    if (!ctx || rt_light::check(hits, scene, ray_dir, width, row_begin, row_end, out) ||
        reinterpret_cast<uintptr_t>(hits) % sizeof(rt_hit) ||
        reinterpret_cast<uintptr_t>(out) % kAlign)
        return RT_ERR_INVALID_ARG;
    const int64_t n = (int64_t)(row_end - row_begin) * width;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > INT32_MAX) return RT_ERR_UNSUPPORTED;
    if (hipSetDevice(rt_internal::ctx_device(ctx)) != hipSuccess) return RT_ERR_HIP;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : rt_internal::ctx_stream(ctx);
    if (!st) return RT_ERR_HIP;
    light_kernel<kOut><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(
        hits, out, n, width, row_begin, ray_dir[0], ray_dir[1], ray_dir[2], *scene);
    return hipGetLastError() == hipSuccess ? RT_OK : RT_ERR_HIP;
}

}  // namespace

namespace rt_internal {
// rt_init: load this translation unit's code object now
int preload_light_kernels() {
    hipFuncAttributes a;
    for (const void* k : {reinterpret_cast<const void*>(light_kernel<kOutI32x4>),
                          reinterpret_cast<const void*>(light_kernel<kOutRgba8>),
                          reinterpret_cast<const void*>(light_kernel<kOutSurface>)})
        if (hipFuncGetAttributes(&a, k) != hipSuccess) return RT_ERR_HIP;
    return RT_OK;
}
}  // namespace rt_internal

extern "C" {

int rt_hit_surfaces_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                           const float ray_dir[4], int32_t width, int32_t row_begin,
                           int32_t row_end, rt_surface* device_out, void* stream) {
    return launch<kOutSurface>(ctx, device_hits, device_scene, ray_dir, width, row_begin, row_end,
                               device_out, stream);
}

int rt_light_hits_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                         const float ray_dir[4], int32_t width, int32_t row_begin,
                         int32_t row_end, int32_t out_format, void* device_out, void* stream) {
    if (out_format == RT_FORMAT_I32X4)
        return launch<kOutI32x4>(ctx, device_hits, device_scene, ray_dir, width, row_begin,
                                 row_end, device_out, stream);
    if (out_format == RT_FORMAT_RGBA8)
        return launch<kOutRgba8>(ctx, device_hits, device_scene, ray_dir, width, row_begin,
                                 row_end, device_out, stream);
    return RT_ERR_INVALID_ARG;
}

}  // extern "C"
