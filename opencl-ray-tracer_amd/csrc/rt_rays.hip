// rt_rays.hip -- rt_cast_rays_device / rt_occlude_rays_device /
// rt_camera_rays_device / rt_cast_camera_device: the ray queries on the device
// (DESIGN.md §3.1f).  The walks of the light pass over rays of the caller's:
// the bounce walk of rt_reflect.hip (closest hit) and the shadow walk of
// rt_shadow.hip (any hit), as rt_light_device.inc has them; the camera
// arithmetic is include/rt_rays_impl.h, the text the host functions compile.
//
// One ray per thread in 256-thread workgroups, one launch per call, no
// workspace.  A ray comes from the caller's array (two 16-byte loads per lane:
// consecutive lanes read consecutive 32-byte records, so a wave's two loads
// cover 2 KiB of whole cache lines between them) or from the camera in the
// kernel arguments and the lane's own index, with no load at all: a 4096 x
// 4096 ray buffer would be 512 MiB written and read again.
//
// The walks are wave-uniform: cube, triangle and sphere are loop counters, so
// the scene comes through scalar loads, once per wave.  A lane indexes by a
// per-lane value only rays[i] and out[i]; its `skip` is range-checked in the
// prologue and then only compared.  The kernels are launch-uniform: whether
// the triangles are stored is a kernel argument.
//
// The walk is the unculled one (12 * cubes + spheres tests per ray, each
// triangle test in fp64): the geometric cull of DESIGN.md §3.5 is its own
// change, and these kernels are where it can be tried from arbitrary origins.
#include "rt_light_device.inc"
#include "rt_rays_impl.h"

namespace {

enum { kFromRays = 0, kFromCamera = 1 };

// Ray i of a ray array: two 16-byte loads.
__device__ __forceinline__ rt_light::Ray load_ray(const rt_ray* __restrict__ rays, int64_t i,
                                                  const rt_scene& s, int32_t& skip) {
    const float4* r = reinterpret_cast<const float4*>(rays) + 2 * i;
    const float4 a = r[0], b = r[1];
    skip = rt_light::ray_skip(s, __float_as_int(a.w));
    return rt_light::Ray{{a.x, a.y, a.z}, {b.x, b.y, b.z}};
}

// Ray i of a camera's band of n = rows * width pixels: pixel (i % width,
// row_begin + i / width), as load_pixel of rt_light_device.inc finds it.
__device__ __forceinline__ rt_light::Ray camera_ray_at(const rt_camera& cam, int64_t i, int64_t n,
                                                       int32_t width, int32_t row_begin) {
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
    return rt_light::camera_ray(cam, (float)x, (float)(row_begin + r));  // exact: both <= 2^24
}

// The closest hit of every ray.  `s` holds device pointers; `rays` is read
// with kFromRays only, `cam`, `width` and `row_begin` with kFromCamera only.
// `out_triangle` may be NULL (uniform).
template <int kSource>
__global__ void __launch_bounds__(256)
cast_kernel(const rt_ray* __restrict__ rays, rt_hit* __restrict__ out_hits,
            int32_t* __restrict__ out_triangle, int64_t n, int32_t width, int32_t row_begin,
            rt_camera cam, rt_scene s) {
    const int64_t i = pixel_index();
    const bool live = i < n;
    rt_light::Ray r{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    int32_t skip = -1;
    if constexpr (kSource == kFromRays) {
        if (live) r = load_ray(rays, i, s, skip);
    } else {
        // (every lane: no memory is touched, and the camera stays in scalar registers)
        r = camera_ray_at(cam, i, n, width, row_begin);
        // The ray is six opaque registers from here on, as a loaded one is.
        // Without this the compiler re-derives three of its doubles inside the
        // walk's triangle loop: 83 fp64 operations per triangle against 78.
        // (not volatile: an asm with side effects would stand between the kernel
        // arguments and their scalar loads)
        asm("" : "+v"(r.o.x), "+v"(r.o.y), "+v"(r.o.z), "+v"(r.d.x), "+v"(r.d.y), "+v"(r.d.z));
    }
    const rt_light::Bounce b = wave_bounce_walk(s, r.o, r.d, skip, live);
    if (live) {
        reinterpret_cast<int2*>(out_hits)[i] = make_int2(__float_as_int(b.best), b.obj2);
        if (out_triangle) out_triangle[i] = b.tri2;
    }
}

// Is the open segment (o, o + d) of every ray cut by an object other than its
// `skip`: one byte per ray.
__global__ void __launch_bounds__(256)
occlude_kernel(const rt_ray* __restrict__ rays, uint8_t* __restrict__ out, int64_t n, rt_scene s) {
    const int64_t i = pixel_index();
    const bool live = i < n;
    rt_light::Ray r{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    int32_t skip = -1;
    if (live) r = load_ray(rays, i, s, skip);
    const double pd[3] = {r.o.x, r.o.y, r.o.z};
    const bool clear = occluder_walk(s, pd, r.o, r.d, skip, live);  // still pending: not occluded
    if (live) out[i] = clear ? 0 : 1;
}

// The rays of a camera's band: two 16-byte stores per lane.
__global__ void __launch_bounds__(256)
camera_kernel(rt_ray* __restrict__ out, int64_t n, int32_t width, int32_t row_begin,
              rt_camera cam) {
    const int64_t i = pixel_index();
    if (i >= n) return;
    const rt_light::Ray r = camera_ray_at(cam, i, n, width, row_begin);
    float4* o = reinterpret_cast<float4*>(out) + 2 * i;
    o[0] = make_float4(r.o.x, r.o.y, r.o.z, __int_as_float(-1));  // skip = -1
    o[1] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);                // reserved = 0
}

// What every entry point does after its checks: the device, the stream, one
// launch of `blocks(n)` workgroups by `enqueue(grid, stream)`.
template <typename Enqueue>
int launch_rays(rt_ctx* ctx, int64_t n, void* stream, Enqueue enqueue) {
    if (n == 0) return RT_OK;
    const int64_t blocks = (n + 255) / 256;  // (<= INT32_MAX: the checks refuse more rays)
    if (hipSetDevice(rt_internal::ctx_device(ctx)) != hipSuccess) return RT_ERR_HIP;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : rt_internal::ctx_stream(ctx);
    if (!st) return RT_ERR_HIP;
    enqueue(dim3((unsigned)blocks), st);
    return hipGetLastError() == hipSuccess ? RT_OK : RT_ERR_HIP;
}

}  // namespace

namespace rt_internal {
int preload_rays_kernels() {
    return preload({reinterpret_cast<const void*>(cast_kernel<kFromRays>),
                    reinterpret_cast<const void*>(cast_kernel<kFromCamera>),
                    reinterpret_cast<const void*>(occlude_kernel),
                    reinterpret_cast<const void*>(camera_kernel)});
}
}  // namespace rt_internal

extern "C" {

int rt_cast_rays_device(rt_ctx* ctx, const rt_ray* device_rays, int64_t n,
                        const rt_scene* device_scene, rt_hit* device_out_hits,
                        int32_t* device_out_triangle, void* stream) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int rc = rt_light::check_rays(device_rays, n, device_scene, device_out_hits,
                                        sizeof(rt_hit), device_out_triangle);
    if (rc) return rc;
    return launch_rays(ctx, n, stream, [&](dim3 grid, hipStream_t st) {
        cast_kernel<kFromRays><<<grid, dim3(256), 0, st>>>(device_rays, device_out_hits,
                                                           device_out_triangle, n, 1, 0,
                                                           rt_camera{}, *device_scene);
    });
}

int rt_occlude_rays_device(rt_ctx* ctx, const rt_ray* device_rays, int64_t n,
                           const rt_scene* device_scene, uint8_t* device_out_occluded,
                           void* stream) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int rc =
        rt_light::check_rays(device_rays, n, device_scene, device_out_occluded, 1, nullptr);
    if (rc) return rc;
    return launch_rays(ctx, n, stream, [&](dim3 grid, hipStream_t st) {
        occlude_kernel<<<grid, dim3(256), 0, st>>>(device_rays, device_out_occluded, n,
                                                   *device_scene);
    });
}

int rt_camera_rays_device(rt_ctx* ctx, const rt_camera* camera, int32_t width, int32_t row_begin,
                          int32_t row_end, rt_ray* device_out_rays, void* stream) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int rc = rt_light::check_camera(camera, nullptr, false, width, row_begin, row_end,
                                          device_out_rays, 16, nullptr);
    if (rc) return rc;
    const int64_t n = (int64_t)(row_end - row_begin) * width;
    return launch_rays(ctx, n, stream, [&](dim3 grid, hipStream_t st) {
        camera_kernel<<<grid, dim3(256), 0, st>>>(device_out_rays, n, width, row_begin, *camera);
    });
}

int rt_cast_camera_device(rt_ctx* ctx, const rt_camera* camera, const rt_scene* device_scene,
                          int32_t width, int32_t row_begin, int32_t row_end,
                          rt_hit* device_out_hits, int32_t* device_out_triangle, void* stream) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int rc = rt_light::check_camera(camera, device_scene, true, width, row_begin, row_end,
                                          device_out_hits, sizeof(rt_hit), device_out_triangle);
    if (rc) return rc;
    const int64_t n = (int64_t)(row_end - row_begin) * width;
    return launch_rays(ctx, n, stream, [&](dim3 grid, hipStream_t st) {
        cast_kernel<kFromCamera><<<grid, dim3(256), 0, st>>>(nullptr, device_out_hits,
                                                             device_out_triangle, n, width,
                                                             row_begin, *camera, *device_scene);
    });
}

}  // extern "C"
