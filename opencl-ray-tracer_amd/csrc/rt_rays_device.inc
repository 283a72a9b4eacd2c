// rt_rays_device.inc -- what the translation units of the ray queries share
// (DESIGN.md §3.1f, g, j): the two ray prologues, the cast and the occlude
// kernel, the launch, and the lane-butterfly reduce of the record builds.
// Included once by each of rt_rays.hip, rt_accel.hip and rt_sphere_groups.hip
// (and for camera_ray_at by rt_camera_light.hip), behind rt_light_device.inc
// and the file's cull policy with its cull_of(); not a standalone translation
// unit.
//
// One ray per thread in 256-thread workgroups, one launch per call, no
// workspace.  A ray comes from the caller's array (two 16-byte loads per lane:
// consecutive lanes read consecutive 32-byte records, so a wave's two loads
// cover 2 KiB of whole cache lines between them) or from the camera in the
// kernel arguments and the lane's own index, with no load at all: a 4096 x
// 4096 ray buffer would be 512 MiB written and read again.
//
// The kernels are one text for the three families.  What a family culls by is
// a parameter pack of kernel arguments, `Cull... cull`, at the place those
// arguments always had: nothing (rt_rays.hip), the cube records (rt_accel.hip),
// the cube records, the group records and their count (rt_sphere_groups.hip).
// cull_of(cull...) is the family's policy for the walks of rt_light_device.inc:
// rt_light_impl.h's for no argument, rt_accel_impl.h's for the cube records,
// rt_sphere_groups.hip's for both kinds of record.
// (A pack and not a policy struct as the argument: an empty struct would still
// take a slot and move `n` out of the preloaded dwords.)
#include "rt_rays_impl.h"

namespace {

using rt_light::cull_of;

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
template <int kSource, typename... Cull>
__global__ void __launch_bounds__(256)
cast_kernel(const rt_ray* __restrict__ rays, rt_hit* __restrict__ out_hits,
            int32_t* __restrict__ out_triangle, Cull... cull, int64_t n, int32_t width,
            int32_t row_begin, rt_camera cam, rt_scene s) {
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
    const rt_light::Bounce b = wave_bounce_walk(s, r.o, r.d, skip, live, cull_of(cull...));
    if (live) {
        reinterpret_cast<int2*>(out_hits)[i] = make_int2(__float_as_int(b.best), b.obj2);
        if (out_triangle) out_triangle[i] = b.tri2;
    }
}

// Is the open segment (o, o + d) of every ray cut by an object other than its
// `skip`: one byte per ray.
template <typename... Cull>
__global__ void __launch_bounds__(256)
occlude_kernel(const rt_ray* __restrict__ rays, uint8_t* __restrict__ out, Cull... cull, int64_t n,
               rt_scene s) {
    const int64_t i = pixel_index();
    const bool live = i < n;
    rt_light::Ray r{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    int32_t skip = -1;
    if (live) r = load_ray(rays, i, s, skip);
    const double pd[3] = {r.o.x, r.o.y, r.o.z};
    // still pending: not occluded
    const bool clear = occluder_walk(s, pd, r.o, r.d, skip, live, cull_of(cull...));
    if (live) out[i] = clear ? 0 : 1;
}

// What every entry point does after its checks: the device, the stream, one
// call of `enqueue(grid, stream)` with a grid of one workgroup per `per_block`
// of the `n` items.
template <typename Enqueue>
int launch_rays(rt_ctx* ctx, int64_t n, int64_t per_block, void* stream, Enqueue enqueue) {
    if (n == 0) return RT_OK;
    const int64_t blocks = (n + per_block - 1) / per_block;  // (<= INT32_MAX: the checks)
    if (hipSetDevice(rt_internal::ctx_device(ctx)) != hipSuccess) return RT_ERR_HIP;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : rt_internal::ctx_stream(ctx);
    if (!st) return RT_ERR_HIP;
    enqueue(dim3((unsigned)blocks), st);
    return hipGetLastError() == hipSuccess ? RT_OK : RT_ERR_HIP;
}

// The reduce of the record builds: `v` over the 2 * first lanes that differ
// from the lane in the bits below, by a butterfly, so every one of them holds
// the result.  MinOf and MaxOf do not depend on the order they meet values in.
struct MinOf {
    template <typename T>
    __device__ T operator()(T a, T b) const {
        return b < a ? b : a;
    }
};
struct MaxOf {
    template <typename T>
    __device__ T operator()(T a, T b) const {
        return b > a ? b : a;
    }
};
template <typename T, typename F>
__device__ __forceinline__ T lanes_reduce(T v, int first, F f) {
    for (int m = first; m >= 1; m >>= 1) v = f(v, __shfl_xor(v, m));
    return v;
}

}  // namespace
