// rt_rays.hip -- rt_cast_rays_device / rt_occlude_rays_device /
// rt_camera_rays_device / rt_cast_camera_device: the ray queries on the device
// (DESIGN.md §3.1f).  The walks of the light pass over rays of the caller's:
// the bounce walk of rt_reflect.hip (closest hit) and the shadow walk of
// rt_shadow.hip (any hit), as rt_light_device.inc has them; the camera
// arithmetic is include/rt_rays_impl.h, the text the host functions compile.
// The ray prologues, cast_kernel, occlude_kernel and the launch are
// rt_rays_device.inc's, the text the culled families compile too; here they
// take no cull arguments.
//
// The walks are wave-uniform: cube, triangle and sphere are loop counters, so
// the scene comes through scalar loads, once per wave.  A lane indexes by a
// per-lane value only rays[i] and out[i]; its `skip` is range-checked in the
// prologue and then only compared.  The kernels are launch-uniform: whether
// the triangles are stored is a kernel argument.
//
// The walk is the unculled one (12 * cubes + spheres tests per ray, each
// triangle test in fp64): the culled ones are rt_accel.hip's and
// rt_sphere_groups.hip's.
#include "rt_light_device.inc"
#include "rt_rays_device.inc"

namespace {

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

}  // namespace

namespace rt_internal {
int preload_rays_kernels() {
    return preload({reinterpret_cast<const void*>(cast_kernel<kFromRays>),
                    reinterpret_cast<const void*>(cast_kernel<kFromCamera>),
                    reinterpret_cast<const void*>(occlude_kernel<>),
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
    return launch_rays(ctx, n, 256, stream, [&](dim3 grid, hipStream_t st) {
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
    return launch_rays(ctx, n, 256, stream, [&](dim3 grid, hipStream_t st) {
        occlude_kernel<><<<grid, dim3(256), 0, st>>>(device_rays, device_out_occluded, n,
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
    return launch_rays(ctx, n, 256, stream, [&](dim3 grid, hipStream_t st) {
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
    return launch_rays(ctx, n, 256, stream, [&](dim3 grid, hipStream_t st) {
        cast_kernel<kFromCamera><<<grid, dim3(256), 0, st>>>(nullptr, device_out_hits,
                                                             device_out_triangle, n, width,
                                                             row_begin, *camera, *device_scene);
    });
}

}  // extern "C"
