// rt_accel.hip -- rt_accel_build_device and rt_cast_rays_accel_device /
// rt_occlude_rays_accel_device / rt_cast_camera_accel_device: the culled ray
// queries on the device.  The kernels of rt_rays.hip with
// one more condition in front of a cube's twelve triangle tests: the keep test
// of include/rt_accel_impl.h on the cube's prebuilt record, the text the host
// functions compile.
//
// The walks are rt_light_device.inc's over CubeCull of rt_accel_impl.h,
// which the culled light pass shares: they stay wave-uniform, so the scene and
// now the record (320 bytes per cube) come through scalar loads, once per wave.
// The ballot skips a cube where no lane of the wave keeps it, so coherent rays
// profit most.
//
// The ray prologues, cast_kernel, occlude_kernel, the launch and the build's
// reduce are rt_rays_device.inc's; here the kernels take the records as their
// one cull argument.
#include "rt_light_device.inc"
#include "rt_accel_impl.h"
#include "rt_rays_device.inc"

namespace {

// rt_light::cube_bound for a wave: one wave per cube, four per workgroup.
// Lanes 0..35 hold one vertex each (one coalesced 576-byte read; the lanes
// above repeat vertex 0, which changes no minimum or maximum); lane 3k holds
// triangle k after two shuffles and computes its edges and normal by the
// host's text; min, max and the largest edge are butterflies, whose result
// does not depend on the order.  Lane 0 stores the 32-byte head as two
// 16-byte stores, lane 3k its normal.
__global__ void __launch_bounds__(256)
accel_build_kernel(const float* __restrict__ cube_vertices, rt_cube_bound* __restrict__ out,
                   int32_t num_cubes) {
    const int32_t lane = threadIdx.x & 63;
    const int32_t j = (int32_t)blockIdx.x * 4 + (int32_t)(threadIdx.x >> 6);  // (< 2^31: the grid)
    if (j >= num_cubes) return;  // (wave-uniform)
    const float4 v = reinterpret_cast<const float4*>(cube_vertices)[36 * (int64_t)j +
                                                                    (lane < 36 ? lane : 0)];
    const bool bad = !(rt_light::finite_f(v.x) && rt_light::finite_f(v.y) && rt_light::finite_f(v.z));
    const bool finite = __ballot(bad) == 0;
    // triangle k in lane 3k: v1 and v2 from the next two lanes
    float tri[12] = {v.x, v.y, v.z, 0.0f, __shfl_down(v.x, 1), __shfl_down(v.y, 1),
                     __shfl_down(v.z, 1), 0.0f, __shfl_down(v.x, 2), __shfl_down(v.y, 2),
                     __shfl_down(v.z, 2), 0.0f};
    const bool owns = lane < 36 && lane % 3 == 0;
    double nrm[3] = {0.0, 0.0, 0.0}, emax = 0.0;
    if (owns && finite) {
        const double l1 = rt_light::edge_len2(tri, tri + 4), l2 = rt_light::edge_len2(tri, tri + 8);
        emax = l1 > l2 ? l1 : l2;
        rt_light::tri_normal(tri, nrm);
    }
    const float inf = __builtin_huge_valf();
    float4 lo, hi;
    if (finite) {
        // (+ 0.0f: a zero bound is +0 whichever of -0 and +0 the order met first)
        lo = make_float4(lanes_reduce(v.x, 32, MinOf{}) + 0.0f,
                         lanes_reduce(v.y, 32, MinOf{}) + 0.0f,
                         lanes_reduce(v.z, 32, MinOf{}) + 0.0f, 0.0f);
        hi = make_float4(lanes_reduce(v.x, 32, MaxOf{}) + 0.0f,
                         lanes_reduce(v.y, 32, MaxOf{}) + 0.0f,
                         lanes_reduce(v.z, 32, MaxOf{}) + 0.0f, 0.0f);
        emax = lanes_reduce(emax, 32, MaxOf{});
        lo.w = rt_light::float_up(emax);
    } else {
        lo = make_float4(-inf, -inf, -inf, inf);
        hi = make_float4(inf, inf, inf, 0.0f);
    }
    rt_cube_bound* o = out + j;
    if (lane == 0) {
        reinterpret_cast<float4*>(o)[0] = lo;
        reinterpret_cast<float4*>(o)[1] = hi;
    }
    if (owns) {
        double* nk = o->normal[lane / 3];
        nk[0] = nrm[0];
        nk[1] = nrm[1];
        nk[2] = nrm[2];
    }
}

}  // namespace

extern "C" {

int rt_accel_build_device(rt_ctx* ctx, const rt_scene* device_scene, rt_cube_bound* device_out,
                          void* stream) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int rc = rt_light::check_accel_build(device_scene, device_out);
    if (rc) return rc;
    return launch_rays(ctx, device_scene->num_cubes, 4, stream, [&](dim3 grid, hipStream_t st) {
        accel_build_kernel<<<grid, dim3(256), 0, st>>>(device_scene->cube_vertices, device_out,
                                                       device_scene->num_cubes);
    });
}

int rt_cast_rays_accel_device(rt_ctx* ctx, const rt_ray* device_rays, int64_t n,
                              const rt_scene* device_scene, const rt_cube_bound* device_accel,
                              rt_hit* device_out_hits, int32_t* device_out_triangle,
                              void* stream) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = rt_light::check_rays(device_rays, n, device_scene, device_out_hits, sizeof(rt_hit),
                                  device_out_triangle);
    if (!rc) rc = rt_light::check_accel(device_scene, device_accel);
    if (rc) return rc;
    return launch_rays(ctx, n, 256, stream, [&](dim3 grid, hipStream_t st) {
        cast_kernel<kFromRays, const rt_cube_bound*><<<grid, dim3(256), 0, st>>>(
            device_rays, device_out_hits, device_out_triangle, device_accel, n, 1, 0, rt_camera{},
            *device_scene);
    });
}

int rt_occlude_rays_accel_device(rt_ctx* ctx, const rt_ray* device_rays, int64_t n,
                                 const rt_scene* device_scene, const rt_cube_bound* device_accel,
                                 uint8_t* device_out_occluded, void* stream) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = rt_light::check_rays(device_rays, n, device_scene, device_out_occluded, 1, nullptr);
    if (!rc) rc = rt_light::check_accel(device_scene, device_accel);
    if (rc) return rc;
    return launch_rays(ctx, n, 256, stream, [&](dim3 grid, hipStream_t st) {
        occlude_kernel<const rt_cube_bound*><<<grid, dim3(256), 0, st>>>(
            device_rays, device_out_occluded, device_accel, n, *device_scene);
    });
}

int rt_cast_camera_accel_device(rt_ctx* ctx, const rt_camera* camera, const rt_scene* device_scene,
                                const rt_cube_bound* device_accel, int32_t width,
                                int32_t row_begin, int32_t row_end, rt_hit* device_out_hits,
                                int32_t* device_out_triangle, void* stream) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = rt_light::check_camera(camera, device_scene, true, width, row_begin, row_end,
                                    device_out_hits, sizeof(rt_hit), device_out_triangle);
    if (!rc) rc = rt_light::check_accel(device_scene, device_accel);
    if (rc) return rc;
    const int64_t n = (int64_t)(row_end - row_begin) * width;
    return launch_rays(ctx, n, 256, stream, [&](dim3 grid, hipStream_t st) {
        cast_kernel<kFromCamera, const rt_cube_bound*><<<grid, dim3(256), 0, st>>>(
            nullptr, device_out_hits, device_out_triangle, device_accel, n, width, row_begin,
            *camera, *device_scene);
    });
}

}  // extern "C"
