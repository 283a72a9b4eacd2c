// rt_accel.cpp -- the culled ray queries on the host:
// rt_accel_build, rt_accel_kept, rt_cast_rays_accel, rt_occlude_rays_accel and
// rt_cast_camera_accel, and the argument checks they share with rt_accel.hip.
// The loops of include/rt_rays_run.h over CulledWalks of
// include/rt_accel_impl.h, the text the kernels compile too.
// Plain C++, no HIP; built with -ffp-contract=off like rt_light.cpp.
#include "rt_accel_impl.h"
#include "rt_args.h"
#include "rt_hip.h"
#include "rt_rays_run.h"

namespace rt_light {

int check_accel_build(const rt_scene* scene, const rt_cube_bound* out) {
    if (!scene) return RT_ERR_INVALID_ARG;
    // the scene alone, as check_rays() checks it
    if (rt_args::check_args(scene, 1, 1, 0, 1, RT_FORMAT_I32X4)) return RT_ERR_INVALID_ARG;
    if (scene->num_lights > 0 && !scene->lights) return RT_ERR_INVALID_ARG;
    return check_accel(scene, out);
}

int check_accel(const rt_scene* scene, const rt_cube_bound* accel) {
    if (scene->num_cubes > 0 && (!accel || misaligned(accel, 16))) return RT_ERR_INVALID_ARG;
    return RT_OK;
}

}  // namespace rt_light

extern "C" {

using namespace rt_light;

int rt_accel_build(const rt_scene* scene, rt_cube_bound* out) {
    const int rc = check_accel_build(scene, out);
    if (rc) return rc;
    for (int32_t j = 0; j < scene->num_cubes; ++j)
        out[j] = cube_bound(scene->cube_vertices + 144 * static_cast<int64_t>(j));
    return RT_OK;
}

// Per ray the number of cubes other than `skip` that the keep test keeps.
int rt_accel_kept(const rt_ray* rays, int64_t n, const rt_scene* scene,
                  const rt_cube_bound* accel, int32_t segment, int32_t* out_count) {
    if (segment != 0 && segment != 1) return RT_ERR_INVALID_ARG;
    int rc = check_rays(rays, n, scene, out_count, 4, nullptr);
    if (!rc) rc = check_accel(scene, accel);
    if (rc) return rc;
    return count_kept(rays, n, *scene, scene->num_cubes, out_count,
                      [=](const double* o, const double* d, int32_t j, int32_t skip) {
                          return j != skip && cube_kept(o, d, accel[j], segment != 0);
                      });
}

int rt_cast_rays_accel(const rt_ray* rays, int64_t n, const rt_scene* scene,
                       const rt_cube_bound* accel, rt_hit* out_hits, int32_t* out_triangle) {
    int rc = check_rays(rays, n, scene, out_hits, sizeof(rt_hit), out_triangle);
    if (!rc) rc = check_accel(scene, accel);
    return rc ? rc : cast_rays(rays, n, *scene, out_hits, out_triangle, CulledWalks{accel});
}

int rt_occlude_rays_accel(const rt_ray* rays, int64_t n, const rt_scene* scene,
                          const rt_cube_bound* accel, uint8_t* out_occluded) {
    int rc = check_rays(rays, n, scene, out_occluded, 1, nullptr);
    if (!rc) rc = check_accel(scene, accel);
    return rc ? rc : occlude_rays(rays, n, *scene, out_occluded, CulledWalks{accel});
}

int rt_cast_camera_accel(const rt_camera* camera, const rt_scene* scene,
                         const rt_cube_bound* accel, int32_t width, int32_t row_begin,
                         int32_t row_end, rt_hit* out_hits, int32_t* out_triangle) {
    int rc = check_camera(camera, scene, true, width, row_begin, row_end, out_hits, sizeof(rt_hit),
                          out_triangle);
    if (!rc) rc = check_accel(scene, accel);
    return rc ? rc
              : cast_camera(*camera, *scene, width, row_begin, row_end, out_hits, out_triangle,
                            CulledWalks{accel});
}

}  // extern "C"
