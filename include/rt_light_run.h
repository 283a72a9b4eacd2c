/*
 * rt_light_run.h -- the pixel loop of the host functions of the deferred light
 * pass (csrc/rt_light.cpp, csrc/rt_light_accel.cpp) and the store it shares with
 * csrc/rt_camera_light.cpp: one text for the three files.
 * Host only.  Internal: not installed, not part of the ABI.
 */
#ifndef RT_LIGHT_RUN_H
#define RT_LIGHT_RUN_H

#include <cstring>
#include <type_traits>

#include "rt_hip.h"
#include "rt_light_impl.h"

namespace rt_light {

// What a lit pixel function returns: the int32x4 pixel, stored in `fmt`.
struct Lit {
    int32_t p[4];
};

// The store of pixel i: a Lit in `fmt`, anything else (rt_surface, the uint32
// mask, a bounce's rt_hit) as it is.
template <typename Out>
void store_pixel(void* out, int64_t i, int32_t fmt, const Out& v) {
    if constexpr (!std::is_same_v<Out, Lit>)
        static_cast<Out*>(out)[i] = v;
    else if (fmt == RT_FORMAT_I32X4)
        std::memcpy(static_cast<int32_t*>(out) + 4 * i, v.p, sizeof v.p);
    else
        static_cast<uint32_t*>(out)[i] = pack_rgba8(v.p);
}

// The pixel loop of every host function: the argument check, then for every
// pixel of the band the id range check, `pixel(s, obj, verts, ox, oy, d, t)`
// (`obj` range-checked, `verts` = cube_verts(s, obj)) and the store of what it
// returns (store_pixel).  `mask`: the output holds one bit per light, so at
// most 32.
template <typename PixelFn>
int run(const rt_hit* hits, const rt_scene* scene, const float* ray_dir, int32_t width,
        int32_t row_begin, int32_t row_end, bool mask, int32_t fmt, void* out, PixelFn pixel) {
    const int rc = check(hits, scene, ray_dir, width, row_begin, row_end, out);
    if (rc) return rc;
    const rt_scene& s = *scene;
    if (mask && s.num_lights > 32) return RT_ERR_UNSUPPORTED;
    const int64_t n_slots = static_cast<int64_t>(s.num_cubes) + s.num_spheres;
    const Vec3 d{ray_dir[0], ray_dir[1], ray_dir[2]};
    int64_t i = 0;
    for (int32_t y = row_begin; y < row_end; ++y) {
        for (int32_t x = 0; x < width; ++x, ++i) {
            const float t = hits[i].t;
            const int32_t obj = hits[i].object;
            if (obj < -1 || obj >= n_slots) return RT_ERR_INVALID_ARG;
            const float ox = static_cast<float>(x), oy = static_cast<float>(y);
            store_pixel(out, i, fmt, pixel(s, obj, cube_verts(s, obj), ox, oy, d, t));
        }
    }
    return RT_OK;
}

}  // namespace rt_light

#endif /* RT_LIGHT_RUN_H */
