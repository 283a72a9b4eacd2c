// rt_light.cpp -- rt_hit_surfaces / rt_light_hits, the shadow term's
// rt_shadow_hits / rt_light_hits_shadowed and the mirror bounce's
// rt_reflect_hits / rt_light_hits_reflected and the two together,
// rt_shadow_hits_reflected / rt_light_hits_shadowed_reflected, on the host, and
// the argument check they share with the device entry points (rt_light.hip,
// rt_shadow.hip, rt_reflect.hip, rt_shadow_reflect.hip).
// Plain C++, no HIP.  The arithmetic is include/rt_light_impl.h, the text the
// kernel compiles too; built with -ffp-contract=off like rt_scene.cpp.
#include <cstring>

#include "rt_args.h"
#include "rt_hip.h"
#include "rt_light_impl.h"

namespace rt_light {

int check(const rt_hit* hits, const rt_scene* scene, const float* ray_dir, int32_t width,
          int32_t row_begin, int32_t row_end, const void* out) {
    if (!hits || !scene || !ray_dir || !out) return RT_ERR_INVALID_ARG;
    // a band of a frame of row_end rows: rt_render's own limits and counts
    if (rt_args::check_args(scene, width, row_end, row_begin, row_end, RT_FORMAT_I32X4))
        return RT_ERR_INVALID_ARG;
    if (scene->num_lights > 0 && !scene->lights) return RT_ERR_INVALID_ARG;
    return RT_OK;
}

namespace {

// kSurface: rt_surface per pixel; else a lit pixel in `fmt`.
template <bool kSurface>
int run(const rt_hit* hits, const rt_scene* scene, const float* ray_dir, int32_t width,
        int32_t row_begin, int32_t row_end, int32_t fmt, void* out) {
    const int rc = check(hits, scene, ray_dir, width, row_begin, row_end, out);
    if (rc) return rc;
    const rt_scene& s = *scene;
    const int64_t n_slots = static_cast<int64_t>(s.num_cubes) + s.num_spheres;
    const Vec3 d{ray_dir[0], ray_dir[1], ray_dir[2]};
    int64_t i = 0;
    for (int32_t y = row_begin; y < row_end; ++y) {
        for (int32_t x = 0; x < width; ++x, ++i) {
            const float t = hits[i].t;
            const int32_t obj = hits[i].object;
            if (obj < -1 || obj >= n_slots) return RT_ERR_INVALID_ARG;
            const float ox = static_cast<float>(x), oy = static_cast<float>(y);
            const float* verts = cube_verts(s, obj);
            if constexpr (kSurface) {
                static_cast<rt_surface*>(out)[i] =
                    surface(s, obj, verts, ox, oy, d, t, hit_point(ox, oy, d, t));
            } else {
                int32_t p[4];
                lit_pixel(s, obj, verts, ox, oy, d, t, p);
                if (fmt == RT_FORMAT_I32X4)
                    std::memcpy(static_cast<int32_t*>(out) + 4 * i, p, sizeof p);
                else
                    static_cast<uint32_t*>(out)[i] = pack_rgba8(p);
            }
        }
    }
    return RT_OK;
}

// The shadow term.  kMask: the uint32 mask per pixel; else
// the lit pixel with the occluded lights left out, in `fmt`.
template <bool kMask>
int run_shadowed(const rt_hit* hits, const rt_scene* scene, const float* ray_dir, int32_t width,
                 int32_t row_begin, int32_t row_end, int32_t fmt, void* out) {
    const int rc = check(hits, scene, ray_dir, width, row_begin, row_end, out);
    if (rc) return rc;
    const rt_scene& s = *scene;
    if (kMask && s.num_lights > 32) return RT_ERR_UNSUPPORTED;
    const int64_t n_slots = static_cast<int64_t>(s.num_cubes) + s.num_spheres;
    const Vec3 d{ray_dir[0], ray_dir[1], ray_dir[2]};
    int64_t i = 0;
    for (int32_t y = row_begin; y < row_end; ++y) {
        for (int32_t x = 0; x < width; ++x, ++i) {
            const float t = hits[i].t;
            const int32_t obj = hits[i].object;
            if (obj < -1 || obj >= n_slots) return RT_ERR_INVALID_ARG;
            const float ox = static_cast<float>(x), oy = static_cast<float>(y);
            const float* verts = cube_verts(s, obj);
            if constexpr (kMask) {
                static_cast<uint32_t*>(out)[i] = shadow_pixel(s, obj, verts, ox, oy, d, t);
            } else {
                int32_t p[4];
                lit_pixel_shadowed(s, obj, verts, ox, oy, d, t, p);
                if (fmt == RT_FORMAT_I32X4)
                    std::memcpy(static_cast<int32_t*>(out) + 4 * i, p, sizeof p);
                else
                    static_cast<uint32_t*>(out)[i] = pack_rgba8(p);
            }
        }
    }
    return RT_OK;
}

// The mirror bounce.  kBounce: the bounce's rt_hit per
// pixel; else the lit pixel blended by r (!= 0) with what it mirrors, in `fmt`.
template <bool kBounce>
int run_reflected(const rt_hit* hits, const rt_scene* scene, const float* ray_dir, int32_t width,
                  int32_t row_begin, int32_t row_end, float r, int32_t fmt, void* out) {
    const int rc = check(hits, scene, ray_dir, width, row_begin, row_end, out);
    if (rc) return rc;
    const rt_scene& s = *scene;
    const int64_t n_slots = static_cast<int64_t>(s.num_cubes) + s.num_spheres;
    const Vec3 d{ray_dir[0], ray_dir[1], ray_dir[2]};
    int64_t i = 0;
    for (int32_t y = row_begin; y < row_end; ++y) {
        for (int32_t x = 0; x < width; ++x, ++i) {
            const float t = hits[i].t;
            const int32_t obj = hits[i].object;
            if (obj < -1 || obj >= n_slots) return RT_ERR_INVALID_ARG;
            const float ox = static_cast<float>(x), oy = static_cast<float>(y);
            const float* verts = cube_verts(s, obj);
            if constexpr (kBounce) {
                const Bounce b = bounce_pixel(s, obj, verts, ox, oy, d, t);
                static_cast<rt_hit*>(out)[i] = rt_hit{b.best, b.obj2};
            } else {
                int32_t p[4];
                lit_pixel_reflected(s, obj, verts, ox, oy, d, t, r, p);
                if (fmt == RT_FORMAT_I32X4)
                    std::memcpy(static_cast<int32_t*>(out) + 4 * i, p, sizeof p);
                else
                    static_cast<uint32_t*>(out)[i] = pack_rgba8(p);
            }
        }
    }
    return RT_OK;
}

// Shadows and the mirror bounce together.  kMask: the uint32
// mask at the point the bounce meets; else the lit pixel, shadowed at the hit
// point and at that point, blended by r (!= 0), in `fmt`.
template <bool kMask>
int run_shadowed_reflected(const rt_hit* hits, const rt_scene* scene, const float* ray_dir,
                           int32_t width, int32_t row_begin, int32_t row_end, float r, int32_t fmt,
                           void* out) {
    const int rc = check(hits, scene, ray_dir, width, row_begin, row_end, out);
    if (rc) return rc;
    const rt_scene& s = *scene;
    if (kMask && s.num_lights > 32) return RT_ERR_UNSUPPORTED;
    const int64_t n_slots = static_cast<int64_t>(s.num_cubes) + s.num_spheres;
    const Vec3 d{ray_dir[0], ray_dir[1], ray_dir[2]};
    int64_t i = 0;
    for (int32_t y = row_begin; y < row_end; ++y) {
        for (int32_t x = 0; x < width; ++x, ++i) {
            const float t = hits[i].t;
            const int32_t obj = hits[i].object;
            if (obj < -1 || obj >= n_slots) return RT_ERR_INVALID_ARG;
            const float ox = static_cast<float>(x), oy = static_cast<float>(y);
            const float* verts = cube_verts(s, obj);
            if constexpr (kMask) {
                static_cast<uint32_t*>(out)[i] = shadow_reflect_pixel(s, obj, verts, ox, oy, d, t);
            } else {
                int32_t p[4];
                lit_pixel_shadowed_reflected(s, obj, verts, ox, oy, d, t, r, p);
                if (fmt == RT_FORMAT_I32X4)
                    std::memcpy(static_cast<int32_t*>(out) + 4 * i, p, sizeof p);
                else
                    static_cast<uint32_t*>(out)[i] = pack_rgba8(p);
            }
        }
    }
    return RT_OK;
}

}  // namespace
}  // namespace rt_light

extern "C" {

int rt_shadow_hits_reflected(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                             int32_t width, int32_t row_begin, int32_t row_end, uint32_t* out) {
    return rt_light::run_shadowed_reflected<true>(hits, scene, ray_dir, width, row_begin, row_end,
                                                  0.0f, 0, out);
}

int rt_light_hits_shadowed_reflected(const rt_hit* hits, const rt_scene* scene,
                                     const float ray_dir[4], int32_t width, int32_t row_begin,
                                     int32_t row_end, float reflectivity, int32_t out_format,
                                     void* out) {
    if (out_format != RT_FORMAT_I32X4 && out_format != RT_FORMAT_RGBA8) return RT_ERR_INVALID_ARG;
    if (!(reflectivity >= 0.0f && reflectivity <= 1.0f)) return RT_ERR_INVALID_ARG;  // NaN too
    if (reflectivity == 0.0f)  // rt_light_hits_shadowed's frame, neither the bounce nor its walk
        return rt_light::run_shadowed<false>(hits, scene, ray_dir, width, row_begin, row_end,
                                             out_format, out);
    return rt_light::run_shadowed_reflected<false>(hits, scene, ray_dir, width, row_begin, row_end,
                                                   reflectivity, out_format, out);
}

int rt_reflect_hits(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                    int32_t width, int32_t row_begin, int32_t row_end, rt_hit* out) {
    return rt_light::run_reflected<true>(hits, scene, ray_dir, width, row_begin, row_end, 0.0f, 0,
                                         out);
}

int rt_light_hits_reflected(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                            int32_t width, int32_t row_begin, int32_t row_end, float reflectivity,
                            int32_t out_format, void* out) {
    if (out_format != RT_FORMAT_I32X4 && out_format != RT_FORMAT_RGBA8) return RT_ERR_INVALID_ARG;
    if (!(reflectivity >= 0.0f && reflectivity <= 1.0f)) return RT_ERR_INVALID_ARG;  // NaN too
    if (reflectivity == 0.0f)  // rt_light_hits' frame, no walk
        return rt_light::run<false>(hits, scene, ray_dir, width, row_begin, row_end, out_format,
                                    out);
    return rt_light::run_reflected<false>(hits, scene, ray_dir, width, row_begin, row_end,
                                          reflectivity, out_format, out);
}

int rt_shadow_hits(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                   int32_t width, int32_t row_begin, int32_t row_end, uint32_t* out) {
    return rt_light::run_shadowed<true>(hits, scene, ray_dir, width, row_begin, row_end, 0, out);
}

int rt_light_hits_shadowed(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                           int32_t width, int32_t row_begin, int32_t row_end, int32_t out_format,
                           void* out) {
    if (out_format != RT_FORMAT_I32X4 && out_format != RT_FORMAT_RGBA8) return RT_ERR_INVALID_ARG;
    return rt_light::run_shadowed<false>(hits, scene, ray_dir, width, row_begin, row_end,
                                         out_format, out);
}

int rt_hit_surfaces(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                    int32_t width, int32_t row_begin, int32_t row_end, rt_surface* out) {
    return rt_light::run<true>(hits, scene, ray_dir, width, row_begin, row_end, 0, out);
}

int rt_light_hits(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4], int32_t width,
                  int32_t row_begin, int32_t row_end, int32_t out_format, void* out) {
    if (out_format != RT_FORMAT_I32X4 && out_format != RT_FORMAT_RGBA8) return RT_ERR_INVALID_ARG;
    return rt_light::run<false>(hits, scene, ray_dir, width, row_begin, row_end, out_format, out);
}

}  // extern "C"
