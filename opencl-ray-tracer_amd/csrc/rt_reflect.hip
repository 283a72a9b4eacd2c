// rt_reflect.hip -- rt_reflect_hits_device / rt_light_hits_reflected_device: the
// mirror bounce of the deferred light pass, on the device.
//
// One kernel template over the output (bounce frame, int32x4, RGBA8): the
// pixel prologue, the surface step, the mirrored direction, the bounce walk,
// one 8-, 16- or 4-byte store.  No workspace, one launch.
//
// The walk is what the kernel costs: 12 * cubes + spheres tests per hit pixel,
// each triangle test in fp64.  A wave without a hit lane never enters it, nor
// does a lit launch with reflectivity 0 (a uniform branch on the kernel
// argument).  After it the lit forms read the bounce's triangle or centre and
// its colour by obj2 / tri2, which the walk took from its own loop counters.
#include "rt_light_device.inc"

namespace {

enum { kOutBounce = 2 };

// `s` holds device pointers.  `refl`: the lit forms' reflectivity.
template <int kOut>
__global__ void __launch_bounds__(256)
reflect_kernel(const rt_hit* __restrict__ hits, void* __restrict__ out, int64_t n, int32_t width,
               int32_t row_begin, float dx, float dy, float dz, float refl, rt_scene s) {
    using rt_light::Vec3;
    const int64_t i = pixel_index();
    if (i >= n) return;
    const Vec3 d{dx, dy, dz};
    float ox, oy;
    int32_t obj;
    const float t = load_pixel(hits, i, n, width, row_begin, s, ox, oy, obj);
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
            const Vec3 nrm = surface_step(s, obj, ox, oy, d, t, p);
            if (kOut != kOutBounce && s.num_lights > 0)
                k = rt_light::light_factor(nrm, p, s.lights, s.num_lights);
            R = rt_light::mirror_dir(nrm, d);
        }
        if (mirrors && __ballot(casts) != 0)  // (uniform) the walk
            b = wave_bounce_walk(s, p, R, obj, casts);
    }
    if constexpr (kOut == kOutBounce) {
        reinterpret_cast<int2*>(out)[i] = make_int2(__float_as_int(b.best), b.obj2);
    } else {
        int32_t lit[4];
        if (mirrors && casts)
            rt_light::shade_mirrored(s, obj, t, k, p, R, b, refl, lit);
        else
            rt_light::shade_lit(t, k, rt_light::slot_colour(s, obj), lit);
        store_lit<kOut>(out, i, lit);
    }
}

}  // namespace

namespace rt_internal {
int preload_reflect_kernels() {
    return preload({reinterpret_cast<const void*>(reflect_kernel<kOutI32x4>),
                    reinterpret_cast<const void*>(reflect_kernel<kOutRgba8>),
                    reinterpret_cast<const void*>(reflect_kernel<kOutBounce>)});
}
}  // namespace rt_internal

extern "C" {

int rt_reflect_hits_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                           const float ray_dir[4], int32_t width, int32_t row_begin,
                           int32_t row_end, rt_hit* device_out, void* stream) {
    return launch(KeepAll{}, 0, reflect_kernel<kOutBounce>, 8, false, ctx, device_hits,
                  device_scene, ray_dir, width, row_begin, row_end, device_out, stream, 0.0f);
}

int rt_light_hits_reflected_device(rt_ctx* ctx, const rt_hit* device_hits,
                                   const rt_scene* device_scene, const float ray_dir[4],
                                   int32_t width, int32_t row_begin, int32_t row_end,
                                   float reflectivity, int32_t out_format, void* device_out,
                                   void* stream) {
    return launch_lit(KeepAll{}, 0, reflect_kernel<kOutI32x4>, reflect_kernel<kOutRgba8>,
                      out_format, ctx, device_hits, device_scene, ray_dir, width, row_begin,
                      row_end, device_out, stream, reflectivity);
}

}  // extern "C"
