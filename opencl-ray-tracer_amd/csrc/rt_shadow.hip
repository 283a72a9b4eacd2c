// rt_shadow.hip -- rt_shadow_hits_device / rt_light_hits_shadowed_device: the
// shadow term of the deferred light pass, on the device.
//
// One kernel template over the output (mask, int32x4, RGBA8): the pixel
// prologue, the surface step, the shadow walk at the hit point, one 4- or
// 16-byte store.  No workspace, one launch.  (shadow_accel_kernel of
// rt_shadow_accel.hip is the mask form over CubeCull.  One body for both was
// one instruction shorter in the mask form and missed the timing rule on one
// line, so each keeps its text: profiles/chain_shared/README.md.)
//
// The walk is what the kernel costs: lights x (12 * cubes + spheres) tests
// per pixel, each triangle test in fp64.  A lane takes part only while it is
// pending (hit pixel, c > 0, not yet occluded for this light); a wave without
// a hit lane, or a launch without lights, never enters it.
#include "rt_light_device.inc"

namespace {

enum { kOutMask = 2 };

// `s` holds device pointers.
template <int kOut>
__global__ void __launch_bounds__(256)
shadow_kernel(const rt_hit* __restrict__ hits, void* __restrict__ out, int64_t n, int32_t width,
              int32_t row_begin, float dx, float dy, float dz, rt_scene s) {
    using rt_light::Vec3;
    const int64_t i = pixel_index();
    if (i >= n) return;
    const Vec3 d{dx, dy, dz};
    float ox, oy;
    int32_t obj;
    const float t = load_pixel(hits, i, n, width, row_begin, s, ox, oy, obj);
    const bool hit = obj >= 0;

    float k = 1.0f;
    uint32_t mask = 0;
    if (s.num_lights > 0 && __ballot(hit) != 0) {  // (uniform) else: no walk at all
        Vec3 p{0.0f, 0.0f, 0.0f}, nrm{0.0f, 0.0f, 0.0f};
        if (hit) {
            p = rt_light::hit_point(ox, oy, d, t);
            nrm = surface_step(s, obj, ox, oy, d, t, p);
        }
        k = light_walk<kOut == kOutMask>(s, p, nrm, obj, hit, mask);
    }
    if constexpr (kOut == kOutMask) {
        reinterpret_cast<uint32_t*>(out)[i] = mask;
    } else {
        int32_t lit[4];
        rt_light::shade_lit(t, k, rt_light::slot_colour(s, obj), lit);
        store_lit<kOut>(out, i, lit);
    }
}

}  // namespace

namespace rt_internal {
int preload_shadow_kernels() {
    return preload({reinterpret_cast<const void*>(shadow_kernel<kOutI32x4>),
                    reinterpret_cast<const void*>(shadow_kernel<kOutRgba8>),
                    reinterpret_cast<const void*>(shadow_kernel<kOutMask>)});
}
}  // namespace rt_internal

extern "C" {

int rt_shadow_hits_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                          const float ray_dir[4], int32_t width, int32_t row_begin,
                          int32_t row_end, uint32_t* device_out, void* stream) {
    return launch(KeepAll{}, 0, shadow_kernel<kOutMask>, 4, true, ctx, device_hits, device_scene,
                  ray_dir, width, row_begin, row_end, device_out, stream);
}

int rt_light_hits_shadowed_device(rt_ctx* ctx, const rt_hit* device_hits,
                                  const rt_scene* device_scene, const float ray_dir[4],
                                  int32_t width, int32_t row_begin, int32_t row_end,
                                  int32_t out_format, void* device_out, void* stream) {
    return launch_lit(KeepAll{}, 0, shadow_kernel<kOutI32x4>, shadow_kernel<kOutRgba8>,
                      out_format, ctx, device_hits, device_scene, ray_dir, width, row_begin,
                      row_end, device_out, stream);
}

}  // extern "C"
