// rt_mirror.hip -- rt_bounce_hits_device / rt_light_hits_mirrored_device: the
// mirror chain of the deferred light pass, on the device:
// the bounce of rt_reflect.hip taken again from the point it meets, up to
// RT_MAX_BOUNCES times, with one reflectivity per colour slot and, on request,
// the shadow term at every level.
//
// One kernel template over the output (bounce frame, int32x4, RGBA8): the
// pixel prologue, the surface step, the level loop, the unwind, one 8-, 16- or
// 4-byte store: hit_chain_kernel of rt_chain_device.inc over the unculled
// walks, with `out` as its second argument.  No workspace, one launch (launch() of rt_light_device.inc with the
// chain's arguments and its shared memory).
//
// rt_init does not load this translation unit's code object: the runtime
// loads it at the first launch of one of its kernels.
#include "rt_light_device.inc"
#include "rt_chain_device.inc"

namespace {

template <int kOut>
constexpr auto mirror_kernel = hit_chain_kernel<kOut, void*>;

}  // namespace

extern "C" {

int rt_bounce_hits_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                          const float ray_dir[4], int32_t width, int32_t row_begin,
                          int32_t row_end, int32_t bounce, rt_hit* device_out, void* stream) {
    if (bounce < 1 || bounce > RT_MAX_BOUNCES) return RT_ERR_INVALID_ARG;
    return launch(KeepAll{}, 0, mirror_kernel<kOutBounce>, 8, false, ctx, device_hits,
                  device_scene, ray_dir, width, row_begin, row_end, device_out, stream,
                  (const float*)nullptr, bounce, 0);
}

int rt_light_hits_mirrored_device(rt_ctx* ctx, const rt_hit* device_hits,
                                  const rt_scene* device_scene, const float ray_dir[4],
                                  int32_t width, int32_t row_begin, int32_t row_end,
                                  const float* device_reflectivity, int32_t max_bounces,
                                  int32_t shadows, int32_t out_format, void* device_out,
                                  void* stream) {
    int32_t depth;
    size_t shared;
    const int rc = chain_settings(device_scene, device_reflectivity, max_bounces, shadows,
                                  out_format, depth, shared);
    if (rc) return rc;
    return launch_lit(KeepAll{}, shared, mirror_kernel<kOutI32x4>, mirror_kernel<kOutRgba8>,
                      out_format, ctx, device_hits, device_scene, ray_dir, width, row_begin,
                      row_end, device_out, stream, device_reflectivity, depth, shadows);
}

}  // extern "C"
