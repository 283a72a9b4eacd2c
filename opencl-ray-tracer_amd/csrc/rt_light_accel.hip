// rt_light_accel.hip -- rt_bounce_hits_accel_device /
// rt_light_hits_mirrored_accel_device: the mirror chain of the deferred light
// pass over the prebuilt cube records, on the device.
// mirror_kernel (rt_mirror.hip) with the walks of rt_light_device.inc culled by
// CubeCull of rt_accel_impl.h: a lane tests a cube only where it is not its own
// and the keep test of include/rt_accel_impl.h keeps it for the lane's shadow
// segment or bounce.  What each call stores is its unculled call's output word
// for word.  The mask, rt_shadow_hits_accel_device, is
// rt_shadow_accel.hip.
//
// One kernel template over the output (int32x4, RGBA8, bounce frame).  The
// level loop, its ballots, the LDS blend stack (depth * 4 KiB of dynamic shared
// memory; none for the bounce frame) and the unwind are rt_mirror.hip's: both
// kernels are hit_chain_kernel of rt_chain_device.inc, here with the records
// as the second argument and `out` as the last.  The record
// comes through scalar loads: accel[j] is indexed by the walks' loop counters
// alone.  No workspace, one launch (launch() of rt_light_device.inc).
//
// Scalar registers are what the lit forms are short of.  The level loop keeps
// the scene's pointers, the record's, the reflectivity's and its own counters
// live across both walks, and the keep test wants the record's twelve normals
// (72 dwords) in flight at once: together that is past the 102 a wave has, and
// the compiler spills 35 of them to lanes of a VGPR.  So the keep test's loop
// over the normals stays a loop here (one normal's six dwords per trip), and
// `out`, which is read once at the end, is the last kernel argument, behind
// the ones that arrive preloaded in registers: no spill, and about 17 VGPRs
// fewer (profiles/light_accel/kernel_resources.md).
//
// rt_init does not load this translation unit's code object: the runtime
// loads it at the first launch of one of its kernels.
#include "rt_light_device.inc"
#ifndef RT_ACCEL_NORMALS_LOOP
#define RT_ACCEL_NORMALS_LOOP _Pragma("clang loop unroll(disable)")
#endif
#include "rt_accel_impl.h"
#include "rt_chain_device.inc"

namespace {

using rt_light::CubeCull;

template <int kOut>
constexpr auto light_accel_kernel = hit_chain_kernel<kOut, const rt_cube_bound*, void*>;

}  // namespace

extern "C" {

int rt_bounce_hits_accel_device(rt_ctx* ctx, const rt_hit* device_hits,
                                const rt_scene* device_scene, const rt_cube_bound* device_accel,
                                const float ray_dir[4], int32_t width, int32_t row_begin,
                                int32_t row_end, int32_t bounce, rt_hit* device_out,
                                void* stream) {
    if (bounce < 1 || bounce > RT_MAX_BOUNCES) return RT_ERR_INVALID_ARG;
    return launch(CubeCull{device_accel}, 0, light_accel_kernel<kOutBounce>, 8, false, ctx,
                  device_hits, device_scene, ray_dir, width, row_begin, row_end, device_out,
                  stream, (const float*)nullptr, bounce, 0);
}

int rt_light_hits_mirrored_accel_device(rt_ctx* ctx, const rt_hit* device_hits,
                                        const rt_scene* device_scene,
                                        const rt_cube_bound* device_accel, const float ray_dir[4],
                                        int32_t width, int32_t row_begin, int32_t row_end,
                                        const float* device_reflectivity, int32_t max_bounces,
                                        int32_t shadows, int32_t out_format, void* device_out,
                                        void* stream) {
    int32_t depth;
    size_t shared;
    const int rc = chain_settings(device_scene, device_reflectivity, max_bounces, shadows,
                                  out_format, depth, shared);
    if (rc) return rc;
    return launch_lit(CubeCull{device_accel}, shared, light_accel_kernel<kOutI32x4>,
                      light_accel_kernel<kOutRgba8>, out_format, ctx, device_hits, device_scene,
                      ray_dir, width, row_begin, row_end, device_out, stream,
                      device_reflectivity, depth, shadows);
}

}  // extern "C"
