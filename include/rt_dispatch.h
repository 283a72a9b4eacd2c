/*
 * rt_dispatch.h -- the render dispatcher's policy (csrc/rt_dispatch.cpp):
 * which kernel chain a binned launch runs and with which parameters, and the
 * workspace it needs.  Host-only arithmetic like rt_args.h: no HIP types, so
 * that every rule runs on the CPU (tests/dispatch_check.cpp).  choose() is the
 * one statement of the rules; rt_trace.inc's launch() only enqueues what it
 * returns.  Internal: not installed, not part of the ABI.
 *
 * The RT_... macros below are compile-time defaults (A/B variants:
 * scripts/variants.sh passes -D to rt_device.hip).  They are read only by
 * Knobs' member initialisers, and only rt_device.hip creates a Knobs (inside
 * rt_ctx, and Knobs{} in the rt_debug_set_* functions): rt_dispatch.cpp reads
 * every value through the Knobs it is handed, so a -D needs to reach
 * rt_device.hip alone.
 */
#ifndef RT_DISPATCH_H
#define RT_DISPATCH_H

#include <stddef.h>
#include <stdint.h>

#include "rt_hip.h"
#include "rt_hip_debug.h"

#ifndef RT_BIN_MASKS
#define RT_BIN_MASKS 1            // default of rt_debug_set_bin_masks
#endif
#ifndef RT_COARSE_CULL
#define RT_COARSE_CULL 10  // default of rt_debug_set_coarse_cull: bins with >= 10 sphere candidates
#endif
#ifndef RT_COARSE_CULL_TRI
#define RT_COARSE_CULL_TRI 4  // default of rt_debug_set_coarse_cull_tri: triangles join the cull
                              // in bins whose tiles keep >= this many candidates on average
#endif
#ifndef RT_SMALL_FUSED
#define RT_SMALL_FUSED 1  // default of rt_debug_set_small_fused
#endif
#ifndef RT_COARSE_CULL_OVERDRAW
#define RT_COARSE_CULL_OVERDRAW 5  // default of rt_debug_set_coarse_cull_overdraw: ... in frames
                                   // whose primitive boxes cover the frame >= 5 times
#endif
#ifndef RT_COARSE_CULL_TRI_RGBA8
#define RT_COARSE_CULL_TRI_RGBA8 2  // the triangle threshold for Texture (RGBA8) renders
#endif
#ifndef RT_COARSE_CULL_OVERDRAW_RGBA8
#define RT_COARSE_CULL_OVERDRAW_RGBA8 0  // the same gate for Texture (RGBA8) renders: every
                                         // frame (its trace is bound by its tests, not by
                                         // its stores)
#endif
// ... and for hit-buffer (RT_FORMAT_HIT) renders, measured on HIT frames of
// config 3's scene at five object sizes: the triangle
// threshold of 2 is 1.6-2 us per frame faster than 4 wherever the cull runs,
// and the cull pays from a box overdraw of about 2 frames on (1.4: 41.5 us
// without, 44.2 with; 2.8: 43.7 / 43.1; 4.3: 49.6 / 43.5)
#ifndef RT_COARSE_CULL_TRI_HIT
#define RT_COARSE_CULL_TRI_HIT 2
#endif
#ifndef RT_COARSE_CULL_OVERDRAW_HIT
#define RT_COARSE_CULL_OVERDRAW_HIT 2
#endif
#ifndef RT_SPLIT4_TILES
#define RT_SPLIT4_TILES 2048  // trace3_split_kernel with 4 waves per tile up to this many tiles
#endif
#ifndef RT_SPLIT2_TILES
#define RT_SPLIT2_TILES 4096  // ... with 2 waves per tile up to this many (round 4: at
                              // 8160, 1920x1080, flat; 4 waves win below 2048 tiles,
                              // 2 up to 4096, one above)
#endif
#ifndef RT_COARSE_W8_BINS
#define RT_COARSE_W8_BINS 256  // coarse3_kernel with 8 waves per bin in bands up to this many
                               // bins (round 4: 80 and 240 bins 0.3-2.3 us faster than 4)
#endif
#ifndef RT_COARSE_W4_BINS
#define RT_COARSE_W4_BINS 1024  // coarse3_kernel with 4 waves per bin in bands up to this many
                                // bins (round 4: 4 waves fastest from 80 to 920 bins, one
                                // at 4096 and up)
#endif
#ifndef RT_COARSE_W2_BINS
#define RT_COARSE_W2_BINS 1024  // ... with 2 waves per bin up to this many (none by default)
#endif
#ifndef RT_TRACE_BIN_OD10
#define RT_TRACE_BIN_OD10 40  // trace_bin_kernel (auto) for int32x4 frames below this box overdraw,
                              // in tenths of a frame (round 5, one stream, config 3's scene scaled:
                              // overdraw 0.08 / 0.3 / 0.7 / 1.4 / 2.8 / 4.3 / 6.1 frames, coarse path
                              // 55.0 / 56.0 / 55.5 / 55.8 / 57.4 / 60.0 / 61.5 us per frame, no coarse
                              // 51.3 / 51.3 / 49.6 / 49.8 / 53.9 / 60.9 / 69.2)
#endif
#ifndef RT_TRACE_BIN_OD10_RGBA8
#define RT_TRACE_BIN_OD10_RGBA8 10  // ... for RGBA8 frames (same scenes: coarse path 37.5 / 39.3 /
                                    // 40.2 / 42.0 / 44.5 / 46.7 / 47.9, no coarse 29.9 / 31.6 / 34.3 /
                                    // 40.0 / 49.3 / 58.1 / 65.9; with 3 frames in flight at overdraw
                                    // 0.08 / 1.4 / 2.8: coarse 18.3 / 27.5 / 32.5, no coarse 17.3 /
                                    // 30.6 / 40.6, so 1 frame, not the one-stream crossover)
#endif
#ifndef RT_COARSE_CULL_TRI_BINS
#define RT_COARSE_CULL_TRI_BINS 768  // triangles join the cull only in bands of at least this
                                     // many coarse bins: fewer coarse waves run as one
                                     // generation and cannot hide the cull's latency (round 4:
                                     // 640x480 to 1920x1080 frames 1-27 us slower with it at
                                     // box overdraw 5-20, 2560x1440 up to 16 us faster;
                                     // DESIGN.md §3.5)
#endif

namespace rt_dispatch {

/* The working set of frame bytes from which the frame stores take
 * RT_STORE_LARGE (int32x4: nontemporal and written through).  Measured at
 * both sides of it (profiles/store_policy/README.md): one 256 MiB frame
 * written over and over loses with them (config 3 on one stream, 50.6 ->
 * 53.3 us per frame), two such frames in flight gain (45.7 -> 42.7), and so
 * does one 1 GiB frame (config 4, 193.9 -> 184.6).  512 MiB is where a single
 * frame already changed sides for nontemporal stores (Knobs::wide_tile_bytes). */
constexpr int64_t kStoreLargeBytes = (int64_t)1 << 29;
/* Renders a target stays in the working set for without being written again,
 * and the entries of the per-device ring (one per render of that window).
 * Twice the most slots a measured frame loop uses (the RGBA8 leg's 4,
 * DESIGN.md section 3.4), so every buffer of such a loop stays in it; loops of
 * 2 and 4 slots were measured with it. */
constexpr int kTargetWindow = 8;

/* Record a render of `bytes` bytes at `base` on `device` and return the
 * device's working set: the bytes of the union of the distinct targets of its
 * last kTargetWindow renders, by any context of the process (this one
 * included).  Thread-safe. */
int64_t track_target(int device, const void* base, int64_t bytes);
/* Forget every device's targets (tests). */
void reset_targets();

/* What one tile build (one inclusion of rt_trace.inc) contributes to the
 * policy: its coarse-bin shape, its kernels' capacities and the sizes of the
 * records its prep writes. */
struct Geometry {
    int coarse_w, coarse_h;  /* coarse bin (candidate list), pixels */
    int tiles_per_bin;       /* wave tiles per coarse bin */
    int list_stride;         /* list words per candidate: its id, then its tile words */
    int prep_threads;        /* primitives per prep workgroup (one chunk) */
    int fused_wg;            /* frame_small_kernel: wave tiles per workgroup */
    int fused_chunks;        /* frame_small_kernel: scenes of up to this many chunks */
    int small_chunks;        /* trace_small_kernel: the same */
    int bin_cap;             /* trace_bin_kernel: scenes of up to this many primitives */
    int mask_bins_max;       /* bin masks: frames of up to this many bin rows + columns */
    int tri_rec_bytes, sph_rec_bytes, cls_bytes, tri_depth_bytes;  /* TriRec, SphRec, Cls, TriDepth */
};

/* The policy's tunables: what the rt_debug_set_* functions set (rt_hip_debug.h
 * explains each), then the thresholds without a setter. */
struct Knobs {
    // coarse lists take 4 B x list_stride x (primitives + 16) per coarse bin; a frame whose
    // lists would exceed this is rendered as internal row bands
    int64_t list_budget = (int64_t)4 << 30;
    bool bin_masks = RT_BIN_MASKS != 0;  // separable bin masks (false: coarse scans every box)
    bool small_path = true;  // <= 64 x small_chunks primitives: trace_small_kernel
    // <= 64 x fused_chunks primitives on frames whose grid is resident at
    // once: frame_small_kernel (1; 2 = on every frame size, tests; 0 = off)
    int small_fused = RT_SMALL_FUSED;
    // waves per wave tile in the binned trace: 0 = by frame size
    // (trace3_split_kernel on small frames), 1 = one (trace3_kernel), 2 / 4
    int trace_split = 0;
    // waves per coarse bin: 0 = by band size, 1 / 2 / 4 / 8
    int coarse_waves = 0;
    // binned frames without the coarse kernel (trace_bin_kernel): 0 = auto
    // (frames above the split sizes whose last binned frame had a box
    // overdraw below the format's threshold), 1 = always where it applies,
    // 2 = never
    int trace_bin = 0;
    int tile_variant = 0;  // 0 = by frame size, 1 = 16x16 tiles, 2 = the wide (128x2) tiles
    // coarse depth cull of sphere candidates in bins with at least this many
    // candidates (0 = off)
    int coarse_cull = RT_COARSE_CULL;
    // triangles join the depth cull in bins whose tiles keep at least this
    // many candidates on average (0 = never)
    int coarse_cull_tri = RT_COARSE_CULL_TRI;
    int coarse_cull_tri_rgba8 = RT_COARSE_CULL_TRI_RGBA8;  // (RGBA8 renders)
    int coarse_cull_tri_hit = RT_COARSE_CULL_TRI_HIT;      // (HIT renders)
    // ... in frames whose boxes' summed area is at least this many frames
    // (int32x4 renders; RGBA8 and HIT renders take their own gates)
    unsigned coarse_cull_overdraw = RT_COARSE_CULL_OVERDRAW;
    unsigned coarse_cull_overdraw_rgba8 = RT_COARSE_CULL_OVERDRAW_RGBA8;
    unsigned coarse_cull_overdraw_hit = RT_COARSE_CULL_OVERDRAW_HIT;
    // ... in bands of at least this many coarse bins
    int64_t coarse_cull_tri_bins = RT_COARSE_CULL_TRI_BINS;

    // no setter: the frame-size thresholds of the split trace and the coarse
    // waves, the overdraw verdict's two thresholds (tenths of a frame)
    int64_t split4_tiles = RT_SPLIT4_TILES, split2_tiles = RT_SPLIT2_TILES;
    int64_t coarse_w8_bins = RT_COARSE_W8_BINS, coarse_w4_bins = RT_COARSE_W4_BINS,
            coarse_w2_bins = RT_COARSE_W2_BINS;
    unsigned long long trace_bin_od10 = RT_TRACE_BIN_OD10,
                       trace_bin_od10_rgba8 = RT_TRACE_BIN_OD10_RGBA8;
    // Frames of at least this many bytes take the wide tiles (auto selection):
    // 512 MiB frames store faster from wide tiles in both formats (config 5's
    // 8-rank band, config 4's half frame, a 512 MiB Texture; measured with 64x4
    // tiles), 384 MiB and smaller ones from 16x16.
    int64_t wide_tile_bytes = (int64_t)1 << 29;
    // The frame stores' cache policy (rt_debug_set_store_policy): RT_STORE_AUTO
    // = RT_STORE_LARGE once the frames in flight on the device (track_target)
    // reach store_large_bytes, else RT_STORE_DEFAULT.
    int store_policy = RT_STORE_AUTO;
    int64_t store_large_bytes = kStoreLargeBytes;
};

/* rt_debug_set_tile_variant: 0 = by frame size, 1 = 16x16, 2 = wide (128x2) */
bool use_wide_tiles(const Knobs& k, int32_t width, int32_t rows, int32_t fmt);

/* Workspace layout of one binned launch over `rows` rows (one band of a
 * frame launch() splits): every offset and size launch() uses, so that
 * reserve() sizes exactly what the launch will ask for. */
struct Plan {
    int n_tri, n_prims, n_cx, n_cy, n_chunks, half_cap;
    int64_t n_coarse;
    bool use_masks;
    size_t tri_off, sph_off, box_off, cls_off, col_off, cnt_off, mask_off, dep_off;
    size_t rec_need, list_need;
};
Plan plan(const Geometry& g, const Knobs& k, int n_spheres, int n_cubes, int32_t width,
          int32_t rows);

/* Rows per internal band of a binned launch: the whole range, or bands of
 * whole coarse rows when the candidate lists would pass the list budget or
 * the trace grid's y dimension (65535 bin rows). */
int64_t band_rows_of(const Geometry& g, const Knobs& k, int64_t n_prims, int32_t width,
                     int32_t rows);

/* What launch() enqueues for rows [row_begin, row_begin + rows). */
struct Decision {
    /* The chain, by the RT_KERNEL_* id of its dominant kernel:
     *   RT_KERNEL_GENERIC      generic_kernel
     *   RT_KERNEL_FRAME_SMALL  frame_small_kernel
     *   RT_KERNEL_TRACE_SMALL  prep_kernel -> trace_small_kernel
     *   RT_KERNEL_TRACE_BIN    prep_kernel -> trace_bin_kernel
     *   RT_KERNEL_TRACE_SPLIT  prep_kernel -> coarse3_kernel -> trace3_split_kernel
     *   RT_KERNEL_TRACE        prep_kernel -> coarse3_kernel -> trace3_kernel
     *                          (no primitives: neither prep nor coarse, empty lists)
     *   RT_KERNEL_NONE         nothing here: render bands of band_rows rows, each
     *                          chosen for by itself (band_rows < rows) */
    int chain;
    int64_t band_rows;  /* rows per internal band; `rows` when the launch is one band */
    Plan plan;          /* the binned chains' workspace (n_chunks: the prep grid) */
    int split;          /* waves per wave tile of the coarse chain's trace: 1, 2, 4 */
    int coarse_waves;   /* waves per coarse bin: 1, 2, 4, 8 */
    int cull_tri;       /* coarse3_kernel's triangle-cull threshold (0 = off) */
    /* the launch's area and the overdraw thresholds, in 64-pixel units: the
     * cull's gate (od_min) and the verdict's two (od_lo: verdict 1 below it,
     * od_hi: 2 below it, 3 above) */
    unsigned long long area_units, od_min, od_lo, od_hi;
    bool feeds_overdraw;  /* prep sums the box overdraw: the launch takes an overdraw slot */
    /* the frame stores' cache policy (RT_STORE_*), in the chains whose trace
     * has one: RT_KERNEL_TRACE_BIN, RT_KERNEL_TRACE_SPLIT, RT_KERNEL_TRACE */
    int store_policy;
};

/* The store policy of a frame of `frame_bytes` bytes while the device writes
 * a working set of `working_set` bytes (track_target; a working set below the
 * frame's own size, 0 for one, means the frame alone).  `verdict`: choose()'s;
 * nearly empty frames (verdict 1) keep RT_STORE_DEFAULT. */
int store_policy_of(const Knobs& k, int64_t frame_bytes, int64_t working_set, unsigned verdict);

/* The dispatch policy.  `verdict`: the context's overdraw verdict word as the
 * caller read it (0 = none yet); `trace_mode`: the diagnostics builds' trace
 * ablation (0 = none); `working_set`: track_target()'s answer for the frame
 * this launch writes (0: the launch's own bytes).  Returns RT_OK and *out, RT_ERR_UNSUPPORTED
 * (RT_PATH_BINNED for rays the binned path cannot take) or RT_ERR_INVALID_ARG
 * (a band whose trace grid would pass 32 bits). */
int choose(const Geometry& g, const Knobs& k, int n_cu, int32_t fmt, int n_spheres, int n_cubes,
           int32_t width, int32_t rows, bool can_bin, int32_t path, unsigned verdict,
           int trace_mode, Decision* out, int64_t working_set = 0);

}  // namespace rt_dispatch

#endif /* RT_DISPATCH_H */
