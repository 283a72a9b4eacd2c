// rt_dispatch.cpp -- the render dispatcher's policy (include/rt_dispatch.h):
// the workspace layout of a binned launch, its internal bands, and choose(),
// the one statement of which kernel chain runs.  Plain C++, no HIP: the
// library links it, and tests/dispatch_check.cpp runs it on the CPU under
// -fsanitize=address,undefined.
#include "rt_dispatch.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <utility>

#include "rt_args.h"

namespace rt_dispatch {

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// coarse bins across a frame of `width` pixels
int64_t bins_x(const Geometry& g, int32_t width) { return (width + g.coarse_w - 1) / g.coarse_w; }
// coarse bin rows of `rows` rows
int64_t bins_y(const Geometry& g, int32_t rows) { return (rows + g.coarse_h - 1) / g.coarse_h; }
// rows of a coarse bin's candidate list (ids, then each tile word): the
// primitives, padded by 8 so the trace's 8-wide scalar reads stay inside the bin
int64_t list_rows(int64_t n_prims) { return (n_prims + 7) / 8 * 8 + 8; }
// bytes of one coarse bin's list
int64_t bin_list_bytes(const Geometry& g, int64_t n_prims) {
    return 4 * g.list_stride * list_rows(n_prims);
}

// The per-format selections: the coarse cull's two gates, and the highest
// overdraw verdict at which the automatic choice still takes trace_bin_kernel
// (RGBA8 frames, bound by their tests, keep the triangle cull from a lower
// overdraw on; HIT frames measured on RGBA8's side of int32x4's threshold:
// DESIGN.md §3.5).
struct FormatGates {
    int cull_tri;
    unsigned cull_overdraw;
    unsigned bin_verdict_max;
};
FormatGates gates_of(const Knobs& k, int32_t fmt) {
    if (fmt == RT_FORMAT_RGBA8) return {k.coarse_cull_tri_rgba8, k.coarse_cull_overdraw_rgba8, 1u};
    if (fmt == RT_FORMAT_HIT) return {k.coarse_cull_tri_hit, k.coarse_cull_overdraw_hit, 1u};
    return {k.coarse_cull_tri, k.coarse_cull_overdraw, 2u};
}

// The frame targets of one device's recent renders: a ring with one entry
// per render of the window, so a target written within it always has one.
struct Target {
    uintptr_t base = 0;
    int64_t bytes = 0;
    uint64_t launch = 0;  // the device's render count when last written (0: empty)
};
struct DeviceTargets {
    Target ring[kTargetWindow];
    uint64_t launches = 0;
};
std::mutex g_targets_mu;
std::map<int, DeviceTargets> g_targets;

}  // namespace

int64_t track_target(int device, const void* base, int64_t bytes) {
    std::lock_guard<std::mutex> lock(g_targets_mu);
    DeviceTargets& d = g_targets[device];
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    const uint64_t now = ++d.launches;
    // the same target again refreshes its entry; a new one takes the oldest
    Target* slot = &d.ring[0];
    for (Target& t : d.ring) {
        if (t.launch && t.base == b && t.bytes == bytes) {
            slot = &t;
            break;
        }
        if (t.launch < slot->launch) slot = &t;
    }
    *slot = Target{b, bytes, now};
    // the union of the ranges written during the window: sorted by base,
    // each range counts what lies past the end of those before it
    std::pair<uintptr_t, uintptr_t> live[kTargetWindow];
    int n = 0;
    for (const Target& t : d.ring)
        if (t.launch && now - t.launch < (uint64_t)kTargetWindow && t.bytes > 0)
            live[n++] = {t.base, t.base + (uintptr_t)t.bytes};
    std::sort(live, live + n);
    int64_t sum = 0;
    uintptr_t end = 0;
    for (int i = 0; i < n; ++i) {
        const uintptr_t from = std::max(live[i].first, end);
        if (live[i].second > from) sum += (int64_t)(live[i].second - from);
        end = std::max(end, live[i].second);
    }
    return sum;
}

void reset_targets() {
    std::lock_guard<std::mutex> lock(g_targets_mu);
    g_targets.clear();
}

int store_policy_of(const Knobs& k, int64_t frame_bytes, int64_t working_set, unsigned verdict) {
    if (k.store_policy != RT_STORE_AUTO) return k.store_policy;
    // Frames with next to nothing in them (overdraw verdict 1: the boxes cover
    // less than a frame) keep the default: nearly every wave stores at once,
    // and the written-through stores then gain nothing that holds from one
    // machine to the next (config 3's sparse scene, 2 frames in flight, 600
    // frames: 46.1 -> 46.9 us per frame on one, 43.9 -> 43.7 on another;
    // profiles/store_policy/README.md).
    return verdict != 1u && std::max(frame_bytes, working_set) >= k.store_large_bytes
               ? RT_STORE_LARGE
               : RT_STORE_DEFAULT;
}

bool use_wide_tiles(const Knobs& k, int32_t width, int32_t rows, int32_t fmt) {
    const int64_t bytes = (int64_t)width * rows * (int64_t)rt_args::pixel_bytes(fmt);
    return k.tile_variant == 2 || (k.tile_variant == 0 && bytes >= k.wide_tile_bytes);
}

Plan plan(const Geometry& g, const Knobs& k, int n_spheres, int n_cubes, int32_t width,
          int32_t rows) {
    Plan p{};
    p.n_tri = 12 * n_cubes;
    p.n_prims = p.n_tri + n_spheres;
    p.n_cx = (int)bins_x(g, width);
    p.n_cy = (int)bins_y(g, rows);
    p.n_coarse = (int64_t)p.n_cx * p.n_cy;
    p.half_cap = (int)list_rows(p.n_prims);
    p.n_chunks = (p.n_prims + g.prep_threads - 1) / g.prep_threads;
    p.use_masks = k.bin_masks && (int64_t)p.n_cx + p.n_cy <= g.mask_bins_max;
    p.tri_off = 0;
    p.sph_off = align_up((size_t)g.tri_rec_bytes * (size_t)p.n_tri, 256);
    p.box_off = p.sph_off + align_up((size_t)g.sph_rec_bytes * (size_t)n_spheres, 256);
    p.cls_off = p.box_off + align_up(16 * (size_t)p.n_prims, 256);  // int4 boxes
    p.col_off = p.cls_off + align_up((size_t)g.cls_bytes * (size_t)p.n_prims, 256);
    p.cnt_off = p.col_off + align_up(16 * (size_t)(n_cubes + n_spheres), 256);  // float4 colours
    p.mask_off = p.cnt_off + align_up(sizeof(int) * (size_t)p.n_coarse, 256);
    const size_t n_mask_words = p.use_masks ? (size_t)p.n_chunks * (size_t)(p.n_cx + p.n_cy) : 0;
    p.dep_off = p.mask_off + align_up(sizeof(unsigned long long) * n_mask_words, 256);
    p.rec_need = p.dep_off + align_up((size_t)g.tri_depth_bytes * (size_t)p.n_tri, 256);
    p.list_need = (size_t)bin_list_bytes(g, p.n_prims) * (size_t)p.n_coarse + 256;
    return p;
}

int64_t band_rows_of(const Geometry& g, const Knobs& k, int64_t n_prims, int32_t width,
                     int32_t rows) {
    const int64_t row_bytes = bin_list_bytes(g, n_prims) * bins_x(g, width);
    const int64_t n_cy = bins_y(g, rows);
    constexpr int64_t kMaxGridY = 65535;
    if (n_cy > 1 && (row_bytes * n_cy > k.list_budget || n_cy > kMaxGridY))
        return std::min<int64_t>(kMaxGridY, std::max<int64_t>(1, k.list_budget / row_bytes)) *
               g.coarse_h;
    return rows;
}

int choose(const Geometry& g, const Knobs& k, int n_cu, int32_t fmt, int n_spheres, int n_cubes,
           int32_t width, int32_t rows, bool can_bin, int32_t path, unsigned verdict,
           int trace_mode, Decision* out, int64_t working_set) {
    Decision& dc = *out;
    dc = Decision{};
    dc.band_rows = rows;
    dc.split = dc.coarse_waves = 1;
    dc.store_policy = RT_STORE_DEFAULT;
    const int store_policy = store_policy_of(
        k, (int64_t)width * rows * (int64_t)rt_args::pixel_bytes(fmt), working_set, verdict);
    if (path == RT_PATH_BINNED && !can_bin) return RT_ERR_UNSUPPORTED;
    if (!(path == RT_PATH_BINNED || (path == RT_PATH_AUTO && can_bin))) {
        dc.chain = RT_KERNEL_GENERIC;  // explicit origins / other directions: brute force
        return RT_OK;
    }
    // Bound the candidate-list workspace: bands of whole coarse rows, each a
    // band render (bin masks per band), each chosen for by itself.
    dc.band_rows = band_rows_of(g, k, 12 * (int64_t)n_cubes + n_spheres, width, rows);
    if (dc.band_rows < rows) return RT_OK;  // (chain RT_KERNEL_NONE)

    dc.plan = plan(g, k, n_spheres, n_cubes, width, rows);
    const Plan& pl = dc.plan;
    const int n_prims = pl.n_prims, n_chunks = pl.n_chunks;
    // trace: one 64-lane workgroup per wave tile; AQL grid sizes are 32-bit
    const int64_t n_tiles = pl.n_coarse * g.tiles_per_bin;
    if (n_tiles * 64 > (int64_t)UINT32_MAX) return RT_ERR_INVALID_ARG;

    // The one-kernel path preps the scene once per workgroup: it pays only
    // while the whole grid is resident at once (8 four-wave workgroups per CU
    // for one chunk, 5 for two: 28 KB of LDS each); on larger frames the
    // preps repeat for every generation of workgroups (4096^2 with 64
    // primitives: 46.9 -> 84.2 us per frame) and prep + trace_small wins.
    const int64_t fused_wgs = pl.n_coarse * (g.tiles_per_bin / g.fused_wg);
    if (n_prims > 0 && n_chunks <= g.fused_chunks && k.small_path && k.small_fused &&
        trace_mode == 0 &&
        (k.small_fused == 2 || fused_wgs <= (int64_t)n_cu * (n_chunks == 1 ? 8 : 5))) {
        dc.chain = RT_KERNEL_FRAME_SMALL;
        return RT_OK;
    }
    // small scenes: every wave tile bins itself from the bin masks
    if (n_prims > 0 && n_chunks <= g.small_chunks && pl.use_masks && k.small_path &&
        trace_mode == 0) {
        dc.chain = RT_KERNEL_TRACE_SMALL;
        return RT_OK;
    }
    // the frame's box overdraw (64-pixel units): prep adds into one of two
    // slots (alternating per launch that feeds them), coarse (or
    // trace_bin_kernel) reads it, zeroes the other for the next launch and
    // writes the verdict: 1 = below trace_bin_od10_rgba8 tenths of a frame
    // (every format takes trace_bin_kernel), 2 = below trace_bin_od10
    // (int32x4 only), 3 = above
    const FormatGates gates = gates_of(k, fmt);
    dc.area_units = ((unsigned long long)width * (unsigned long long)rows + 63ull) >> 6;
    dc.od_lo = k.trace_bin_od10_rgba8 * dc.area_units / 10;
    dc.od_hi = k.trace_bin_od10 * dc.area_units / 10;
    // Binned frames without the coarse kernel (trace_bin_kernel): frames
    // above the split-trace sizes whose last binned frame on this context
    // had a box overdraw below the format's threshold (the coarse kernel's
    // depth culls then save less than the kernel costs)
    const bool bin_ok = n_prims > 0 && n_prims <= g.bin_cap && pl.use_masks && trace_mode == 0;
    if (bin_ok && (k.trace_bin == 1 ||
                   (k.trace_bin == 0 && n_tiles > k.split2_tiles && k.trace_split == 0 &&
                    verdict >= 1u && verdict <= gates.bin_verdict_max))) {
        dc.chain = RT_KERNEL_TRACE_BIN;
        dc.feeds_overdraw = true;
        dc.store_policy = store_policy;
        return RT_OK;
    }
    if (n_prims > 0) {
        dc.feeds_overdraw = true;
        dc.od_min = gates.cull_overdraw * dc.area_units;
        // triangles join the depth cull only in bands of enough coarse bins
        // (RT_COARSE_CULL_TRI_BINS)
        dc.cull_tri = pl.n_coarse < k.coarse_cull_tri_bins ? 0 : gates.cull_tri;
        // waves per coarse bin: bands of few bins run their coarse waves as
        // one generation, each walking its bin's whole candidate list; more
        // waves per bin shorten that (rt_debug_set_coarse_waves: 0 = by band
        // size, else 1 / 2 / 4 / 8)
        dc.coarse_waves = k.coarse_waves > 0                ? k.coarse_waves
                          : pl.n_coarse <= k.coarse_w8_bins ? 8
                          : pl.n_coarse <= k.coarse_w4_bins ? 4
                          : pl.n_coarse <= k.coarse_w2_bins ? 2
                                                            : 1;
    }
    // Small frames: several waves per wave tile (trace3_split_kernel) while
    // the trace grid is a fraction of the chip's wave slots: 4 waves per tile
    // up to RT_SPLIT4_TILES tiles, 2 up to RT_SPLIT2_TILES
    // (rt_debug_set_trace_split: 0 = that choice, 1 = never, 2 / 4 = always);
    // the diagnostics' trace ablations exist for trace3_kernel only
    dc.split = trace_mode != 0             ? 1
               : k.trace_split > 0         ? k.trace_split
               : n_tiles <= k.split4_tiles ? 4
               : n_tiles <= k.split2_tiles ? 2
                                           : 1;
    dc.chain = dc.split > 1 ? RT_KERNEL_TRACE_SPLIT : RT_KERNEL_TRACE;
    dc.store_policy = store_policy;
    return RT_OK;
}

}  // namespace rt_dispatch
