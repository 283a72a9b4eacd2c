// dispatch_check.cpp -- the render dispatcher's policy (csrc/rt_dispatch.cpp)
// on the CPU, as a stand-alone program like tests/hit_args_check.cpp:
// tests/test_dispatch.py builds it with -fsanitize=address,undefined next to
// rt_dispatch.cpp and rt_args.cpp and runs it.  No GPU, no HIP.
//
// Every expected value is a literal, worked out by hand from the rules (bins =
// ceil(width / bin width) x ceil(rows / bin height), tiles = 16 x bins, ...);
// none is computed by calling the code under test a second way.
//   - which chain runs: split and coarse waves by frame size, the fused
//     path's residency rule, the small path, trace_bin_kernel's choice over
//     every knob value x verdict x format, the cull gates, the generic path,
//     the six rows of tests/test_gpu_parity.py's
//     test_last_kernel_names_the_path_taken;
//   - the workspace plan's byte counts and the internal bands, and that the
//     plan rt_reserve sizes is the plan launch() gets for the same band.
// Exit 0 and "dispatch check ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "rt_dispatch.h"
#include "rt_hip.h"

namespace {

using rt_dispatch::Decision;
using rt_dispatch::Geometry;
using rt_dispatch::Knobs;
using rt_dispatch::Plan;

int failures = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, \
                         #cond);                                                 \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

// The two tile builds (rt_trace.inc's kGeometry): 16x16 tiles in 64x64 bins,
// 128x2 tiles in 128x32 bins; 16 tiles per bin and two list words per
// candidate in both.
const Geometry G16{64, 64, 16, 2, 64, 4, 2, 8, 1024, 4096, 128, 32, 32, 48};
const Geometry GWIDE{128, 32, 16, 2, 64, 4, 2, 8, 1024, 4096, 128, 32, 32, 48};

// One question to choose(); the defaults are an automatic int32x4 render of
// a binnable direction on a 256-CU device, no verdict yet.
struct Q {
    const Geometry* g = &G16;
    Knobs k;
    int n_cu = 256;
    int32_t fmt = RT_FORMAT_I32X4;
    int ns = 0, nc = 0;  // spheres, cubes (12 triangles each)
    int32_t w = 0, h = 0;
    bool can_bin = true;
    int32_t path = RT_PATH_AUTO;
    unsigned verdict = 0;
    int trace_mode = 0;
};

Q frame(int ns, int nc, int32_t w, int32_t h, const Geometry* g = &G16) {
    Q q;
    q.g = g;
    q.ns = ns;
    q.nc = nc;
    q.w = w;
    q.h = h;
    return q;
}

int ask(const Q& q, Decision* dc) {
    return rt_dispatch::choose(*q.g, q.k, q.n_cu, q.fmt, q.ns, q.nc, q.w, q.h, q.can_bin, q.path,
                               q.verdict, q.trace_mode, dc);
}

// the chain of a question that must succeed
int chain(const Q& q) {
    Decision dc;
    const int rc = ask(q, &dc);
    CHECK(rc == RT_OK);
    return rc == RT_OK ? dc.chain : -1;
}

// rt_last_kernel's names (the Python package's KERNEL_NAMES)
const char* name_of(int kernel) {
    switch (kernel) {
    case RT_KERNEL_TRACE: return "trace3_kernel";
    case RT_KERNEL_TRACE_SMALL: return "trace_small_kernel";
    case RT_KERNEL_FRAME_SMALL: return "frame_small_kernel";
    case RT_KERNEL_GENERIC: return "generic_kernel";
    case RT_KERNEL_TRACE_SPLIT: return "trace3_split_kernel";
    case RT_KERNEL_TRACE_BIN: return "trace_bin_kernel";
    default: return "none";
    }
}
bool runs(const Q& q, const char* kernel) { return std::strcmp(name_of(chain(q)), kernel) == 0; }

// 256 spheres + 64 cubes: 1024 primitives, 16 prep chunks -- past the small
// paths, still within trace_bin_kernel's reach
constexpr int NS = 256, NC = 64;

void split_waves() {
    struct Row {
        int32_t w, h;
        int64_t bins16, bins_wide;
        int split, kernel;
    };
    // 64x64 bins: 16x8, 16x9, 16x16, 17x16; 128x32 bins: 8x16, 8x18, 8x32, 9x32
    const Row rows[] = {{1024, 512, 128, 128, 4, RT_KERNEL_TRACE_SPLIT},
                        {1024, 576, 144, 144, 2, RT_KERNEL_TRACE_SPLIT},
                        {1024, 1024, 256, 256, 2, RT_KERNEL_TRACE_SPLIT},
                        {1088, 1024, 272, 288, 1, RT_KERNEL_TRACE}};
    for (const Row& r : rows) {
        for (const Geometry* g : {&G16, &GWIDE}) {
            Decision dc;
            Q q = frame(NS, NC, r.w, r.h, g);
            CHECK(ask(q, &dc) == RT_OK);
            CHECK(dc.plan.n_coarse == (g == &G16 ? r.bins16 : r.bins_wide));
            CHECK(dc.split == r.split && dc.chain == r.kernel);
            CHECK(dc.band_rows == r.h && dc.feeds_overdraw);
            // rt_debug_set_trace_split overrides the frame size
            for (int forced : {1, 2, 4}) {
                q.k.trace_split = forced;
                CHECK(ask(q, &dc) == RT_OK && dc.split == forced);
                CHECK(dc.chain == (forced == 1 ? RT_KERNEL_TRACE : RT_KERNEL_TRACE_SPLIT));
            }
        }
    }
    // the diagnostics' trace ablations exist for trace3_kernel only
    Q q = frame(NS, NC, 1024, 512);
    q.trace_mode = 1;
    Decision dc;
    CHECK(ask(q, &dc) == RT_OK && dc.chain == RT_KERNEL_TRACE && dc.split == 1);
}

void coarse_waves() {
    struct Row {
        int32_t w, h;
        int64_t bins;
        int waves;
    };
    // 16x16, 257x1, 32x32 and 25x41 bins of 64x64
    const Row rows[] = {{1024, 1024, 256, 8}, {16448, 64, 257, 4}, {2048, 2048, 1024, 4},
                        {1600, 2624, 1025, 1}};
    for (const Row& r : rows) {
        Decision dc;
        Q q = frame(NS, NC, r.w, r.h);
        CHECK(ask(q, &dc) == RT_OK);
        CHECK(dc.plan.n_coarse == r.bins && dc.coarse_waves == r.waves);
        for (int forced : {1, 2, 4, 8}) {
            q.k.coarse_waves = forced;
            CHECK(ask(q, &dc) == RT_OK && dc.coarse_waves == forced);
        }
    }
}

void fused_residency() {
    // one chunk (16 spheres + 4 cubes = 64 primitives): 4 workgroups per bin,
    // 8 per CU resident: 256 x 8 = 2048 workgroups = 512 bins
    CHECK(chain(frame(16, 4, 1920, 1080)) == RT_KERNEL_FRAME_SMALL);  // 30x17 = 510 bins
    CHECK(chain(frame(16, 4, 2048, 1024)) == RT_KERNEL_FRAME_SMALL);  // 32x16 = 512
    CHECK(chain(frame(16, 4, 1728, 1216)) == RT_KERNEL_TRACE_SMALL);  // 27x19 = 513
    CHECK(chain(frame(16, 4, 1024, 2048, &GWIDE)) == RT_KERNEL_FRAME_SMALL);  // 8x64 = 512
    CHECK(chain(frame(16, 4, 1152, 1824, &GWIDE)) == RT_KERNEL_TRACE_SMALL);  // 9x57 = 513
    // two chunks (65 to 128 primitives): 5 per CU, 1280 workgroups = 320 bins
    CHECK(chain(frame(5, 5, 1280, 1024)) == RT_KERNEL_FRAME_SMALL);  // 65 primitives, 20x16
    CHECK(chain(frame(8, 10, 1280, 1024)) == RT_KERNEL_FRAME_SMALL);  // 128 primitives
    CHECK(chain(frame(5, 5, 6848, 192)) == RT_KERNEL_TRACE_SMALL);  // 107x3 = 321 bins
    CHECK(chain(frame(8, 10, 6848, 192)) == RT_KERNEL_TRACE_SMALL);
    // fewer CUs, fewer resident workgroups: 128 x 8 = 1024 = 256 bins
    Q q = frame(16, 4, 1024, 1024);  // 256 bins
    q.n_cu = 128;
    CHECK(chain(q) == RT_KERNEL_FRAME_SMALL);
    q.w = 1088;  // 17x16 = 272
    CHECK(chain(q) == RT_KERNEL_TRACE_SMALL);
    // rt_debug_set_small_fused: 2 = on every frame size, 0 = never
    q = frame(16, 4, 4096, 4096);
    CHECK(chain(q) == RT_KERNEL_TRACE_SMALL);
    q.k.small_fused = 2;
    CHECK(chain(q) == RT_KERNEL_FRAME_SMALL);
    q = frame(16, 4, 1920, 1080);
    q.k.small_fused = 0;
    CHECK(chain(q) == RT_KERNEL_TRACE_SMALL);
    // 129 primitives are three chunks: never fused
    q = frame(9, 10, 640, 480);
    CHECK(chain(q) == RT_KERNEL_TRACE_SMALL);
    q.k.small_fused = 2;
    CHECK(chain(q) == RT_KERNEL_TRACE_SMALL);
    // rt_debug_set_small_path(0) turns both off
    q = frame(16, 4, 640, 480);  // 10x8 bins, 1280 tiles
    q.k.small_path = false;
    CHECK(chain(q) == RT_KERNEL_TRACE_SPLIT);
    // a trace ablation takes the coarse chain's trace3_kernel
    q = frame(16, 4, 640, 480);
    q.trace_mode = 3;
    CHECK(chain(q) == RT_KERNEL_TRACE);
}

void small_path() {
    // 32 spheres + 40 cubes = 512 primitives = 8 chunks; 4096x1024 is 64x16 bins
    CHECK(chain(frame(32, 40, 4096, 1024)) == RT_KERNEL_TRACE_SMALL);
    CHECK(chain(frame(33, 40, 4096, 1024)) == RT_KERNEL_TRACE);  // 513: nine chunks
    Q q = frame(32, 40, 4096, 1024);
    q.k.bin_masks = false;
    CHECK(chain(q) == RT_KERNEL_TRACE);
    // bin masks hold up to 4096 bin rows + columns: 4095 + 1, then 4096 + 1
    CHECK(chain(frame(32, 40, 262080, 64)) == RT_KERNEL_TRACE_SMALL);
    CHECK(chain(frame(32, 40, 262144, 64)) == RT_KERNEL_TRACE);
    Decision dc;
    CHECK(ask(frame(32, 40, 262144, 64), &dc) == RT_OK && !dc.plan.use_masks);
    CHECK(ask(frame(32, 40, 262080, 64), &dc) == RT_OK && dc.plan.use_masks);
}

void self_binning() {
    const int BIN = RT_KERNEL_TRACE_BIN, TR = RT_KERNEL_TRACE, SP = RT_KERNEL_TRACE_SPLIT;
    const int32_t fmts[3] = {RT_FORMAT_I32X4, RT_FORMAT_RGBA8, RT_FORMAT_HIT};
    // 2048x2048: 1024 bins, 16384 tiles.  [trace_bin][verdict][format]
    const int big[3][4][3] = {
        // 0 = automatic: verdict 1 in every format, verdict 2 in int32x4 alone
        {{TR, TR, TR}, {BIN, BIN, BIN}, {BIN, TR, TR}, {TR, TR, TR}},
        // 1 = always
        {{BIN, BIN, BIN}, {BIN, BIN, BIN}, {BIN, BIN, BIN}, {BIN, BIN, BIN}},
        // 2 = never
        {{TR, TR, TR}, {TR, TR, TR}, {TR, TR, TR}, {TR, TR, TR}}};
    // 1024x1024: 256 bins, exactly 4096 tiles -- not above the split sizes, so
    // never by itself; the coarse chain there is the two-wave split trace
    const int at4096[3][4][3] = {
        {{SP, SP, SP}, {SP, SP, SP}, {SP, SP, SP}, {SP, SP, SP}},
        {{BIN, BIN, BIN}, {BIN, BIN, BIN}, {BIN, BIN, BIN}, {BIN, BIN, BIN}},
        {{SP, SP, SP}, {SP, SP, SP}, {SP, SP, SP}, {SP, SP, SP}}};
    for (int tb = 0; tb < 3; ++tb)
        for (unsigned v = 0; v < 4; ++v)
            for (int f = 0; f < 3; ++f) {
                Q q = frame(NS, NC, 2048, 2048);
                q.k.trace_bin = tb;
                q.verdict = v;
                q.fmt = fmts[f];
                CHECK(chain(q) == big[tb][v][f]);
                q.w = q.h = 1024;
                CHECK(chain(q) == at4096[tb][v][f]);
                q.g = &GWIDE;  // 8x32 bins: 4096 tiles too
                CHECK(chain(q) == at4096[tb][v][f]);
            }
    // scenes of at most 1024 primitives
    Q q = frame(NS, NC, 2048, 2048);
    q.k.trace_bin = 1;
    CHECK(chain(q) == BIN);
    q.ns = NS + 1;
    CHECK(chain(q) == TR);
    // ... and only with bin masks
    q = frame(NS, NC, 2048, 2048);
    q.k.trace_bin = 1;
    q.k.bin_masks = false;
    CHECK(chain(q) == TR);
    // a forced split vetoes the automatic choice, not the forced one
    for (int forced : {1, 2, 4}) {
        q = frame(NS, NC, 2048, 2048);
        q.verdict = 1;
        CHECK(chain(q) == BIN);
        q.k.trace_split = forced;
        CHECK(chain(q) == (forced == 1 ? TR : SP));
        q.k.trace_bin = 1;
        CHECK(chain(q) == BIN);
    }
    // a trace ablation vetoes both
    q = frame(NS, NC, 2048, 2048);
    q.verdict = 1;
    q.trace_mode = 2;
    CHECK(chain(q) == TR);
    q.k.trace_bin = 1;
    CHECK(chain(q) == TR);
    // the launch feeds the overdraw slots and carries the verdict's thresholds
    q = frame(NS, NC, 2048, 2048);
    q.k.trace_bin = 1;
    Decision dc;
    CHECK(ask(q, &dc) == RT_OK && dc.feeds_overdraw);
    CHECK(dc.area_units == 65536 && dc.od_lo == 65536 && dc.od_hi == 262144);
}

void cull_gates() {
    const int32_t fmts[3] = {RT_FORMAT_I32X4, RT_FORMAT_RGBA8, RT_FORMAT_HIT};
    const int tri_at_768[3] = {4, 2, 2};
    Decision dc;
    for (int f = 0; f < 3; ++f) {
        Q q = frame(NS, NC, 832, 3776);  // 13x59 = 767 bins
        q.fmt = fmts[f];
        CHECK(ask(q, &dc) == RT_OK && dc.plan.n_coarse == 767 && dc.cull_tri == 0);
        q.w = 2048, q.h = 1536;  // 32x24 = 768
        CHECK(ask(q, &dc) == RT_OK && dc.plan.n_coarse == 768 && dc.cull_tri == tri_at_768[f]);
        // rt_debug_set_coarse_cull_tri(7): one value for every format
        q.k.coarse_cull_tri = q.k.coarse_cull_tri_rgba8 = q.k.coarse_cull_tri_hit = 7;
        CHECK(ask(q, &dc) == RT_OK && dc.cull_tri == 7);
        // rt_debug_set_coarse_cull_overdraw(3): the gate in every format and
        // no floor on the band's bins
        q = frame(NS, NC, 832, 3776);
        q.fmt = fmts[f];
        q.k.coarse_cull_overdraw = q.k.coarse_cull_overdraw_rgba8 = q.k.coarse_cull_overdraw_hit = 3;
        q.k.coarse_cull_tri_bins = 0;
        CHECK(ask(q, &dc) == RT_OK && dc.cull_tri == tri_at_768[f]);
        CHECK(dc.area_units == 49088 && dc.od_min == 147264);  // 832 x 3776 / 64 = 49088
    }
    // 1001 x 999 = 999999 pixels: 15625 units of 64 (rounded up)
    const unsigned long long od_min[3] = {78125, 0, 31250};  // 5, 0 and 2 frames
    for (int f = 0; f < 3; ++f) {
        Q q = frame(NS, NC, 1001, 999);
        q.fmt = fmts[f];
        CHECK(ask(q, &dc) == RT_OK && dc.chain == RT_KERNEL_TRACE_SPLIT);
        CHECK(dc.area_units == 15625 && dc.od_min == od_min[f]);
        CHECK(dc.od_lo == 15625 && dc.od_hi == 62500);  // 1.0 and 4.0 frames
        CHECK(dc.feeds_overdraw && dc.cull_tri == 0 && dc.coarse_waves == 8 && dc.split == 2);
    }
}

void generic_and_empty() {
    Decision dc;
    Q q = frame(8, 2, 256, 128);
    q.can_bin = false;
    q.path = RT_PATH_BINNED;
    CHECK(ask(q, &dc) == RT_ERR_UNSUPPORTED);
    q.path = RT_PATH_AUTO;
    CHECK(ask(q, &dc) == RT_OK && dc.chain == RT_KERNEL_GENERIC && dc.band_rows == 128);
    q.path = RT_PATH_GENERIC;
    CHECK(chain(q) == RT_KERNEL_GENERIC);
    q.can_bin = true;
    CHECK(chain(q) == RT_KERNEL_GENERIC);
    q.path = RT_PATH_BINNED;
    CHECK(chain(q) == RT_KERNEL_FRAME_SMALL);
    // a generic frame is never split into bands
    q = frame(NS, NC, 1920, 1080);
    q.path = RT_PATH_GENERIC;
    q.k.list_budget = 1000;
    CHECK(ask(q, &dc) == RT_OK && dc.chain == RT_KERNEL_GENERIC && dc.band_rows == 1080);
    // no primitives: the coarse chain's trace over empty lists, no prep, no coarse
    q = frame(0, 0, 640, 480);  // 10x8 bins, 1280 tiles
    CHECK(ask(q, &dc) == RT_OK && dc.chain == RT_KERNEL_TRACE_SPLIT && dc.split == 4);
    CHECK(!dc.feeds_overdraw && dc.plan.n_prims == 0 && dc.plan.n_chunks == 0);
    q.k.trace_bin = 1;
    q.k.small_fused = 2;
    CHECK(chain(q) == RT_KERNEL_TRACE_SPLIT);
    CHECK(chain(frame(0, 0, 2048, 2048)) == RT_KERNEL_TRACE);
    // the trace grid counts lanes in 32 bits: 64 lanes x 16 tiles x bins, so
    // 2047 x 2048 bins pass and 2048 x 2048 do not
    CHECK(ask(frame(0, 0, 131008, 131072), &dc) == RT_OK && dc.chain == RT_KERNEL_TRACE);
    CHECK(dc.plan.n_coarse == 4192256);
    CHECK(ask(frame(0, 0, 131072, 131072), &dc) == RT_ERR_INVALID_ARG);
}

// The rows of tests/test_gpu_parity.py::test_last_kernel_names_the_path_taken
// (its scenes are synthetic(w, h, spheres, cubes); "bin" forces trace_bin_kernel
// on, every other row forces it off).
void gpu_suite_rows() {
    struct Row {
        int ns, nc;
        int32_t w, h;
        const char* path;
        const char* kernel;
    };
    const Row rows[] = {{16, 4, 1920, 1080, "auto", "frame_small_kernel"},
                        {100, 30, 4096, 1024, "auto", "trace_small_kernel"},
                        {256, 64, 1024, 1024, "auto", "trace3_split_kernel"},
                        {256, 64, 2048, 2048, "auto", "trace3_kernel"},
                        {256, 64, 2048, 2048, "bin", "trace_bin_kernel"},
                        {8, 2, 256, 128, "generic", "generic_kernel"}};
    for (const Row& r : rows) {
        Q q = frame(r.ns, r.nc, r.w, r.h);
        q.k.trace_bin = std::strcmp(r.path, "bin") == 0 ? 1 : 2;
        q.path = std::strcmp(r.path, "generic") == 0 ? RT_PATH_GENERIC : RT_PATH_AUTO;
        CHECK(runs(q, r.kernel));
    }
}

bool same_plan(const Plan& a, const Plan& b) {
    return a.n_tri == b.n_tri && a.n_prims == b.n_prims && a.n_cx == b.n_cx && a.n_cy == b.n_cy &&
           a.n_chunks == b.n_chunks && a.half_cap == b.half_cap && a.n_coarse == b.n_coarse &&
           a.use_masks == b.use_masks && a.tri_off == b.tri_off && a.sph_off == b.sph_off &&
           a.box_off == b.box_off && a.cls_off == b.cls_off && a.col_off == b.col_off &&
           a.cnt_off == b.cnt_off && a.mask_off == b.mask_off && a.dep_off == b.dep_off &&
           a.rec_need == b.rec_need && a.list_need == b.list_need;
}

void plans_and_bands() {
    // Scene A: 256 spheres + 64 cubes: 768 triangles, 1024 primitives, 16
    // chunks, 1032 list rows.  Records: TriRec 98304, SphRec 8192, boxes 16384,
    // Cls 32768, colours 5120 -> counts at 160768; TriDepth 36864.
    // Scene B: 3 spheres + 2 cubes: 24 triangles, 27 primitives, one chunk, 40
    // list rows.  3072, 96 -> 256, 432 -> 512, 864 -> 1024, 80 -> 256 -> counts
    // at 5120; TriDepth 1152 -> 1280.
    // Frames: 1920x1080 = 30x17 (64x64) or 15x34 (128x32) = 510 bins: counts
    // 2040 -> 2048; 1000x700 = 16x11 or 8x22 = 176 bins: counts 704 -> 768.
    // Masks: 8 B x chunks x (bin rows + columns), rounded up to 256.
    // Lists: 4 B x 2 x list rows x bins + 256.
    struct Row {
        const Geometry* g;
        int ns, nc;
        int32_t w, h;
        int n_cx, n_cy;
        size_t cnt_off, mask_off, dep_off, rec_need, list_need;
    };
    const Row rows[] = {
        {&G16, 256, 64, 1920, 1080, 30, 17, 160768, 162816, 168960, 205824, 4210816},
        {&GWIDE, 256, 64, 1920, 1080, 15, 34, 160768, 162816, 169216, 206080, 4210816},
        {&G16, 256, 64, 1000, 700, 16, 11, 160768, 161536, 165120, 201984, 1453312},
        {&GWIDE, 256, 64, 1000, 700, 8, 22, 160768, 161536, 165376, 202240, 1453312},
        {&G16, 3, 2, 1920, 1080, 30, 17, 5120, 7168, 7680, 8960, 163456},
        {&GWIDE, 3, 2, 1920, 1080, 15, 34, 5120, 7168, 7680, 8960, 163456},
        {&G16, 3, 2, 1000, 700, 16, 11, 5120, 5888, 6144, 7424, 56576},
        {&GWIDE, 3, 2, 1000, 700, 8, 22, 5120, 5888, 6144, 7424, 56576}};
    const Knobs defaults;
    for (const Row& r : rows) {
        const Plan p = rt_dispatch::plan(*r.g, defaults, r.ns, r.nc, r.w, r.h);
        CHECK(p.n_tri == 12 * r.nc && p.n_prims == 12 * r.nc + r.ns);
        CHECK(p.n_cx == r.n_cx && p.n_cy == r.n_cy && p.n_coarse == (int64_t)r.n_cx * r.n_cy);
        CHECK(p.n_chunks == (r.ns == 256 ? 16 : 1) && p.half_cap == (r.ns == 256 ? 1032 : 40));
        CHECK(p.use_masks);
        CHECK(p.cnt_off == r.cnt_off && p.mask_off == r.mask_off && p.dep_off == r.dep_off);
        CHECK(p.rec_need == r.rec_need && p.list_need == r.list_need);
        const size_t offs[] = {p.tri_off, p.sph_off, p.box_off, p.cls_off, p.col_off,
                               p.cnt_off, p.mask_off, p.dep_off, p.rec_need};
        CHECK(offs[0] == 0);
        for (int i = 0; i < 9; ++i) CHECK(offs[i] % 256 == 0);
        for (int i = 1; i < 9; ++i) CHECK(offs[i] > offs[i - 1]);
        // without bin masks nothing is set aside for them
        Knobs no_masks;
        no_masks.bin_masks = false;
        const Plan q = rt_dispatch::plan(*r.g, no_masks, r.ns, r.nc, r.w, r.h);
        CHECK(!q.use_masks && q.dep_off == q.mask_off && q.mask_off == p.mask_off);

        // what launch() gets is what rt_reserve sized: for the whole frame ...
        Decision dc;
        Q ql = frame(r.ns, r.nc, r.w, r.h, r.g);
        CHECK(rt_dispatch::band_rows_of(*r.g, defaults, p.n_prims, r.w, r.h) == r.h);
        CHECK(ask(ql, &dc) == RT_OK && dc.band_rows == r.h && same_plan(dc.plan, p));
    }

    // Bands.  Scene A at 1920x1080: a bin's list is 4 x 2 x 1032 = 8256 B, a
    // bin row 30 x 8256 = 247680 B (64x64 bins) or 15 x 8256 = 123840 B
    // (128x32); a budget of 1000000 B holds 4 / 8 bin rows: 256 rows each way,
    // 120 bins, 990720 B of lists.
    for (const Geometry* g : {&G16, &GWIDE}) {
        Knobs k;
        k.list_budget = 1000000;  // (rt_debug_set_list_budget)
        const int64_t per = rt_dispatch::band_rows_of(*g, k, 1024, 1920, 1080);
        CHECK(per == 256 && per % g->coarse_h == 0);
        const Plan band = rt_dispatch::plan(*g, k, NS, NC, 1920, (int32_t)per);
        CHECK(band.n_coarse == 120 && band.list_need == 990976);
        CHECK(band.list_need <= (size_t)k.list_budget + 256);
        // launch(): the frame is split, and each band's own decision carries
        // the plan reserve() sized -- the last band (1080 - 4 x 256 = 56 rows) a smaller one
        Q q = frame(NS, NC, 1920, 1080, g);
        q.k = k;
        Decision dc;
        CHECK(ask(q, &dc) == RT_OK && dc.chain == RT_KERNEL_NONE && dc.band_rows == 256);
        q.h = 256;
        CHECK(ask(q, &dc) == RT_OK && dc.band_rows == 256 && same_plan(dc.plan, band));
        CHECK(dc.chain == RT_KERNEL_TRACE_SPLIT && dc.split == 4);  // 120 bins, 1920 tiles
        q.h = 56;
        CHECK(ask(q, &dc) == RT_OK && dc.band_rows == 56);
        CHECK(dc.plan.list_need <= band.list_need && dc.plan.rec_need <= band.rec_need);
        // a budget below one bin row still renders one bin row at a time
        k.list_budget = 1000;
        CHECK(rt_dispatch::band_rows_of(*g, k, 1024, 1920, 1080) == g->coarse_h);
        // one bin row is never split
        CHECK(rt_dispatch::band_rows_of(*g, k, 1024, 1920, g->coarse_h) == g->coarse_h);
    }
    // more than 65535 bin rows (the trace grid's y) force bands of 65535
    const Knobs k;
    CHECK(rt_dispatch::band_rows_of(G16, k, 27, 64, 65535 * 64) == 65535 * 64);
    CHECK(rt_dispatch::band_rows_of(G16, k, 27, 64, 65536 * 64) == 4194240);
    CHECK(rt_dispatch::band_rows_of(GWIDE, k, 27, 128, 65536 * 32) == 2097120);
    // the default budget of 4 GiB: config 3's 4096x4096 (64x64 bins of 8256 B:
    // 33.8 MB) is one band
    CHECK(rt_dispatch::band_rows_of(G16, k, 1024, 4096, 4096) == 4096);
}

void tile_variant() {
    Knobs k;
    // 512 MiB frames and larger take the wide tiles: 8192 x 4096 x 16 B
    CHECK(rt_dispatch::use_wide_tiles(k, 8192, 4096, RT_FORMAT_I32X4));
    CHECK(!rt_dispatch::use_wide_tiles(k, 8192, 4095, RT_FORMAT_I32X4));
    CHECK(!rt_dispatch::use_wide_tiles(k, 8192, 4096, RT_FORMAT_HIT));
    CHECK(rt_dispatch::use_wide_tiles(k, 8192, 8192, RT_FORMAT_HIT));
    CHECK(rt_dispatch::use_wide_tiles(k, 16384, 8192, RT_FORMAT_RGBA8));
    k.tile_variant = 1;
    CHECK(!rt_dispatch::use_wide_tiles(k, 8192, 4096, RT_FORMAT_I32X4));
    k.tile_variant = 2;
    CHECK(rt_dispatch::use_wide_tiles(k, 64, 64, RT_FORMAT_RGBA8));
}

void defaults() {
    const Knobs k;
    CHECK(k.list_budget == (int64_t)4 << 30 && k.bin_masks && k.small_path && k.small_fused == 1);
    CHECK(k.trace_split == 0 && k.coarse_waves == 0 && k.trace_bin == 0 && k.tile_variant == 0);
    CHECK(k.coarse_cull == 10 && k.coarse_cull_tri == 4 && k.coarse_cull_tri_rgba8 == 2 &&
          k.coarse_cull_tri_hit == 2);
    CHECK(k.coarse_cull_overdraw == 5 && k.coarse_cull_overdraw_rgba8 == 0 &&
          k.coarse_cull_overdraw_hit == 2 && k.coarse_cull_tri_bins == 768);
    CHECK(k.split4_tiles == 2048 && k.split2_tiles == 4096);
    CHECK(k.coarse_w8_bins == 256 && k.coarse_w4_bins == 1024 && k.coarse_w2_bins == 1024);
    CHECK(k.trace_bin_od10 == 40 && k.trace_bin_od10_rgba8 == 10);
    CHECK(k.wide_tile_bytes == (int64_t)1 << 29);
}

}  // namespace

int main() {
    defaults();
    split_waves();
    coarse_waves();
    fused_residency();
    small_path();
    self_binning();
    cull_gates();
    generic_and_empty();
    gpu_suite_rows();
    plans_and_bands();
    tile_variant();
    if (failures) return 1;
    std::printf("dispatch check ok\n");
    return 0;
}
