// rt_trace.inc -- the tile-shape-dependent half of librt_hip.so: every
// kernel of the binned and generic paths and the host launch() that
// enqueues them.  Included twice by rt_device.hip, once per wave-tile width
// (RT_TILE_W = 16: 16x16 tiles; 128: 128x2 tiles), each in its own namespace;
// rt_device.hip picks one per frame.  Not a standalone translation unit.
//
// Kernels (DESIGN.md §3): six chains, listed at rt_dispatch::Decision
// (include/rt_dispatch.h); which one a frame takes, by scene and frame size,
// is rt_dispatch::choose() (csrc/rt_dispatch.cpp), the one statement of the
// rules.  launch() below enqueues what it returns.
// Every pixel-writing kernel exists per output format (kFmt): int32x4, the
// Texture's RGBA8 word, or RT_FORMAT_HIT (rt_hit: the walk's closest and
// colour slot, unshaded).

// Compile-time experiments that were measured, decided and removed
// (DESIGN.md §3.5).  A stale recipe passing one of them must not silently
// build, and "measure", the default.
#if defined(RT_WALK_BALLOT) || defined(RT_WALK_BALLOT_SPLIT) || defined(RT_BIN_ABLATE) ||    \
    defined(RT_EXTRA_VALU) || defined(RT_EXTRA_SALU) || defined(RT_REC_U32) ||               \
    defined(RT_PREP_TRIDEPTH) || defined(RT_PREP_OVERDRAW) || defined(RT_DEPTH_CULL)
#error "RT_WALK_BALLOT, RT_WALK_BALLOT_SPLIT, RT_BIN_ABLATE, RT_EXTRA_VALU, RT_EXTRA_SALU, RT_REC_U32, RT_PREP_TRIDEPTH, RT_PREP_OVERDRAW and RT_DEPTH_CULL were decided and removed (DESIGN.md §3.5); their code is in history, last at commit 9cad428"
#endif
#if defined(RT_RECOMPUTE_XY) || defined(RT_ROW_GROUP)
#error "RT_RECOMPUTE_XY and RT_ROW_GROUP (the 8-rows-per-lane trace3_kernel) were decided and removed (DESIGN.md §3.5); their code is in history, last at commit 96b3fb5"
#endif
namespace {

// Build-time geometry / feature knobs (A/B variants: scripts/variants.sh).
#ifndef RT_TILE_W
#define RT_TILE_W 16              // wave tile width (lanes per row); 8 (8x32 tiles) measured
                                  // 1.9 us per frame slower at config 3 (DESIGN.md)
#endif
#ifndef RT_ROWS
#define RT_ROWS 4                 // pixels per lane (rows, 64/RT_TILE_W apart)
#endif
#ifndef RT_TRACE_WAVES
#define RT_TRACE_WAVES 8          // amdgpu_waves_per_eu floor for trace (0 = none)
#endif
#ifndef RT_TIMELINE
#define RT_TIMELINE 0             // diagnostics: per-wave phase timestamps
#endif
// A wave tile is kLaneRows lane rows of kLanesX lanes; a lane's kRowsPerLane
// pixels step kStepsX times along x (kLanesX apart), then down (kLaneRows
// apart).  RT_TILE_W <= 64: one pixel column per lane (16x16, 64x4 tiles);
// RT_TILE_W = 128: 128x2 tiles, a lane's 4 pixels 2 along x (64 apart) in 2
// rows; RT_TILE_W = 256: 256x1 tiles, a lane's 4 pixels 64 apart in one row.
constexpr int kWaveTile = RT_TILE_W;                       // wave tile width
constexpr int kRowsPerLane = RT_ROWS;                      // pixels per lane
constexpr int kLanesX = RT_TILE_W < 64 ? RT_TILE_W : 64;   // lanes along x
constexpr int kStepsX = RT_TILE_W / kLanesX;               // a lane's pixels along x
constexpr int kLaneRows = 64 / kLanesX;                    // lane rows
constexpr int kWaveTileH = kLaneRows * (RT_ROWS / kStepsX);  // wave tile height
static_assert(RT_ROWS % kStepsX == 0, "tile geometry");
// pixel j of a lane: (lane % kLanesX + pix_dx(j), lane / kLanesX + pix_dy(j))
__host__ __device__ constexpr int pix_dx(int j) { return kLanesX * (j % kStepsX); }
__host__ __device__ constexpr int pix_dy(int j) { return kLaneRows * (j / kStepsX); }
// coarse bin (candidate list) size, pixels: 64x64, or one tile wide
#ifdef RT_COARSE_W
constexpr int kCoarseW = RT_COARSE_W;
#else
constexpr int kCoarseW = RT_TILE_W > 64 ? RT_TILE_W : 64;
#endif
#ifdef RT_COARSE_H
constexpr int kCoarseH = RT_COARSE_H;
#else
constexpr int kCoarseH = RT_TILE_W > 64 ? 4096 / RT_TILE_W : 64;
#endif
static_assert(kCoarseW % kWaveTile == 0 && kCoarseH % kWaveTileH == 0,
              "wave tiles must tile a coarse bin");
// prep_triangle's classifier margin covers tiles that overhang a box by up to
// kTileSpan pixels on any side
constexpr int kTileSpan = kWaveTile > kWaveTileH ? kWaveTile : kWaveTileH;
static_assert(kTileSpan <= 256, "tile span");
// Row blocks: the classifier's unit inside a wave tile.  Lane row j of a
// tile covers pixel rows tile_y + kLaneRows * j + [0, kLaneRows), i.e. one
// kWaveTile x kLaneRows block per j, so a per-block verdict (skip / test /
// u,v proven inside) is wave-uniform for each of a lane's rows.
// RT_ROWBITS 0 (default) classifies whole tiles (one block of kWaveTileH
// rows); 1 also classifies the row blocks of a triangle's partial tiles
// (measured slower: the trace saves 1.1 us, coarse pays 3.7 us; DESIGN.md).
#ifndef RT_ROWBITS
#define RT_ROWBITS 0
#endif
constexpr int kBlocks = RT_ROWBITS ? kRowsPerLane : 1;   // blocks per wave tile
static_assert(kBlocks == 1 || kStepsX == 1, "row blocks need one pixel column per lane");
constexpr int kBlockH = kWaveTileH / kBlocks;             // rows per block
constexpr int kTileBits = 2 * kBlocks;                    // bit 2b keep, 2b+1 inside
constexpr int kTilesPerWord = 32 / kTileBits;
constexpr unsigned kTileMask = kTileBits == 32 ? ~0u : (1u << kTileBits) - 1u;
constexpr unsigned kKeepMask = 0x55555555u & kTileMask;
static_assert(kBlockH * kBlocks == kWaveTileH && kTileBits <= 32, "row blocks");
// the block of lane row j
__host__ __device__ constexpr int row_block(int j) { return j * kBlocks / kRowsPerLane; }

constexpr int kThreads = 256;       // generic_kernel block
constexpr int kPrepThreads = 64;  // prep: one wave per block, spread over CUs
// Separable bin masks: a box overlaps a coarse bin iff it overlaps the bin's
// row of bins and its column of bins, so prep publishes, per bin row and per
// bin column, one 64-bit ballot per 64-primitive chunk, and a coarse wave
// ANDs its row's and column's words to get its candidates in primitive
// order without reading any box.  Frames with more than kMaskBinsMax bin
// rows + columns (extreme aspect ratios) scan the boxes instead.
constexpr int kMaskBinsMax = 4096;
constexpr double kEpsilon = 0.000001;      // MainState.cpp:15
constexpr float kFar = 300000.0f;          // MainState.cpp:345

typedef int int4v __attribute__((ext_vector_type(4)));

// Per-triangle constants of the binned path (128 B, scalar-loaded).
// With implicit origins (x, y, 0) and dir = (0, 0, D): pvec = d x e2 and
// det, inv_det are per-triangle; tvec = (x - v0x, y - v0y, -v0z) varies only
// in x and y.  Every field is produced by the same fp64 operation sequence as
// MainState.cpp:257-298, so per-pixel results are bit-identical.
struct alignas(16) TriRec {
    double v0x, v0y, p0, p1;
    double inv_det, e1x, e1y, e1z;
    double e2x, e2y, e2z, k0;  // k0 = tz * e1y
    double k1, dz, pad0, pad1; // k1 = tz * e1x, dz = D
};
static_assert(sizeof(TriRec) == 128, "TriRec layout");

// Per-triangle depth model for the coarse depth cull (48 B): the trace's t
// (tri_rows) is, in exact arithmetic, the affine function A + Bx x + By y of
// the pixel; the computed t differs from that by at most M0 + Mx|x| + My|y|
// (see prep_triangle).  Invalid (never a coverer, never dropped) when M0 is
// not finite.
struct alignas(16) TriDepth {
    double a, bx, by, m0, mx, my;
};
static_assert(sizeof(TriDepth) == 48, "TriDepth layout");

// Per-sphere constants of the binned path (32 B).  With dir = (0, 0, D, Dw)
// and origins (x, y, 0, 1): tca = dot4(L, d) and the z/w half of dot4(L, L)
// do not depend on the pixel (MainState.cpp:300-327, glm pairwise dot).
// `fast` (1 or 0): every lane that can hit gets an r2 - dist2 in
// {0} u [2^-94, 2^102], where sqrt_rn_normal equals sqrtf (see prep_sphere).
// `tmin_key`: order_key of a lower bound of every lane's t0 (see prep_sphere;
// 0 = no bound), for depth culling in the trace.
struct alignas(16) SphRec {
    float cx, cy, kzw, tca2;  // kzw = Lz*Lz + Lw*Lw, tca2 = tca*tca
    float r2, tca, fast;
    unsigned tmin_key;
};
static_assert(sizeof(SphRec) == 32, "SphRec layout");

// Per-primitive tile classifier (32 B, fp32; evaluated by the coarse kernel).
// Triangle: a = (v0x, v0y, au, bu), b = (av, bv, g, 0) with the exact
// barycentrics u = au (x - v0x) + bu (y - v0y), v = av (x - v0x) + bv (y -
// v0y) up to a margin g that also covers the fp64 rounding of the per-pixel
// test, so a wave tile can be proven fully outside (skip) or fully inside
// (no u/v tests, t only) in fp32.  g = +inf disables both.
// Sphere: a = (cx, cy, R2, 0): every pixel farther than sqrt(R2) misses.
struct Cls {
    float4 a, b;
};
static_assert(sizeof(Cls) == 32, "Cls layout");

struct Box { int x0, y0, x1, y1; };  // inclusive pixel range, empty if x0 > x1

// Inverted far-out-of-range box: fails every overlap test against any pixel
// rectangle, so empty primitives can never reach a bin or a wave tile.
__host__ __device__ inline Box empty_box() {
    return Box{1 << 30, 1 << 30, -(1 << 30), -(1 << 30)};
}

// Unsigned key with the order of the float (for non-NaN values): positives
// above negatives, -0 just below +0.
__host__ __device__ inline unsigned order_key(float f) {
    unsigned b;
    memcpy(&b, &f, sizeof b);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

__host__ __device__ inline bool finite3(double a, double b, double c) {
    return std::isfinite(a) && std::isfinite(b) && std::isfinite(c);
}

__host__ __device__ inline int clamp_floor(double v, int lo, int hi) {
    if (!(v > (double)lo)) return lo;
    if (!(v < (double)hi)) return hi;
    return (int)floor(v);
}
__host__ __device__ inline int clamp_ceil(double v, int lo, int hi) {
    if (!(v > (double)lo)) return lo;
    if (!(v < (double)hi)) return hi;
    return (int)ceil(v);
}

// Triangle prep.  Returns false when the triangle can never report a hit in
// the reference (|det| < EPSILON or a NaN det).  The box bound: outside the
// triangle's xy box by a distance Dist, the exact barycentric minimum is
// <= -Dist / (2 * extent); the computed u, v differ from the exact ones by
// at most `err` (rounding of e1, e2, pvec, det, tvec and the products), so
// a pad of 2 * extent * (2 * err + slack) (here x4 more) guarantees that
// the computed test rejects.  Ill-conditioned dets get the whole band.
__host__ __device__ inline bool prep_triangle(const float* a, const float* b, const float* c,
                                              double dx, double dy, double dz, int width,
                                              int row_begin, int row_end, TriRec* rec,
                                              Box* box, Cls* cls, bool* nonfinite,
                                              TriDepth* depth = nullptr) {
    const double v0[3] = {a[0], a[1], a[2]};
    const double v1[3] = {b[0], b[1], b[2]};
    const double v2[3] = {c[0], c[1], c[2]};
    *nonfinite = !(finite3(v0[0], v0[1], v0[2]) && finite3(v1[0], v1[1], v1[2]) &&
                   finite3(v2[0], v2[1], v2[2]));
    const double e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const double e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    const double p0 = dy * e2[2] - dz * e2[1];
    const double p1 = dz * e2[0] - dx * e2[2];
    const double p2 = dx * e2[1] - dy * e2[0];
    const double det = e1[0] * p0 + e1[1] * p1 + e1[2] * p2;
    *box = empty_box();
    cls->a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    cls->b = make_float4(0.0f, 0.0f, INFINITY, 0.0f);
    if ((det > -kEpsilon && det < kEpsilon) || !(det == det) || *nonfinite) return false;
    const double inv_det = 1.0 / det;
    const double tz = 0.0 - v0[2];
    rec->v0x = v0[0];
    rec->v0y = v0[1];
    rec->p0 = p0;
    rec->p1 = p1;
    rec->inv_det = inv_det;
    rec->e1x = e1[0];
    rec->e1y = e1[1];
    rec->e1z = e1[2];
    rec->e2x = e2[0];
    rec->e2y = e2[1];
    rec->e2z = e2[2];
    rec->k0 = tz * e1[1];
    rec->k1 = tz * e1[0];
    rec->dz = dz;
    rec->pad0 = rec->pad1 = 0.0;
    if (depth) {
        // tri_row's t = ((e2x q0 + e2y q1) + e2z q2) inv with q0 = ty e1z - k0,
        // q1 = k1 - tx e1z, q2 = tx e1y - ty e1x, tx = x - v0x, ty = y - v0y,
        // is, exactly, A + Bx x + By y with Bx = (e2z e1y - e2y e1z) inv,
        // By = (e2x e1z - e2z e1x) inv, A = (e2y k1 - e2x k0) inv - Bx v0x -
        // By v0y.  Error bound (u = 2^-53): the trace's roundings contribute
        // at most 16u S with S = s0 + aBx |tx| + aBy |ty| (s0 = (|e2x k0| +
        // |e2y k1|) |inv|, aBx, aBy the absolute-value sums of Bx, By), the
        // fp64 coefficients and their evaluation at most 16u (aA + aBx |x| +
        // aBy |y|) (aA that of A); with |tx| <= |x| + |v0x| and 2x slack,
        // M0 = 64u (s0 + aA + aBx |v0x| + aBy |v0y|), Mx = 64u aBx, My = 64u aBy.
        const double ai = fabs(inv_det);
        const double bx = (e2[2] * e1[1] - e2[1] * e1[2]) * inv_det;
        const double by = (e2[0] * e1[2] - e2[2] * e1[0]) * inv_det;
        const double k0 = rec->k0, k1 = rec->k1;
        const double a0 = (e2[1] * k1 - e2[0] * k0) * inv_det - bx * v0[0] - by * v0[1];
        const double abx = (fabs(e2[2] * e1[1]) + fabs(e2[1] * e1[2])) * ai;
        const double aby = (fabs(e2[0] * e1[2]) + fabs(e2[2] * e1[0])) * ai;
        const double s0 = (fabs(e2[0] * k0) + fabs(e2[1] * k1)) * ai;
        const double aa = s0 + abx * fabs(v0[0]) + aby * fabs(v0[1]);
        const double u64 = 64.0 * 1.1102230246251565e-16;
        depth->a = a0;
        depth->bx = bx;
        depth->by = by;
        depth->m0 = u64 * (s0 + aa + abx * fabs(v0[0]) + aby * fabs(v0[1])) + 1e-300;
        depth->mx = u64 * abx;
        depth->my = u64 * aby;
    }

    const double eps = 1.1102230246251565e-16;  // 2^-53
    const double mnx = fmin(v0[0], fmin(v1[0], v2[0])), mxx = fmax(v0[0], fmax(v1[0], v2[0]));
    const double mny = fmin(v0[1], fmin(v1[1], v2[1])), mxy = fmax(v0[1], fmax(v1[1], v2[1]));
    // |tx|, |ty| bounds over the band, widened by one bin for tile overhang
    const double tx_max = fmax(fabs(0.0 - v0[0]), fabs((double)(width + 31) - v0[0])) + 1.0;
    const double ty_max =
        fmax(fabs((double)row_begin - v0[1]), fabs((double)(row_end + 31) - v0[1])) + 1.0;
    const double adet = fabs(det);
    const double rho =
        8.0 * eps * (fabs(e1[0] * p0) + fabs(e1[1] * p1) + fabs(e1[2] * p2)) / adet + 4.0 * eps;
    Box bx{0, row_begin, width - 1, row_end - 1};
    if (rho < 0.25) {
        const double s = (tx_max * (fabs(p0) + fabs(e1[1] * dz)) +
                          ty_max * (fabs(p1) + fabs(e1[0] * dz))) * fabs(inv_det);
        const double err = (32.0 * eps + 4.0 * rho) * s + 32.0 * eps;
        const double g = 2.0 * err + 8.0 * eps * s + 32.0 * eps;
        // fp32 classifier planes and their margin.  The classifier only ever
        // sees pixels of wave tiles (at most kTileSpan px on a side) that
        // overlap the box, so |x - v0x| and |y - v0y| are bounded by the padded
        // box plus kTileSpan: the margin
        // covers the fp64 test's rounding there (err_loc) and the fp32
        // rounding of the coefficients and of the plane evaluation (2^-24
        // each, x32 slack).
        const double padx0 = 8.0 * (mxx - mnx) * g + 0.5, pady0 = 8.0 * (mxy - mny) * g + 0.5;
        const double span = (double)kTileSpan;
        const double tx_loc = fmax(fabs(mnx - padx0 - span - v0[0]), fabs(mxx + padx0 + span - v0[0])) + 1.0;
        const double ty_loc = fmax(fabs(mny - pady0 - span - v0[1]), fabs(mxy + pady0 + span - v0[1])) + 1.0;
        const double s_loc = (tx_loc * (fabs(p0) + fabs(e1[1] * dz)) +
                              ty_loc * (fabs(p1) + fabs(e1[0] * dz))) * fabs(inv_det);
        const double err_loc = (32.0 * eps + 4.0 * rho) * s_loc + 32.0 * eps;
        const double g_loc = 2.0 * err_loc + 8.0 * eps * s_loc + 32.0 * eps;
        const double au = p0 * inv_det, bu = p1 * inv_det;
        const double av = dz * e1[1] * inv_det, bv = -(dz * e1[0]) * inv_det;
        const double suv = (fabs(au) + fabs(av)) * tx_loc + (fabs(bu) + fabs(bv)) * ty_loc;
        const double gm = g_loc + 32.0 * 5.9604644775390625e-08 * suv + 1e-6;
        cls->a = make_float4((float)v0[0], (float)v0[1], (float)au, (float)bu);
        cls->b = make_float4((float)av, (float)bv, (float)(gm * (1.0 + 1e-6)), 0.0f);
        const double padx = 8.0 * (mxx - mnx) * g + 0.5;
        const double pady = 8.0 * (mxy - mny) * g + 0.5;
        bx.x0 = clamp_floor(mnx - padx, 0, width - 1);
        bx.x1 = clamp_ceil(mxx + padx, 0, width - 1);
        bx.y0 = clamp_floor(mny - pady, row_begin, row_end - 1);
        bx.y1 = clamp_ceil(mxy + pady, row_begin, row_end - 1);
        // wholly outside the band / frame?
        if (mxx + padx < 0.0 || mnx - padx > (double)(width - 1) ||
            mxy + pady < (double)row_begin || mny - pady > (double)(row_end - 1))
            return true;  // box stays empty
    }
    *box = bx;
    return true;
}

// Sphere prep (fp32, MainState.cpp:300-327 with glm's pairwise vec4 dot).
// Miss is guaranteed where |L|^2 (1 - 8e) > r2 - (kzw - tca2) + 8e(|kzw| +
// |tca2|), e = 2^-23 (bound on the fp32 rounding of Lx, Ly, their squares
// and the two sums); the box is that radius plus one pixel.
__host__ __device__ inline void prep_sphere(const float* o, float radius, float dx, float dy,
                                            float dz, float dw, int width, int row_begin,
                                            int row_end, SphRec* rec, Box* box, Cls* cls,
                                            bool* nonfinite) {
    *box = empty_box();
    cls->a = make_float4(o[0], o[1], -1.0f, 0.0f);
    cls->b = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    *nonfinite = !(std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]) &&
                   std::isfinite(o[3]) && std::isfinite(radius));
    const float lz = o[2] - 0.0f;
    const float lw = o[3] - 1.0f;
    const float tca = (lz * dz) + (lw * dw);  // + (Lx*dx + Ly*dy) == +-0
    const float kzw = (lz * lz) + (lw * lw);
    const float tca2 = tca * tca;
    const float r2 = radius * radius;
    rec->cx = o[0];
    rec->cy = o[1];
    rec->kzw = kzw;
    rec->tca2 = tca2;
    rec->r2 = r2;
    rec->tca = tca;
    // r2 >= 2^-70: a hitting lane has dist2 <= r2, so r2 - dist2 is 0, or
    // >= r2 / 2 (dist2 <= r2 / 2), or an exact nonzero difference of floats
    // >= r2 / 2, a multiple of ulp(2^-71) = 2^-94.  The 2^100 caps keep
    // dist2 >= -2^101, so r2 - dist2 <= 2^102 (and tca2 finite).
    rec->fast = (r2 >= 0x1p-70f && r2 <= 0x1p100f && fabsf(tca2) <= 0x1p100f &&
                 fabsf(kzw) <= 0x1p100f) ? 1.0f : 0.0f;
    // Lower bound of t0 over all pixels, by monotonicity of IEEE rounding:
    // lx*lx + ly*ly >= 0, so dist2 = ((.) + kzw) - tca2 >= kzw - tca2 = d0,
    // arg = r2 - dist2 <= r2 - d0 = a0, thc <= sqrtf(a0) (correctly rounded
    // on both sides), t0 = tca - thc >= tca - sqrtf(a0).  The same float ops
    // in the same order, so the bound holds for the computed values.
    {
        const float d0 = kzw - tca2;
        const float a0 = r2 - d0;
        const float tmin = tca - sqrtf(a0);
        rec->tmin_key = tmin == tmin ? order_key(tmin) : 0u;  // NaN: no bound
    }
    (void)dx;
    (void)dy;
    if (*nonfinite || !(tca >= 0.0f)) return;  // tca < 0 (or NaN): never a hit
    const double e = 1.1920928955078125e-07;  // 2^-23
    const double bound = ((double)r2 - ((double)kzw - (double)tca2) +
                          8.0 * e * (fabs((double)kzw) + fabs((double)tca2))) /
                         (1.0 - 8.0 * e);
    if (!(bound >= 0.0)) return;  // every pixel misses
    const double r = sqrt(bound * (1.0 + 1e-6) + 1e-6) + 1.0;
    cls->a.z = (float)(bound * (1.0 + 1e-5) + 1e-5);
    const double cx = o[0], cy = o[1];
    if (cx + r < 0.0 || cx - r > (double)(width - 1) || cy + r < (double)row_begin ||
        cy - r > (double)(row_end - 1))
        return;
    box->x0 = clamp_floor(cx - r, 0, width - 1);
    box->x1 = clamp_ceil(cx + r, 0, width - 1);
    box->y0 = clamp_floor(cy - r, row_begin, row_end - 1);
    box->y1 = clamp_ceil(cy + r, row_begin, row_end - 1);
}

// Bounds [lo, hi] of the trace's computed t (tri_row, fp64,
// MainState.cpp:257-298) over every pixel (x, y) of [xa, xb] x [ya, yb]
// (pixel coordinates >= 0): the affine model's extremes, at the corners,
// widened by its error bound at the largest x, y (TriDepth, prep_triangle)
// and, 2x, for the few roundings of this evaluation.  Returns false when a
// bound is not finite (no cull for this triangle).
__host__ __device__ inline bool tri_t_bounds(const TriDepth& d, double xa, double xb, double ya,
                                             double yb, double* lo, double* hi) {
    const double x1 = d.bx * xa, x2 = d.bx * xb, y1 = d.by * ya, y2 = d.by * yb;
    const double m = 2.0 * (d.m0 + d.mx * xb + d.my * yb);
    *lo = (d.a + fmin(x1, x2) + fmin(y1, y2)) - m;
    *hi = (d.a + fmax(x1, x2) + fmax(y1, y2)) + m;
    return *lo > -INFINITY && *hi < INFINITY && m < INFINITY;  // false for NaN too
}

// (int)f as x86-64 cvttss2si: truncation, NaN / out of range -> INT32_MIN.
__device__ __forceinline__ int cvt_i32(float f) {
    return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT32_MIN;
}

// The same on the hot path: v_cvt_i32_f32 truncates and saturates (-inf and
// everything below -2^31 -> INT32_MIN, NaN -> 0, >= 2^31 -> INT32_MAX); the
// one compare maps NaN and >= 2^31 to x86's INT32_MIN.  Inline asm keeps the
// hardware semantics (a C++ (int) of an out-of-range float is undefined).
__device__ __forceinline__ int cvt_i32_fast(float f) {
    int r;
    asm volatile("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(f));
    return f < 2147483648.0f ? r : INT32_MIN;
}

// Correctly rounded x / 180.0f without the IEEE division sequence:
// q0 = x * RN(1/180), q = fma(fma(-q0, 180, x), RN(1/180), q0) equals RN(x/180)
// for every finite float with |x| >= 2^-100 (exhaustively checked on the host,
// scripts/check_div180.c); smaller |x| takes the division.
__device__ __forceinline__ float div180(float x) {
    const float r = 1.0f / 180.0f;
    const float q0 = x * r;
    const float rem = __builtin_fmaf(-q0, 180.0f, x);
    float q = __builtin_fmaf(rem, r, q0);
    const bool tiny = !(__builtin_fabsf(x) >= 0x1p-100f);
    if (__ballot(tiny)) q = tiny ? x / 180.0f : q;
    return q;
}

// MainState.cpp:396-407 + :952-955 (or the Texture packing :1026-1036).
__device__ __forceinline__ int4v shade(float closest, float4 colour) {
    if (closest == kFar) return int4v{0, 0, 0, 255};
    const float normalised = (closest - 0.0f) / (180.0f - 0.0f);
    const float scalar = 255.0f - (normalised * 255.0f);
    return int4v{cvt_i32(scalar * colour.x), cvt_i32(scalar * colour.y),
                 cvt_i32(scalar * colour.z), 255};
}

__device__ __forceinline__ unsigned pack_rgba8(int4v p) {
    return (unsigned)(unsigned char)p.x | ((unsigned)(unsigned char)p.y << 8) |
           ((unsigned)(unsigned char)p.z << 16) | 0xFF000000u;
}

// ---------------------------------------------------------------------------
// Generic per-pixel path: the reference algorithm verbatim (any origin and
// direction).  MainState.cpp:257-298 (fp64 MT), :300-327, :330-408.
// ---------------------------------------------------------------------------
__device__ inline int intersect_tri(const double* orig, const double* dir, const double* v0,
                                    const double* v1, const double* v2, double* t) {
    double e1[3], e2[3], tv[3], pv[3], qv[3];
    e1[0] = v1[0] - v0[0]; e1[1] = v1[1] - v0[1]; e1[2] = v1[2] - v0[2];
    e2[0] = v2[0] - v0[0]; e2[1] = v2[1] - v0[1]; e2[2] = v2[2] - v0[2];
    pv[0] = dir[1] * e2[2] - dir[2] * e2[1];
    pv[1] = dir[2] * e2[0] - dir[0] * e2[2];
    pv[2] = dir[0] * e2[1] - dir[1] * e2[0];
    const double det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
    if (det > -kEpsilon && det < kEpsilon) return 0;
    const double inv_det = 1.0 / det;
    tv[0] = orig[0] - v0[0]; tv[1] = orig[1] - v0[1]; tv[2] = orig[2] - v0[2];
    const double u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) * inv_det;
    if (u < 0.0 || u > 1.0) return 0;
    qv[0] = tv[1] * e1[2] - tv[2] * e1[1];
    qv[1] = tv[2] * e1[0] - tv[0] * e1[2];
    qv[2] = tv[0] * e1[1] - tv[1] * e1[0];
    const double v = (dir[0] * qv[0] + dir[1] * qv[1] + dir[2] * qv[2]) * inv_det;
    if (v < 0.0 || u + v > 1.0) return 0;
    *t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * inv_det;
    return 1;
}

__device__ inline float dot4(float4 a, float4 b) {
    return ((a.x * b.x) + (a.y * b.y)) + ((a.z * b.z) + (a.w * b.w));
}

__device__ inline float intersect_sphere(float4 o, float4 d, float radius, float4 c) {
    const float4 l = make_float4(c.x - o.x, c.y - o.y, c.z - o.z, c.w - o.w);
    const float tca = dot4(l, d);
    if (tca < 0) return 0.0f;
    const float dist2 = dot4(l, l) - tca * tca;
    const float r2 = radius * radius;
    if (dist2 > r2) return 0.0f;
    const float thc = sqrtf(r2 - dist2);
    return tca - thc;
}

struct SceneDev {
    const float4* __restrict__ sphere_origins;
    const float* __restrict__ sphere_radius;
    const float4* __restrict__ sphere_colours;
    const float4* __restrict__ cube_vertices;
    const float4* __restrict__ cube_colours;
    int n_spheres, n_cubes;
};

// The collide loop (MainState.cpp:345-394) up to, not including, the shade:
// `closest` and what the winner leaves behind.  kSlot: its colour slot (cube
// c: c, sphere i: n_cubes + i; -1 beside kFar: no hit), for RT_FORMAT_HIT.
// Otherwise its colour, loaded when it wins as the reference does (the two
// colour formats' code is what it was before the slot existed; `slot` is
// then not tracked and stays -1).
struct GenericHit {
    float closest;
    int slot;
    float4 colour;
};
template <bool kSlot>
__device__ inline GenericHit closest_generic(const SceneDev& s, float4 origin, float4 dir) {
    const double o[3] = {origin.x, origin.y, origin.z};
    const double d[3] = {dir.x, dir.y, dir.z};
    float closest = kFar;
    int slot = -1;
    float4 colour = make_float4(0.0f, 0.0f, 0.0f, 255.0f);
    for (int c = 0; c < s.n_cubes; ++c) {
        const float4* tri = s.cube_vertices + 36 * c;
        for (int k = 0; k < 36; k += 3) {
            const float4 a = tri[k], b = tri[k + 1], e = tri[k + 2];
            const double v0[3] = {a.x, a.y, a.z}, v1[3] = {b.x, b.y, b.z}, v2[3] = {e.x, e.y, e.z};
            double t;
            if (intersect_tri(o, d, v0, v1, v2, &t) == 1 && (float)t < closest) {
                closest = (float)t;
                if constexpr (kSlot)
                    slot = c;
                else
                    colour = s.cube_colours[c];
            }
        }
    }
    for (int i = 0; i < s.n_spheres; ++i) {
        const float dist = intersect_sphere(origin, dir, s.sphere_radius[i], s.sphere_origins[i]);
        if (dist == 0.0f) continue;
        if (dist < closest) {
            closest = dist;
            if constexpr (kSlot)
                slot = s.n_cubes + i;
            else
                colour = s.sphere_colours[i];
        }
    }
    return GenericHit{closest, slot, colour};
}

// A lane's RT_FORMAT_HIT pixel in the kernels' pixel registers: the rt_hit
// words in x and y (z, w unused).
__device__ __forceinline__ int4v hit_pixel(float closest, int slot) {
    return int4v{(int)__float_as_uint(closest), slot, 0, 0};
}

// One hit_pixel to pixel `idx` of an rt_hit frame.
__device__ __forceinline__ void store_hit(void* __restrict__ out, int64_t idx, int4v pix) {
    reinterpret_cast<int2*>(out)[idx] = make_int2(pix.x, pix.y);
}

// The reference's pixel: the collide loop, then its shade (int32x4; the
// Texture word is packed from it) -- or, for RT_FORMAT_HIT, the loop's result
// itself (hit_pixel).
template <int kFmt = RT_FORMAT_I32X4>
__device__ inline int4v collide_generic(const SceneDev& s, float4 origin, float4 dir) {
    const GenericHit h = closest_generic<kFmt == RT_FORMAT_HIT>(s, origin, dir);
    if constexpr (kFmt == RT_FORMAT_HIT)
        return hit_pixel(h.closest, h.slot);
    else
        return shade(h.closest, h.colour);
}

__global__ void __launch_bounds__(kThreads) generic_kernel(
    SceneDev scene, float4 dir, const float4* __restrict__ origins, int width,
    int row_begin, int row_end, int out_format, void* __restrict__ out) {
    // grid-stride: the AQL grid counts work-items in 32 bits, frames may not
    const int64_t n = (int64_t)width * (row_end - row_begin);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int x = (int)(i % width);
        const int y = row_begin + (int)(i / width);
        // `origins` starts at row row_begin (the band's rows only)
        const float4 o = origins ? origins[i] : make_float4((float)x, (float)y, 0.0f, 1.0f);
        if (out_format == RT_FORMAT_HIT) {  // (kernel-uniform)
            store_hit(out, i, collide_generic<RT_FORMAT_HIT>(scene, o, dir));
            continue;
        }
        const int4v p = collide_generic(scene, o, dir);
        if (out_format == RT_FORMAT_I32X4)
            reinterpret_cast<int4v*>(out)[i] = p;
        else
            reinterpret_cast<unsigned*>(out)[i] = pack_rgba8(p);
    }
}

// ---------------------------------------------------------------------------
// Binned path
// ---------------------------------------------------------------------------
// Bin masks (`row_masks` != nullptr): after its records and boxes, each prep
// wave (one 64-primitive chunk) writes row_masks[r * n_chunks + chunk] and
// col_masks[c * n_chunks + chunk]: the ballot of its primitives whose box
// overlaps bin row r / bin column c.  Every word is written every frame.
// Wave64 OR scans on DPP (no LDS round trips; every lane active).  Prefix:
// lane l gets lanes 0..l -- row_shr 1, 2, 4, 8 within each row of 16, then
// row_bcast 15 / 31 carry the rows below.  Suffix: lane l gets lanes l..63 --
// row_shl within each row, then the totals of the rows above (their first
// lanes, read into scalars).
__device__ __forceinline__ unsigned wave_prefix_or(unsigned v) {
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}
__device__ __forceinline__ unsigned wave_suffix_or(unsigned v, int lane) {
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, false);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x102, 0xf, 0xf, false);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xf, 0xf, false);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x108, 0xf, 0xf, false);
    const unsigned r1 = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
    const unsigned r2 = (unsigned)__builtin_amdgcn_readlane((int)v, 32);
    const unsigned r3 = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
    return v | (lane < 16 ? (r1 | r2 | r3) : lane < 32 ? (r2 | r3) : lane < 48 ? r3 : 0u);
}
// Wave64 inclusive prefix sum (every lane active): DPP row prefix sums, then
// the row broadcasts; the sum is lane 63's value.
__device__ __forceinline__ unsigned wave_prefix_sum(unsigned v) {
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
    return (unsigned)__builtin_amdgcn_readlane((int)wave_prefix_sum(v), 63);
}
__device__ __forceinline__ unsigned long long wave_prefix_or64(unsigned long long v) {
    return (unsigned long long)wave_prefix_or((unsigned)v) |
           ((unsigned long long)wave_prefix_or((unsigned)(v >> 32)) << 32);
}
__device__ __forceinline__ unsigned long long wave_suffix_or64(unsigned long long v, int lane) {
    return (unsigned long long)wave_suffix_or((unsigned)v, lane) |
           ((unsigned long long)wave_suffix_or((unsigned)(v >> 32), lane) << 32);
}

#ifndef RT_BIN_DROP
#define RT_BIN_DROP 1  // depth cull: bin-level lower bound before the tile-local ones
#endif
__global__ void __launch_bounds__(kPrepThreads) prep_kernel(
    SceneDev scene, float4 dir, int width, int row_begin, int row_end,
    TriRec* __restrict__ tri, TriDepth* __restrict__ tdep, SphRec* __restrict__ sph,
    int4* __restrict__ boxes,
    Cls* __restrict__ cls, float4* __restrict__ colours, unsigned* __restrict__ nonfinite_flag,
    unsigned gen, unsigned long long* __restrict__ row_masks,
    unsigned long long* __restrict__ col_masks, int n_cx, int n_cy,
    unsigned long long* __restrict__ overdraw) {
    const int n_tri = 12 * scene.n_cubes;
    const int n_prims = n_tri + scene.n_spheres;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x;
    Box b = empty_box();
    Cls k{};
    bool bad = false;
    if (i < n_tri) {
        const float4* v = scene.cube_vertices + 3 * i;
        const float4 a = v[0], bb = v[1], c = v[2];
        const float fa[3] = {a.x, a.y, a.z}, fb[3] = {bb.x, bb.y, bb.z}, fc[3] = {c.x, c.y, c.z};
        if (i % 12 == 0) colours[i / 12] = scene.cube_colours[i / 12];
        TriRec r{};
        TriDepth dd{0.0, 0.0, 0.0, INFINITY, 0.0, 0.0};
        prep_triangle(fa, fb, fc, (double)dir.x, (double)dir.y, (double)dir.z, width, row_begin,
                      row_end, &r, &b, &k, &bad, &dd);
        tri[i] = r;
        tdep[i] = dd;
    } else if (i < n_prims) {
        const int s = i - n_tri;
        const float4 o = scene.sphere_origins[s];
        colours[scene.n_cubes + s] = scene.sphere_colours[s];
        const float fo[4] = {o.x, o.y, o.z, o.w};
        SphRec r{};
        prep_sphere(fo, scene.sphere_radius[s], dir.x, dir.y, dir.z, dir.w, width, row_begin,
                    row_end, &r, &b, &k, &bad);
        sph[s] = r;
    }
    if (i < n_prims) {
        boxes[i] = make_int4(b.x0, b.y0, b.x1, b.y1);
        cls[i] = k;
        if (bad) atomicMax(nonfinite_flag, gen);
    }
    if (overdraw) {
        // the frame's box overdraw for the coarse kernel's triangle gate: the
        // sum of the boxes' areas in units of 64 pixels, one atomic add per
        // wave (coarse zeroes the other slot for the next launch)
        // (per primitive at most 2^25 units, so a wave's sum fits 32 bits)
        unsigned v = 0u;
        if (i < n_prims && b.x0 <= b.x1 && b.y0 <= b.y1) {
            const unsigned long long a =
                ((unsigned long long)(b.x1 - b.x0 + 1) * (unsigned long long)(b.y1 - b.y0 + 1) +
                 63ull) >> 6;
            v = a < (1ull << 25) ? (unsigned)a : (1u << 25);
        }
        const unsigned total = wave_sum(v);
        if (lane == 0 && total) atomicAdd(overdraw, (unsigned long long)total);
    }
    if (!row_masks) return;
    const int chunk = (int)blockIdx.x;
    const int n_chunks = (int)gridDim.x;
    const bool live = i < n_prims && b.x0 <= b.x1 && b.y0 <= b.y1;
    // Per block of 64 bins, lane r builds bin r's word without a ballot per
    // bin: first[r] / last[r] collect the primitives whose box starts / ends
    // in bin r (LDS OR), a prefix OR of first and a suffix OR of last (plus
    // the primitives starting before / ending after the block) give the
    // primitives with start <= r and end >= r; their AND is bin r's word.
    __shared__ unsigned long long s_first[64], s_last[64];
    auto bin_words = [&](int lo, int hi, int n_bins, int bin_px, unsigned long long* out) {
        const int blo = live ? lo / bin_px : INT32_MAX;
        const int bhi = live ? hi / bin_px : -1;
        const unsigned long long me = 1ull << lane;
        for (int r0 = 0; r0 < n_bins; r0 += 64) {
            s_first[lane] = 0ull;
            s_last[lane] = 0ull;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (blo >= r0 && blo < r0 + 64) atomicOr(&s_first[blo - r0], me);
            if (bhi >= r0 && bhi < r0 + 64) atomicOr(&s_last[bhi - r0], me);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const unsigned long long f = wave_prefix_or64(s_first[lane]);
            const unsigned long long e = wave_suffix_or64(s_last[lane], lane);
            const unsigned long long f_in = __ballot(blo < r0);        // started before
            const unsigned long long e_in = __ballot(bhi >= r0 + 64 && bhi != -1);  // ends after
            if (r0 + lane < n_bins)
                out[(int64_t)(r0 + lane) * n_chunks + chunk] = (f | f_in) & (e | e_in);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    };
    bin_words(b.y0 - row_begin, b.y1 - row_begin, n_cy, kCoarseH, row_masks);
    bin_words(b.x0, b.x1, n_cx, kCoarseW, col_masks);
}

#if RT_TIMELINE
// per wave: realtime at entry / first staged / walked / stores issued,
// s_memtime at entry / end, HW_ID, XCC_ID
__device__ unsigned* g_timeline;
__device__ __forceinline__ unsigned rt_now() { return (unsigned)__builtin_amdgcn_s_memrealtime(); }
#define TL_MARK(v) const unsigned v = rt_now()
#else
#define TL_MARK(v)
#endif

// A candidate's record (wave-uniform index, 0 <= i < 2^25), addressed by a
// 32-bit byte offset (one s_lshl_b32, then the 64-bit add) instead of the
// sign extension and 64-bit shift of base[i], shortening the scalar chain in
// front of each record's load (round 6: kernels 0.2-1 % faster, DESIGN.md
// §3.5).
__device__ __forceinline__ TriRec tri_at(const TriRec* __restrict__ base, int i) {
    return *reinterpret_cast<const TriRec*>(reinterpret_cast<const char*>(base) +
                                            ((unsigned)i << 7));
}
__device__ __forceinline__ SphRec sph_at(const SphRec* __restrict__ base, int i) {
    return *reinterpret_cast<const SphRec*>(reinterpret_cast<const char*>(base) +
                                            ((unsigned)i << 5));
}

// The overdraw verdict word (rt_ctx::od_verdict): one lane's vector store at
// system scope, so that a word in page-locked host memory is written through
// to it rather than held in the device's caches.
__device__ __forceinline__ void store_verdict(unsigned* w, unsigned v) {
    __hip_atomic_store(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Per-lane exact tests of one candidate primitive `p` (wave-uniform) on the
// lane's kRowsPerLane pixels.  Triangles: MainState.cpp:257-298 restated on
// the per-triangle constants (see TriRec); `inside` (wave-uniform) means the
// tile classifier proved every pixel of the tile passes the u/v tests, so
// only the exact t is computed.  Spheres: :300-327 on SphRec.
// Select-based form: every row evaluates the whole test and a compare picks
// the result, so the wave never diverges inside the walk.  The per-lane
// (row-invariant) products are hoisted; each is the same fp64 operation on
// the same operands as in MainState.cpp:257-298, so values are unchanged.
// (Skipping a row whose lanes all miss, by ballot, measured slower in both
// formats: DESIGN.md §3.5.)

// px[j], py[j]: pixel j of this lane (px[j] equal for every j in the
// one-column geometries, py[j] in the 256x1 one: the x- or y-only terms are
// then computed once).
//
// Each test is split in two: *_rows computes, per row, the candidate's
// float t, or NaN where it may not take the pixel (u,v failed for a
// triangle, t0 == 0 for a sphere; a sphere miss gives t0 = NaN by itself),
// and take_rows applies the strict `<` against closest (MainState.cpp:
// 386-391), which NaN never passes (closest is never NaN).  The walk keeps
// one take_rows after both primitive branches, so closest and hit are
// updated in one place.

// One row of MainState.cpp:257-298 on TriRec; `uv`: evaluate the u, v tests.
__device__ __forceinline__ float tri_row(const TriRec& r, double px, double py, bool uv,
                                         bool* pass) {
    const double tx = px - r.v0x;
    const double txe1y = tx * r.e1y;               // q2 = tx*e1y - ty*e1x
    const double q1 = r.k1 - tx * r.e1z;           // q1 = tz*e1x - tx*e1z
    const double e2yq1 = r.e2y * q1;
    const double txp0 = tx * r.p0;                 // u = (tx*p0 + ty*p1) * inv_det
    const double ty = py - r.v0y;
    const double q2 = txe1y - ty * r.e1x;
    *pass = true;
    if (uv) {
        const double u = (txp0 + ty * r.p1) * r.inv_det;
        const double v = (r.dz * q2) * r.inv_det;
        *pass = !((u < 0.0) | (u > 1.0) | (v < 0.0) | (u + v > 1.0));
    }
    const double q0 = ty * r.e1z - r.k0;
    const double t = ((r.e2x * q0 + e2yq1) + r.e2z * q2) * r.inv_det;
    return (float)t;
}

// The rows of a lane for one triangle: its pixel coordinates are held in
// px / py (exact integers) for the whole walk.
__device__ __forceinline__ void tri_rows(const TriRec& r, unsigned bits, const double* px,
                                         const double* py, float* t) {
    bool pass;
    if constexpr (kBlocks == 1) {
        // one verdict for the whole tile (wave-uniform), branched once
        if (bits & 2u) {
#pragma unroll
            for (int j = 0; j < kRowsPerLane; ++j)
                t[j] = tri_row(r, px[kStepsX == 1 ? 0 : j], py[j], false, &pass);
        } else {
#pragma unroll
            for (int j = 0; j < kRowsPerLane; ++j) {
                const float tf = tri_row(r, px[kStepsX == 1 ? 0 : j], py[j], true, &pass);
                t[j] = pass ? tf : __builtin_nanf("");
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) {
            // this row's block: bit 0 keep, bit 1 u,v proven inside (wave-uniform)
            const unsigned rb = bits >> (2 * row_block(j));
            const float tf = tri_row(r, px[kStepsX == 1 ? 0 : j], py[j], !(rb & 2u), &pass);
            t[j] = pass && (rb & 1u) ? tf : __builtin_nanf("");
        }
    }
}

__device__ __forceinline__ void take_rows(const float* t, int slot, float* closest, int* hit) {
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
        const bool take = t[j] < closest[j];
        closest[j] = take ? t[j] : closest[j];
        hit[j] = take ? slot : hit[j];
    }
}

// Correctly rounded sqrtf for x in [2^-96, FLT_MAX]: v_sqrt_f32 plus the two
// FMA residual corrections of the compiler's IEEE expansion, without its
// denormal scaling and zero/inf fix-up (equal to sqrtf on every float of
// that range: exhaustive check, scripts/check_sqrt.hip).
__device__ __forceinline__ float sqrt_rn_normal(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const int si = __builtin_bit_cast(int, s);
    const float sm = __builtin_bit_cast(float, si - 1);
    const float sp = __builtin_bit_cast(float, si + 1);
    float r = __builtin_fmaf(-sm, s, x) <= 0.0f ? sm : s;
    r = __builtin_fmaf(-sp, s, x) > 0.0f ? sp : r;
    return r;
}

// MainState.cpp:300-327 on SphRec, per row: t0 = tca - thc.  dist2 > r2 (a
// miss, :314) makes arg = r2 - dist2 < 0 (the sign of a difference of
// floats is exact), so thc and t0 are NaN and `t0 < closest` fails: the
// miss test needs no compare of its own.  A NaN dist2 gives a NaN t0 too.
__device__ __forceinline__ void sph_rows(const SphRec& s, unsigned bits, const float* pxf,
                                         const float* pyf, float* t) {
    float arg[kRowsPerLane];
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
        const float lx = s.cx - pxf[kStepsX == 1 ? 0 : j];
        const float lx2 = lx * lx;
        const float ly = s.cy - pyf[j];
        const float a = lx2 + ly * ly;
        const float dist2 = (a + s.kzw) - s.tca2;
        arg[j] = s.r2 - dist2;
    }
    // per sphere (scalar, branched once): the general sqrtf only where a
    // hitting lane's argument could leave the range sqrt_rn_normal is exact on
    if (!(s.fast != 0.0f)) {
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) t[j] = s.tca - sqrtf(arg[j]);
    } else {
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) t[j] = s.tca - sqrt_rn_normal(arg[j]);
    }
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j)  // t0 == 0 never takes; block kept (uniform)
        t[j] = (t[j] != 0.0f) && ((bits >> (2 * row_block(j))) & 1u) ? t[j] : __builtin_nanf("");
}

// Tile classification of one candidate against the rectangle
// [x0, x0+kW-1] x [y0, y0+kH-1] (fp32, conservative; see Cls).
template <int kWpx = kWaveTile, int kHpx = kWaveTileH>
__device__ __forceinline__ void classify(const Cls& k, bool is_tri, float x0, float y0,
                                         bool* keep, bool* inside) {
    constexpr float kW = (float)(kWpx - 1), kH = (float)(kHpx - 1);
    if (is_tri) {
        const float xl = x0 - k.a.x, xh = (x0 + kW) - k.a.x;
        const float yl = y0 - k.a.y, yh = (y0 + kH) - k.a.y;
        const float u1 = k.a.z * xl, u2 = k.a.z * xh, u3 = k.a.w * yl, u4 = k.a.w * yh;
        const float v1 = k.b.x * xl, v2 = k.b.x * xh, v3 = k.b.y * yl, v4 = k.b.y * yh;
        const float umin = fminf(u1, u2) + fminf(u3, u4), umax = fmaxf(u1, u2) + fmaxf(u3, u4);
        const float vmin = fminf(v1, v2) + fminf(v3, v4), vmax = fmaxf(v1, v2) + fmaxf(v3, v4);
        const float g = k.b.z;
        const bool out = umax < -g || umin > 1.0f + g || vmax < -g || vmin > 1.0f + g ||
                         umin + vmin > 1.0f + g;
        *keep = !out;
        *inside = umin > g && umax < 1.0f - g && vmin > g && vmax < 1.0f - g &&
                  umax + vmax < 1.0f - g;
    } else {
        const float dx = fmaxf(fmaxf(x0 - k.a.x, k.a.x - (x0 + kW)), 0.0f);
        const float dy = fmaxf(fmaxf(y0 - k.a.y, k.a.y - (y0 + kH)), 0.0f);
        *keep = !(dx * dx + dy * dy > k.a.z);
        *inside = false;
    }
}

// Pixel value of the Texture format (MainState.cpp:1026-1036), int32x4, or
// the rt_hit words of hit_pixel.
template <int kFmt>
__device__ __forceinline__ void store_fmt(void* __restrict__ out, int64_t idx, int4v pix) {
    if (kFmt == RT_FORMAT_I32X4)
        reinterpret_cast<int4v*>(out)[idx] = pix;
    else if (kFmt == RT_FORMAT_HIT)
        store_hit(out, idx, pix);
    else
        reinterpret_cast<unsigned*>(out)[idx] = pack_rgba8(pix);
}

// The same for shade_pixels' output: RGBA8 words arrive packed in pix.x.
// Nontemporal frame stores (per build, RT_NT_STORES, set by rt_device.hip
// for each inclusion; per format below): the wide build's frames (>= 512 MiB)
// drain faster with them (config 5 dense trace 733 -> 695 us, its RGBA8 form
// 478 -> 376 us, config 4 191 -> 186-187 us), and so do the 16x16 build's
// RGBA8 frames (config 3 29.0 -> 28.6 us, config 4 77.1 -> 75.7 us); its
// int32x4 frames are much slower with them (config 3 44.0 -> 54.9 us;
// DESIGN.md §3.5).
constexpr bool kNtI32 = (RT_NT_STORES & 1) != 0;
constexpr bool kNtRgba8 = (RT_NT_STORES & 2) != 0;
// RT_FORMAT_HIT frames (8-byte pixels): bit 2 (DESIGN.md §3.5)
constexpr bool kNtHit = (RT_NT_STORES & 4) != 0;
typedef unsigned uint2v __attribute__((ext_vector_type(2)));
// The cache-policy bits (the raw buffer store's aux operand on gfx950: bit 0
// sc0, bit 1 nt, bit 4 sc1) of a format's frame stores under a store policy
// (rt_dispatch.h: RT_STORE_DEFAULT = this build's choice above,
// RT_STORE_LARGE = the frames in flight have outgrown what the last-level
// cache absorbs).  Under RT_STORE_LARGE int32x4 frames are stored nt sc1,
// nontemporal and written through, so no dirty line stays behind in an L2 for
// a later store to push out: of the eight combinations of the three bits it
// and nt sc0 sc1 alone gain in the two-buffer frame loop (config 3, 2 frames
// in flight: 45.7 -> 42.7 us per frame, nt alone 45.6; config 4's one 1 GiB
// frame 193.9 -> 184.6, nt alone the same 194.0), and on one 256 MiB buffer
// written over and over it loses (50.6 -> 53.3), hence the policy
// (profiles/store_policy/README.md).  RGBA8 frames measured fastest with nt
// alone (4 in flight: nt 25.8, nt sc1 26.5, plain 27.9) and HIT frames keep
// it.  Two policies with equal bits share one kernel instance.
constexpr int kAuxNt = 2, kAuxSc1 = 16;
constexpr int store_aux(int fmt, int policy) {
    return policy == RT_STORE_LARGE
               ? (fmt == RT_FORMAT_I32X4 ? kAuxNt | kAuxSc1 : kAuxNt)
           : (fmt == RT_FORMAT_I32X4 ? kNtI32 : fmt == RT_FORMAT_HIT ? kNtHit : kNtRgba8) ? kAuxNt
                                                                                          : 0;
}
// (raw buffer stores: the tile origin in a buffer descriptor, the lane's
// 32-bit byte offset in a VGPR, the row's byte step as the scalar offset)
template <int kFmt, int kAux>
__device__ __forceinline__ void store_shaded(__amdgpu_buffer_rsrc_t tile, unsigned lane_off,
                                             int row_off, int4v pix) {
    if (kFmt == RT_FORMAT_I32X4)
        __builtin_amdgcn_raw_buffer_store_b128(pix, tile, (int)lane_off, row_off, kAux);
    else if (kFmt == RT_FORMAT_HIT)
        __builtin_amdgcn_raw_buffer_store_b64(uint2v{(unsigned)pix.x, (unsigned)pix.y}, tile,
                                              (int)lane_off, row_off, kAux);
    else
        __builtin_amdgcn_raw_buffer_store_b32(pix.x, tile, (int)lane_off, row_off, kAux);
}

// The Texture packing (MainState.cpp:1026-1036) of three (int) channels.
// Two v_perm_b32 (selector bytes 0-3 pick the second operand's bytes, 4-7
// the first's, 12 gives 0x00 and 13 gives 0xFF): r0 g0 . . then r0 g0 b0 FF.
__device__ __forceinline__ unsigned pack_bytes(int r, int g, int b) {
    const unsigned rg = __builtin_amdgcn_perm((unsigned)g, (unsigned)r, 0x0c0c0400u);
    return __builtin_amdgcn_perm((unsigned)b, rg, 0x0d040100u);
}

// Shade (MainState.cpp:396-407) one lane's kRowsPerLane pixels.  Int32x4:
// pix[j] is the pixel.  RGBA8: pix[j].x is the packed Texture word.
// RT_FORMAT_HIT: no shade at all, pix[j] is hit_pixel: the walk's closest[j]
// and hit[j] as they stand (every walk starts them at kFar / -1 and
// take_rows only ever writes a slot >= 0 beside a t < closest, so a miss is
// {kFar, -1} and nothing else).
template <int kMode = 0, int kFmt = RT_FORMAT_I32X4>
__device__ __forceinline__ void shade_pixels(const float4* __restrict__ colours,
                                             const float* closest, const int* hit, int4v* pix) {
    if (kFmt == RT_FORMAT_HIT) {
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) pix[j] = hit_pixel(closest[j], hit[j]);
        return;
    }
    bool lane_hit = false;
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) lane_hit |= hit[j] >= 0;
    const bool any_hit = __ballot(lane_hit) != 0ull;
    if (kFmt == RT_FORMAT_RGBA8) {
        // The Texture keeps the low byte of each (int) channel.  x86's (int)
        // gives INT32_MIN (low byte 0) for NaN, +-inf and |f| >= 2^31;
        // v_cvt_i32_f32 agrees on that byte except for f >= 2^31 (it
        // saturates to 0x7fffffff), so one wave-uniform max3 test replaces
        // the per-channel fix-ups of cvt_i32_fast on the common path.
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) pix[j].x = (int)0xFF000000u;
        if (!any_hit) return;
        float4 col[kRowsPerLane];
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j)
            col[j] = kMode == 4 ? make_float4(1.0f, 0.5f, 0.25f, 255.0f)
                                : colours[hit[j] >= 0 ? hit[j] : 0];
        float f[kRowsPerLane][3];
        bool big = false;
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) {
            // a lane without a hit shades kFar (discarded below): on div180's
            // fast path like every hit
            const float normalised = div180(closest[j]);
            const float scalar = 255.0f - (normalised * 255.0f);
            f[j][0] = scalar * col[j].x;
            f[j][1] = scalar * col[j].y;
            f[j][2] = scalar * col[j].z;
            big |= !(fmaxf(fmaxf(f[j][0], f[j][1]), f[j][2]) < 2147483648.0f);
        }
        if (__ballot(big)) {
#pragma unroll
            for (int j = 0; j < kRowsPerLane; ++j) {
                const unsigned w = pack_bytes(cvt_i32_fast(f[j][0]), cvt_i32_fast(f[j][1]),
                                              cvt_i32_fast(f[j][2]));
                pix[j].x = hit[j] >= 0 ? (int)w : pix[j].x;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kRowsPerLane; ++j) {
                int c[3];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    asm volatile("v_cvt_i32_f32 %0, %1" : "=v"(c[k]) : "v"(f[j][k]));
                const unsigned w = pack_bytes(c[0], c[1], c[2]);
                pix[j].x = hit[j] >= 0 ? (int)w : pix[j].x;
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) pix[j] = int4v{0, 0, 0, 255};
    if (!any_hit) return;
    float4 col[kRowsPerLane];
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j)  // kMode 4: no gather (diagnostics)
        col[j] = kMode == 4 ? make_float4(1.0f, 0.5f, 0.25f, 255.0f)
                            : colours[hit[j] >= 0 ? hit[j] : 0];
    // x86's (int) and v_cvt_i32_f32 agree except on NaN (INT32_MIN vs 0) and
    // f >= 2^31 (INT32_MIN vs INT32_MAX): one wave-uniform test picks the
    // raw converts, the per-channel fix-ups (cvt_i32_fast) run only when some
    // lane needs them.  Lanes without a hit shade kFar (discarded): on
    // div180's fast path like every hit.
    float f[kRowsPerLane][3];
    bool fix = false;
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
        const float normalised = div180(closest[j]);
        const float scalar = 255.0f - (normalised * 255.0f);
        f[j][0] = scalar * col[j].x;
        f[j][1] = scalar * col[j].y;
        f[j][2] = scalar * col[j].z;
        fix |= !(fmaxf(fmaxf(f[j][0], f[j][1]), f[j][2]) < 2147483648.0f) |
               __builtin_isunordered(f[j][0], f[j][1]) | __builtin_isunordered(f[j][2], f[j][2]);
    }
    if (__ballot(fix)) {
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) {
            const int4v c{cvt_i32_fast(f[j][0]), cvt_i32_fast(f[j][1]), cvt_i32_fast(f[j][2]), 255};
            pix[j] = hit[j] >= 0 ? c : pix[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) {
            int c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                asm volatile("v_cvt_i32_f32 %0, %1" : "=v"(c[k]) : "v"(f[j][k]));
            pix[j] = hit[j] >= 0 ? int4v{c[0], c[1], c[2], 255} : pix[j];
        }
    }
}

// Store one lane's kRowsPerLane shaded pixels (pix_dx / pix_dy apart) of the
// wave tile at (rel_x, rel_y) of the band (rows from the band's first), in
// the Texture format (MainState.cpp:1026-1036, packed by shade_pixels),
// int32x4 or rt_hit.  Each row's address is a wave-uniform base (SGPRs: the tile
// origin plus the row's step) and the lane's 32-bit byte offset, so the
// stores take the saddr + voffset form with no per-pixel 64-bit address
// arithmetic (round 4).  `full`: the whole tile lies inside the frame band,
// so no per-lane bounds checks.
template <int kMode, int kFmt, int kAux = store_aux(kFmt, RT_STORE_DEFAULT)>
__device__ __forceinline__ void store_rows(const int4v* pix, int rel_x, int rel_y, int lane,
                                           int width, int band_h, bool full,
                                           void* __restrict__ out) {
    constexpr int kBytes = (int)rt_args::pixel_bytes(kFmt);
    const int lx = lane % kLanesX, ly = lane / kLanesX;
    // ly * width as a 24-bit multiply (width <= 2^24, so width - 1 fits)
    const unsigned lane_off =
        (__umul24((unsigned)ly, (unsigned)(width - 1)) + (unsigned)(ly + lx)) * (unsigned)kBytes;
    char* const origin = static_cast<char*>(out) + ((int64_t)rel_y * width + rel_x) * kBytes;
    // (0x00020000: the gfx9 raw-buffer format word; the range is never the
    // limit, the exec mask below is)
    const __amdgpu_buffer_rsrc_t tile =
        __builtin_amdgcn_make_buffer_rsrc(origin, (short)0, (int)0xffffffff, 0x00020000);
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
        // kMode 3: everything but the stores (a store the compiler cannot drop)
        const bool store = kMode != 3 || pix[j].x == 0x7fffffff;
        const int row_off = (pix_dy(j) * width + pix_dx(j)) * kBytes;
        const bool in = full || (rel_x + lx + pix_dx(j) < width && rel_y + ly + pix_dy(j) < band_h);
        if (in && store) store_shaded<kFmt, kAux>(tile, lane_off, row_off, pix[j]);
    }
}

// Tiles of one coarse bin: kCoarseW / kWaveTile x kCoarseH / kWaveTileH.
constexpr int kTilesX = kCoarseW / kWaveTile;
constexpr int kTilesY = kCoarseH / kWaveTileH;
constexpr int kTiles = kTilesX * kTilesY;
// tile words per candidate: kTileBits per tile, kTilesPerWord tiles a word
constexpr int kTmWords = (kTiles + kTilesPerWord - 1) / kTilesPerWord;
// ints per candidate slot of a coarse-bin list: the id, then the tile words
constexpr int kListStride = 1 + kTmWords;
static_assert(kTiles <= 16 && kTmWords <= 4, "tile words");

// Coarse binning with per-block classification: one wave per coarse bin.
// counts[cb] = -1 flags a frame whose scene data is not finite (prep's
// generation-stamped flag): the trace then runs the reference verbatim.
// (1) the ids whose box touches the coarse bin are compacted, in primitive
// order, into LDS (rounds of kRound); (2) the (candidate, tile) pairs are
// spread over the lanes, 16 lanes per candidate, each testing box overlap +
// classifier for every row block of its tile and OR-ing the bits (per
// block b: bit 2b keep, bit 2b+1 inside) into the candidate's LDS tile word;
// (3) candidates kept by some block are appended in order.  Output:
// counts[cb]; at lists + cb * kListStride * half_cap: half_cap ids, then
// tile word w of every candidate at [(1 + w) * half_cap ...].
#ifndef RT_C3_ROUND
#define RT_C3_ROUND 64
#endif
#ifndef RT_C3_BATCH
#define RT_C3_BATCH 8
#endif
constexpr int kRound = RT_C3_ROUND;
static_assert(kTmWords == 1, "coarse depth cull: one tile word per candidate");
#ifndef RT_COARSE_WAVES
#define RT_COARSE_WAVES 6  // amdgpu_waves_per_eu floor for coarse3_kernel (0 = none): 80 VGPRs, 6 waves/SIMD (86 and 5 without; config 3 -0.4 us, config 5 dense -1.3%)
#endif
#if RT_COARSE_WAVES > 0
#define RT_COARSE_ATTR __attribute__((amdgpu_waves_per_eu(RT_COARSE_WAVES)))
#else
#define RT_COARSE_ATTR
#endif

// Coarse depth cull (`cull`): an upper bound on every pixel's final closest
// per wave tile, from the spheres that provably hit the WHOLE tile.  The
// trace computes, per pixel, dist2 = ((lx*lx + ly*ly) + kzw) - tca2 with
// lx = cx - x, ly = cy - y, then t0 = tca - sqrtf(r2 - dist2) (sph_rows);
// every step is monotone under IEEE rounding, and |lx|, |ly| are largest at
// a tile edge, so the same operations on the tile's extreme |lx|, |ly| give
// dist2max >= dist2 and T = tca - sqrtf(r2 - dist2max) >= t0 at every pixel
// of the tile (exactly, no margin).  If dist2max <= r2 every pixel hits
// the sphere, and if t0 != 0 is guaranteed too (T < 0, or prep's lower
// bound tmin > 0) every pixel's closest ends <= T.  A sphere whose lower
// bound tmin is STRICTLY greater than the tile's smallest T then never wins
// a pixel of the tile (not even a tie: MainState.cpp:386-391 keeps the
// first of equal t), so its tile bits are cleared, and a candidate no tile
// keeps leaves the list.
// One-sided bounds of the correctly rounded sqrtf (x >= 0): v_sqrt_f32 is
// within 1 ulp of it on [2^-96, 2^126] (sqrt_rn_normal's +-1 ulp fix-up is
// exhaustively exact there, scripts/check_sqrt.hip), so +-2 ulp brackets it.
__device__ __forceinline__ float sqrt_lo_bound(float x) {  // <= sqrtf(x)
    if (!(x >= 0x1p-96f)) return 0.0f;
    if (!(x <= 0x1p126f)) return 0x1p63f;
    return __builtin_bit_cast(float, __builtin_bit_cast(int, __builtin_amdgcn_sqrtf(x)) - 2);
}
__device__ __forceinline__ float sqrt_hi_bound(float x) {  // >= sqrtf(x)
    if (!(x >= 0x1p-96f)) return 0x1p-48f;
    if (!(x <= 0x1p126f)) return INFINITY;
    return __builtin_bit_cast(float, __builtin_bit_cast(int, __builtin_amdgcn_sqrtf(x)) + 2);
}

// Upper bound (order key) of t0 over every pixel of the tile at (tx, ty),
// when the sphere provably hits all of them with t0 != 0; else ~0u.
__device__ __forceinline__ unsigned tile_cover_key(const SphRec& r, int tx, int ty) {
    const float xa = (float)tx, xb = (float)(tx + kWaveTile - 1);
    const float ya = (float)ty, yb = (float)(ty + kWaveTileH - 1);
    const float mx = fmaxf(fabsf(r.cx - xa), fabsf(r.cx - xb));
    const float my = fmaxf(fabsf(r.cy - ya), fabsf(r.cy - yb));
    const float a = (mx * mx) + (my * my);
    const float dist2 = (a + r.kzw) - r.tca2;
    if (!(dist2 <= r.r2)) return 0xffffffffu;  // some pixel may miss (or NaN)
    const float t = r.tca - sqrt_lo_bound(r.r2 - dist2);
    const bool nonzero = t < 0.0f || (t == t && r.tmin_key > order_key(0.0f));
    return nonzero ? order_key(t) : 0xffffffffu;
}

// Lower bound (order key) of t0 over the pixels of the tile at (tx, ty)
// that can hit the sphere: the same monotone operations on the tile's
// smallest |lx|, |ly| (0 when the centre's coordinate lies inside the
// tile's span) bound dist2 from below, so r2 - dist2 and thc from above.
// ~0u: no pixel of the tile hits (dist2 > r2 everywhere); 0: no bound.
__device__ __forceinline__ unsigned rect_low_key(const SphRec& r, float xa, float xb, float ya,
                                                 float yb) {
    const float lxa = r.cx - xa, lxb = r.cx - xb;  // lxa >= lxb
    const float lya = r.cy - ya, lyb = r.cy - yb;
    const float mx = (lxa >= 0.0f && lxb <= 0.0f) ? 0.0f : fminf(fabsf(lxa), fabsf(lxb));
    const float my = (lya >= 0.0f && lyb <= 0.0f) ? 0.0f : fminf(fabsf(lya), fabsf(lyb));
    const float a = (mx * mx) + (my * my);
    const float dist2 = (a + r.kzw) - r.tca2;
    if (dist2 > r.r2) return 0xffffffffu;
    const float t = r.tca - sqrt_hi_bound(r.r2 - dist2);
    return t == t ? order_key(t) : 0u;
}
__device__ __forceinline__ unsigned tile_low_key(const SphRec& r, int tx, int ty) {
    return rect_low_key(r, (float)tx, (float)(tx + kWaveTile - 1), (float)ty,
                        (float)(ty + kWaveTileH - 1));
}

// Triangles join the depth cull through tri_t_bounds: a triangle whose tile
// classifier proved the tile fully inside it (every pixel passes u/v) gives
// the cover bound (float)hi; a triangle whose (float)lo strictly exceeds the
// tile's cover bound leaves the tile, exactly like a sphere.
__device__ __forceinline__ unsigned tri_cover_key(const TriDepth& r, int tx, int ty) {
    double lo, hi;
    if (!tri_t_bounds(r, (double)tx, (double)(tx + kWaveTile - 1), (double)ty,
                      (double)(ty + kWaveTileH - 1), &lo, &hi))
        return 0xffffffffu;
    return order_key((float)hi);
}
// The same lower bounds over a whole coarse bin (pixels [xa, xb] x [ya, yb]):
// no larger than over any of its tiles, so exceeding every tile's cover
// takes the candidate out of all of them at once.
__device__ __forceinline__ unsigned tri_rect_low_key(const TriDepth& r, int xa, int xb, int ya,
                                                     int yb) {
    double lo, hi;
    if (!tri_t_bounds(r, (double)xa, (double)xb, (double)ya, (double)yb, &lo, &hi)) return 0u;
    return order_key((float)lo);
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ unsigned tri_low_key(const TriDepth& r, int tx, int ty) {
    double lo, hi;
    if (!tri_t_bounds(r, (double)tx, (double)(tx + kWaveTile - 1), (double)ty,
                      (double)(ty + kWaveTileH - 1), &lo, &hi))
        return 0u;
    return order_key((float)lo);
}

// The coarse binning of ONE bin `cb` by kW waves (wave `wave`, lane `lane`):
// candidates (bin masks, or a scan of every box), per-tile classification,
// depth cull, the list and counts[cb].  Boxes, classifiers, sphere records and
// triangle depth models come from global memory, staged per round into the
// workgroup's LDS.  With kW > 1 (bands of few bins, round 4) the waves share
// every (candidate, tile) pair loop and the staging loads; the candidate
// order, counts and gates are computed by every wave alike from the same
// LDS data, and wave 0 alone writes the shared staging slots and the list.
template <int kW>
__device__ __forceinline__ void coarse_bin(
    int cb, int wave, int lane, const int4* __restrict__ boxes, const Cls* __restrict__ cls,
    const SphRec* __restrict__ sph, const TriDepth* __restrict__ tri, int n_prims, int n_tri,
    int n_cx, const unsigned long long* __restrict__ row_masks,
    const unsigned long long* __restrict__ col_masks, int row_begin, int half_cap,
    bool nonfinite, unsigned long long od, unsigned long long overdraw_min, int cull_min,
    int cull_min_all, int* __restrict__ counts, int* __restrict__ lists, int* s_ids,
    SphRec* s_sph, unsigned* s_tkey, int* s_sidx, unsigned* s_tm, unsigned char* s_raw) {
    int4* const s_box = reinterpret_cast<int4*>(s_raw);
    Cls* const s_cls = reinterpret_cast<Cls*>(s_raw + kRound * sizeof(int4));
    TriDepth* const s_tri = reinterpret_cast<TriDepth*>(s_raw);
    const int x0 = (cb % n_cx) * kCoarseW, x1 = x0 + kCoarseW - 1;
    const int y0 = row_begin + (cb / n_cx) * kCoarseH, y1 = y0 + kCoarseH - 1;
    // (kW == 1: the wave's own barrier; the compiler folds wave to 0)
    if (kW == 1) wave = 0;
    const bool w0 = wave == 0;
    auto sync = [&]() {
        if (kW == 1) {
            __builtin_amdgcn_wave_barrier();
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
        } else {
            __syncthreads();
        }
    };
    const int wl = 64 * wave + lane;  // this lane's slot in the workgroup's pair loops
    int* out_id = lists + (int64_t)cb * kListStride * half_cap;
    int* out_tm = out_id + half_cap;
    int count = 0;   // appended to the output
    int staged = 0;  // ids in s_ids
    int pairs = 0;   // this lane's kept (candidate, tile) pairs, for the triangle gate
    if (w0 && lane < kTiles) s_tkey[lane] = 0xffffffffu;
    // the depth cull runs in bins with at least cull_min sphere candidates
    // (0: never); triangles take part in frames whose boxes cover the frame
    // at least RT_COARSE_CULL_OVERDRAW times (the trace is then bound by its
    // tests, not its stores) and, there, in bins whose tiles keep at least
    // cull_min_all candidates each on average (their depth complexity,
    // counted once every candidate is classified; 0: never)
    bool cull = false, cull_tri = false;
    int n_sph_cand = 0;  // sphere candidates among the first 4096 primitives (box-scan gate)
    constexpr int kBatch = RT_C3_BATCH;
    // candidate c's data, staged in this wave's LDS slice
    auto box_c = [&](int c) -> int4 { return s_box[c]; };
    auto cls_c = [&](int c) -> Cls { return s_cls[c]; };
    auto sph_c = [&](int c) -> SphRec { return s_sph[c]; };
    auto tri_c = [&](int c) -> TriDepth { return s_tri[c]; };
    auto classify_round = [&](int n) {
        sync();
        // each candidate's box and classifier into LDS once
        for (int e = wl; e < n; e += 64 * kW) {
            const int id = s_ids[e];
#pragma unroll
            for (int w = 0; w < kTmWords; ++w) s_tm[e * kTmWords + w] = 0u;
            s_box[e] = boxes[id];
            s_cls[e] = cls[id];
        }
        sync();
        for (int q0 = 64 * wave; q0 < n * kTiles; q0 += 64 * kW) {
            const int q = q0 + lane;
            if (q < n * kTiles) {
                const int c = q / kTiles, t = q % kTiles;
                const bool is_tri = s_ids[c] < n_tri;
                const int4 pb = box_c(c);
                const int tx = x0 + (t % kTilesX) * kWaveTile;
                const int ty = y0 + (t / kTilesX) * kWaveTileH;
                unsigned bits = 0u;
                bool keep = false, inside = false;
                if (pb.x <= tx + kWaveTile - 1 && pb.z >= tx && pb.y <= ty + kWaveTileH - 1 &&
                    pb.w >= ty)
                    classify(cls_c(c), is_tri, (float)tx, (float)ty, &keep, &inside);
                if (keep) bits = inside ? kTileMask : kKeepMask;
#if RT_ROWBITS == 1
                // a triangle's partial tile: classify each row block
                if (kBlocks > 1 && is_tri && keep && !inside) {
                    bits = 0u;
#pragma unroll
                    for (int b = 0; b < kBlocks; ++b) {
                        const int by = ty + b * kBlockH;
                        bool bk = false, bi = false;
                        if (pb.y <= by + kBlockH - 1 && pb.w >= by)
                            classify<kWaveTile, kBlockH>(cls_c(c), true, (float)tx, (float)by, &bk, &bi);
                        bits |= ((bk ? 1u : 0u) | (bk && bi ? 2u : 0u)) << (2 * b);
                    }
                }
#endif
                if (bits)
                    atomicOr(&s_tm[c * kTmWords + t / kTilesPerWord],
                             bits << (kTileBits * (t % kTilesPerWord)));
            }
        }
        sync();
        for (int e0 = 0; e0 < n; e0 += 64) {
            const int e = e0 + lane;
            unsigned tm[kTmWords];
            bool any = false;
#pragma unroll
            for (int w = 0; w < kTmWords; ++w) {
                tm[w] = e < n ? s_tm[e * kTmWords + w] : 0u;
                any |= tm[w] != 0u;
            }
            const unsigned long long m2 = __ballot(any);
            if (any) pairs += __popc(tm[0] & 0x55555555u);  // every tile's keep bit
            if (any && w0) {
                const int pos = count + (int)__builtin_amdgcn_mbcnt_hi(
                    (unsigned)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m2, 0u));
                out_id[pos] = s_ids[e];
#pragma unroll
                for (int w = 0; w < kTmWords; ++w) out_tm[w * half_cap + pos] = (int)tm[w];
            }
            count += __popcll(m2);
        }
        sync();
    };
    // Stage the overlapping ids in primitive order (rounds of kRound).
    auto stage = [&](unsigned long long m, int chunk_base) {
        const int n_ov = __popcll(m);
        if (n_ov == 0) return;
        if (staged + n_ov > kRound) {
            classify_round(staged);
            staged = 0;
        }
        if (!row_masks && chunk_base < 64 * 64) {
            // sphere bits of this chunk, among the first 4096 primitives:
            // the same count the bin-mask path's gate takes (below)
            const int first = n_tri - chunk_base;
            n_sph_cand += __popcll(first <= 0 ? m : first >= 64 ? 0ull : m & (~0ull << first));
        }
        if (w0 && ((m >> lane) & 1ull)) {
            const unsigned below = __builtin_amdgcn_mbcnt_hi(
                (unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            s_ids[staged + (int)below] = chunk_base + lane;
        }
        staged += n_ov;
    };
    const int n_chunks = (n_prims + 63) / 64;
    if (row_masks) {
        // candidates = this bin row's chunk words AND this bin column's
        const unsigned long long* rw = row_masks + (int64_t)(cb / n_cx) * n_chunks;
        const unsigned long long* cw = col_masks + (int64_t)(cb % n_cx) * n_chunks;
        // lane l loads chunk c0 + l's two words; the nonzero chunks are
        // staged in order
        for (int c0 = 0; c0 < n_chunks; c0 += 64) {
            const int c = c0 + lane;
            const unsigned long long w = c < n_chunks ? rw[c] & cw[c] : 0ull;
            if (c0 == 0 && cull_min > 0) {
                // the gate: sphere candidates (ids >= n_tri) among the first
                // 4096 primitives, popcounts summed over the wave
                const int first = n_tri - 64 * c;
                const unsigned long long sph_bits =
                    first <= 0 ? ~0ull : first >= 64 ? 0ull : ~0ull << first;
                cull = (int)wave_sum((unsigned)__popcll(w & sph_bits)) >= cull_min;
            }
            // the 64 chunk words' candidates all fit in this round: each lane
            // places its own word's ids at its prefix-sum offset (primitive
            // order: lanes in chunk order, bits ascending)
            {
                const unsigned cnt = (unsigned)__popcll(w);
                const unsigned incl = wave_prefix_sum(cnt);
                const int total = __builtin_amdgcn_readlane((int)incl, 63);
                if (staged + total <= kRound) {
                    int pos = staged + (int)(incl - cnt);
                    unsigned long long m = w0 ? w : 0ull;
                    while (m) {
                        s_ids[pos++] = c * 64 + __builtin_ctzll(m);
                        m &= m - 1ull;
                    }
                    staged += total;
                    continue;
                }
            }
            unsigned long long nz = __ballot(w != 0ull);
            while (nz) {
                const int l = __builtin_ctzll(nz);
                nz &= nz - 1ull;
                const unsigned long long m =
                    (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)w, l) |
                    ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(w >> 32), l) << 32);
                stage(m, (c0 + l) * 64);
            }
        }
    } else {
        // (the sphere gate is set after the scan, from its sphere count)
        cull_tri = false;
        // scan every box (frames with too many bin rows + columns for masks)
        for (int base = 0; base < n_prims; base += 64 * kBatch) {
            int4 bb[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const int e = base + 64 * k + lane;
                bb[k] = e < n_prims ? boxes[e]
                                    : make_int4(1 << 30, 1 << 30, -(1 << 30), -(1 << 30));
            }
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const int4 q = bb[k];
                stage(__ballot(q.x <= x1 && q.z >= x0 && q.y <= y1 && q.w >= y0), base + 64 * k);
            }
        }
    }
    if (staged) classify_round(staged);
    if (!row_masks) cull = cull_min > 0 && n_sph_cand >= cull_min;
    // the triangle gate: kept (candidate, tile) pairs per tile, on average
    if (cull_min_all > 0 && count > 0 && od >= overdraw_min) {
        cull_tri = (int)wave_sum((unsigned)pairs) >= cull_min_all * kTiles;
    }
    // Depth cull (see tile_cover_key): once every candidate of the bin has
    // been classified, drop each sphere's (and, with cull_tri, triangle's)
    // tiles whose cover bound its tile-local lower bound strictly exceeds,
    // and compact the list in place (in order: a kept entry only moves
    // down, past entries this wave has already read).
    if constexpr (kTmWords == 1 && kBlocks == 1) {
    if ((cull || cull_tri) && count > 0) {
        sync();
        // the list this wave wrote is read back: its own stores are ordered
        // before the loads by a workgroup-scope fence (a wave is its own
        // workgroup here; agent scope would write back L2)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        // The list is walked 64 entries at a time: each lane stages one
        // entry's id, tile word and record in LDS, then the entries'
        // (entry, tile) pairs are spread over the lanes.
        auto stage_chunk = [&](int e0) {
            const int e = e0 + lane;
            if (w0) {  // (wave 0 wrote the list: it reads it back)
                int id = -1;
                unsigned tm = 0u;
                if (e < count) {
                    id = out_id[e];
                    tm = (unsigned)out_tm[e];
                    if (id >= n_tri) s_sph[lane] = sph[id - n_tri];
                    else if (cull_tri) s_tri[lane] = tri[id];
                }
                s_ids[lane] = id;
                s_tm[lane] = tm;
            }
            sync();
        };
        // triangles proved to cover a whole tile (both bits) bound it; so do
        // spheres when the sphere gate did not already have the
        // classification pass compute theirs
        auto cover_chunk = [&](int n) {
            for (int q = wl; q < n * kTiles; q += 64 * kW) {
                const int c = q / kTiles, t = q % kTiles;
                const unsigned bits = s_tm[c] >> (kTileBits * t) & kTileMask;
                const int cid = s_ids[c];
                if (!bits) continue;
                const int tx = x0 + (t % kTilesX) * kWaveTile;
                const int ty = y0 + (t / kTilesX) * kWaveTileH;
                unsigned key = 0xffffffffu;
                if (cid < n_tri) {
                    if (cull_tri && bits == kTileMask) key = tri_cover_key(tri_c(c), tx, ty);
                } else {
                    key = tile_cover_key(sph_c(c), tx, ty);
                }
                if (key != 0xffffffffu) atomicMin(&s_tkey[t], key);
            }
            sync();
        };
        const bool one = count <= 64;
        // the cover pass (always for triangles; for spheres too unless the
        // classification computed their covers)
        const bool cover_pass = cull_tri || cull;
        if (cover_pass) {
            for (int e0 = 0; e0 < count; e0 += 64) {
                stage_chunk(e0);
                cover_chunk(min(64, count - e0));
            }
        }
        const unsigned own = lane < kTiles ? s_tkey[lane] : 0xffffffffu;
        if (__ballot(own != 0xffffffffu)) {
            // the largest tile cover; ~0u while some tile has none (then no
            // candidate can leave every tile)
            const unsigned max_t = wave_max_u32(lane < kTiles ? own : 0u);
            int kept = 0;
            for (int e0 = 0; e0 < count; e0 += 64) {
                const int n = min(64, count - e0);
                const int e = e0 + lane;
                if (!(one && cover_pass)) stage_chunk(e0);  // (one chunk: still staged)
                const int id = s_ids[lane];
                // a candidate whose lower bound over the whole bin exceeds
                // every tile's cover leaves all of its tiles at once; the
                // others go through the tiles one by one
                bool all_out = false;
                if (RT_BIN_DROP && max_t != 0xffffffffu && lane < n) {
                    if (id >= n_tri)
                        all_out = rect_low_key(sph_c(lane), (float)x0, (float)x1, (float)y0,
                                               (float)y1) > max_t;
                    else if (cull_tri)
                        all_out = tri_rect_low_key(tri_c(lane), x0, x1, y0, y1) > max_t;
                }
                const unsigned long long surv = __ballot(lane < n && !all_out);
                // (no wave reads s_tm or s_sidx between the last barrier and the next)
                if (w0 && all_out) s_tm[lane] = 0u;
                if (w0 && ((surv >> lane) & 1ull))
                    s_sidx[__builtin_amdgcn_mbcnt_hi((unsigned)(surv >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((unsigned)surv, 0u))] =
                        lane;
                const int n_s = __popcll(surv);
                sync();
                // a candidate leaves a tile whose cover bound its tile-local
                // lower bound strictly exceeds
                for (int q = wl; q < n_s * kTiles; q += 64 * kW) {
                    const int c = s_sidx[q / kTiles], t = q % kTiles;
                    const unsigned tkey = s_tkey[t];
                    const int cid = s_ids[c];
                    if (cid >= 0 && (cid >= n_tri || cull_tri) && tkey != 0xffffffffu &&
                        ((s_tm[c] >> (kTileBits * t)) & 1u)) {
                        const int tx = x0 + (t % kTilesX) * kWaveTile;
                        const int ty = y0 + (t / kTilesX) * kWaveTileH;
                        const unsigned low = cid >= n_tri ? tile_low_key(sph_c(c), tx, ty)
                                                          : tri_low_key(tri_c(c), tx, ty);
                        if (low > tkey) atomicAnd(&s_tm[c], ~(kTileMask << (kTileBits * t)));
                    }
                }
                sync();
                const unsigned tm = s_tm[lane];
                sync();
                const bool any = e < count && tm != 0u;
                const unsigned long long m = __ballot(any);
                if (any && w0) {
                    const int pos = kept + (int)__builtin_amdgcn_mbcnt_hi(
                        (unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                    out_id[pos] = id;
                    out_tm[pos] = (int)tm;
                }
                kept += __popcll(m);
            }
            count = kept;
        }
    }
    }
    if (w0 && lane == 0) counts[cb] = nonfinite ? -1 : count;
}

template <int kW>
__global__ void __launch_bounds__(64 * kW) RT_COARSE_ATTR coarse3_kernel(
    const int4* __restrict__ boxes, const Cls* __restrict__ cls,
    const SphRec* __restrict__ sph, const TriDepth* __restrict__ tri, int n_prims, int n_tri,
    int n_cx, int n_coarse, const unsigned long long* __restrict__ row_masks,
    const unsigned long long* __restrict__ col_masks, int row_begin, int half_cap,
    const unsigned* __restrict__ nonfinite_flag, unsigned gen, int cull_min, int cull_min_all,
    const unsigned long long* __restrict__ overdraw, unsigned long long overdraw_min,
    unsigned long long* __restrict__ overdraw_next, int* __restrict__ counts,
    int* __restrict__ lists, unsigned long long od_lo, unsigned long long od_hi,
    unsigned* __restrict__ od_verdict) {
    // one workgroup of kW waves per bin (more bins per workgroup measured
    // slower, DESIGN.md §3.5; kW > 1: bands of few bins, round 4)
    const int cb = (int)blockIdx.x;
    const int wave = kW == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    (void)n_coarse;
    __shared__ int s_ids[kRound];
    __shared__ SphRec s_sph[kRound];
    __shared__ unsigned s_tkey[kTiles];  // per tile: smallest cover bound
    __shared__ int s_sidx[64];  // the depth cull's surviving entries of a chunk
    // read early (independent of the scan): a non-finite scene is handed to
    // the trace as count -1, so the trace's first scalar load tells it both
    const bool nonfinite = *nonfinite_flag == gen;
    // the triangle gate's frame half: the boxes' overdraw (prep_kernel)
    // (a vector load: as a scalar one, the first lgkmcnt wait for the kernel
    // arguments would also wait for it)
    const unsigned long long od =
        __hip_atomic_load(overdraw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    __shared__ unsigned s_tm[kRound * kTmWords];
    // the classification's boxes and classifiers, then (same LDS) the depth
    // cull's staged triangle models
    constexpr size_t kRawBytes = kRound * (sizeof(int4) + sizeof(Cls));
    static_assert(64 * sizeof(TriDepth) <= kRawBytes && sizeof(int4) % 16 == 0, "LDS alias");
    __shared__ alignas(16) unsigned char s_raw[kRawBytes];
    const int lane = threadIdx.x & 63;
    coarse_bin<kW>(cb, wave, lane, boxes, cls, sph, tri, n_prims, n_tri, n_cx, row_masks, col_masks,
                      row_begin, half_cap, nonfinite, od, overdraw_min, cull_min, cull_min_all,
                      counts, lists, s_ids, s_sph, s_tkey, s_sidx, s_tm, s_raw);
    // the other overdraw slot starts the next binned launch at zero (a
    // per-lane, i.e. vector, store; at the end, so no wave waits for its
    // address before its scan)
    if (cb == 0 && wave == 0 && lane == 0) {
        *overdraw_next = 0ull;
        // the frame's overdraw verdict for the host's path choice (the
        // host's mapped word, or device memory that launch() copies)
        store_verdict(od_verdict, od < od_lo ? 1u : od < od_hi ? 2u : 3u);
    }
}

#if RT_TRACE_WAVES > 0
#define RT_TRACE_ATTR __attribute__((amdgpu_waves_per_eu(RT_TRACE_WAVES)))
#else
#define RT_TRACE_ATTR
#endif

// Two candidate walks (round 6, interleaved A/B, DESIGN.md §3.5).
// trace3_kernel reads the bin's list in scalar batches of 8 and tests every
// entry's keep bit; trace3_split_kernel loads it as vectors, 64 entries a
// round, and visits only the entries its tile keeps (one keep ballot).  The
// ballot walk won on the small-frame split trace (11.9 -> 9.4 us, reference
// scene 3 at 640x480) and was flat to slower in the full-size trace3_kernel
// (int32x4 43.4 -> 44.1 us, config 5 dense RGBA8 366 -> 395).

// The walk's sphere depth cull: a sphere whose lower bound (SphRec::tmin_key)
// no lane's closest exceeds cannot be taken by any lane (strict <), so it is
// skipped.  The bound, refreshed lazily by each walk, is the wave-uniform
// order_key of the largest closest[] of the wave: per-lane max over its rows,
// then a DPP max to lane 63 (row_shr 1/2/4/8 within rows of 16, row_bcast
// 15/31 across them; shifted-in lanes read 0, the identity).
__device__ __forceinline__ unsigned wave_max_key(const float* closest) {
    float m = closest[0];
#pragma unroll
    for (int j = 1; j < kRowsPerLane; ++j) m = fmaxf(m, closest[j]);
    unsigned v = order_key(m);
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// What the five tile kernels below (trace3_kernel, trace3_split_kernel,
// trace_small_kernel, trace_bin_kernel, frame_small_kernel) have in common,
// as preprocessor text: the compiler gets the same tokens at the same place
// as from a copy in each kernel, so every kernel's instruction stream is what
// it was with the copies (profiles/walk_shared/).  As __forceinline__
// functions, in seven wordings, none of the three was codegen-neutral in
// these kernels at the 64-VGPR ceiling (DESIGN.md §3.5).  #undef first: this
// file is compiled once per tile build.

// Non-finite scene data: the reference algorithm verbatim for the lane's
// pixels (generic_kernel's collide_generic), one row at a time.  Which waves
// run it, and on what condition, is each kernel's own.
// Expects in scope: x, y0, width, row_begin, row_end, scene, dir, out, kFmt.
#undef RT_REFERENCE_PIXELS
#define RT_REFERENCE_PIXELS()                                                            \
    _Pragma("unroll 1") for (int j = 0; j < kRowsPerLane; ++j) {                         \
        const int xj = x + pix_dx(j), y = y0 + pix_dy(j);                                \
        if (xj < width && y < row_end)                                                   \
            store_fmt<kFmt>(                                                             \
                out, (int64_t)(y - row_begin) * width + xj,                              \
                collide_generic<kFmt>(scene, make_float4((float)xj, (float)y, 0.0f, 1.0f), \
                                      dir));                                             \
    }

// A lane's state for the walk: nothing hit yet, and the coordinates of its
// kRowsPerLane pixels (exact integers) as tri_rows and sph_rows take them.
// Expects in scope: x, y0 (the lane's pixel 0), and the arrays closest, hit,
// px, py, pxf, pyf, declared by the kernel.
#undef RT_INIT_ROWS
#define RT_INIT_ROWS()                                             \
    _Pragma("unroll") for (int j = 0; j < kRowsPerLane; ++j) {     \
        closest[j] = kFar;                                         \
        hit[j] = -1;                                               \
        py[j] = (double)(y0 + pix_dy(j));                          \
        pyf[j] = (float)(y0 + pix_dy(j));                          \
        px[j] = (double)(x + pix_dx(j));                           \
        pxf[j] = (float)(x + pix_dx(j));                           \
    }

// The record declarations of the candidate step.  From memory: scalar loads,
// three of the triangle's fields pinned in SGPRs.  From frame_small_kernel's
// LDS (s_tri, s_sph): broadcast LDS reads, used as VGPR operands (moving them
// to SGPRs, one v_readfirstlane per dword, measured slower).
#undef RT_TRI_MEM
#define RT_TRI_MEM                   \
    const TriRec r = tri_at(tri, p); \
    asm volatile("" ::"s"(r.p0), "s"(r.p1), "s"(r.dz))
#undef RT_SPH_MEM
#define RT_SPH_MEM const SphRec r = sph_at(sph, p - n_tri)
#undef RT_TRI_LDS
#define RT_TRI_LDS const TriRec& r = s_tri[p]
#undef RT_SPH_LDS
#define RT_SPH_LDS const SphRec& r = s_sph[p - n_tri]

// One kept candidate p (tile bits `bits`) against the lane's rows.  Both
// branches produce t per row (NaN: may not take); closest and hit are updated
// once, after them (round 4: trace 1-3 % faster than a test-and-update in
// each branch, DESIGN.md §3.5).  A sphere whose lower bound no lane's closest
// exceeds is skipped: t0 >= tmin >= every closest, so no lane can take it
// (strict <); the bound is refreshed only when a candidate was tested since.
// It `continue`s on such a sphere, so it stands directly inside the walk's
// loop, not in a nested one.
// TRI, SPH: the declaration of the record `r` (one pair above).  N_CUBES: the
// cube count as the kernel has it (an argument or scene.n_cubes: which SGPR).
// Expects in scope: p, bits, n_tri, px, py, pxf, pyf, closest, hit,
// tile_max_key, dirty.
#undef RT_TEST_CANDIDATE
#define RT_TEST_CANDIDATE(TRI, SPH, N_CUBES)              \
    float tc[kRowsPerLane];                               \
    int slot;                                             \
    if (p < n_tri) {                                      \
        TRI;                                              \
        tri_rows(r, bits, px, py, tc);                    \
        slot = p / 12;                                    \
    } else {                                              \
        SPH;                                              \
        if (dirty) {                                      \
            tile_max_key = wave_max_key(closest);         \
            dirty = false;                                \
        }                                                 \
        if (r.tmin_key >= tile_max_key) continue;         \
        sph_rows(r, bits, pxf, pyf, tc);                  \
        slot = (N_CUBES) + (p - n_tri);                   \
    }                                                     \
    take_rows(tc, slot, closest, hit);                    \
    dirty = true

// One wave (= one workgroup) per kWaveTile x kWaveTileH tile, all candidate
// data on scalar loads: count, then ids and tile words 8 at a time, then the
// records of the candidates this tile keeps (in the reference's primitive
// order).  2-D grid: x = bin column x kTiles + tile, y = bin row, so a wave
// finds its bin with shifts (kTiles is a power of two), no division in front
// of its first load.  (Measured and removed, DESIGN.md §3.5: several tiles
// per workgroup (again in round 4) or
// per wave, the triangle record in one round of scalar loads
// (both round-4 knobs: profiles/r04/trace_variants.patch), an XCD-contiguous
// tile order, the first
// list batch loaded beside the count, a store hand-off through LDS, the
// keep-ballot walk of trace3_split_kernel here, with and without the list's
// first 64 entries loaded beside the count; last in 9cad428.)
static_assert((kTiles & (kTiles - 1)) == 0, "tiles per bin: a power of two");
// (Arguments in the order the wave needs them: with kernel-argument
// preloading the first 14 dwords arrive in SGPRs.)
// Every output format is an instance of this one template; kMode != 0 (the
// trace ablations of rt_debug_set_trace_mode) exists in RT_DIAG builds only.
template <int kMode, int kFmt, int kAux>
__global__ void __launch_bounds__(64) RT_TRACE_ATTR trace3_kernel(
    const int* __restrict__ counts, const int* __restrict__ lists,
    const TriRec* __restrict__ tri, const SphRec* __restrict__ sph, int n_cx, int half_cap,
    int width, int row_begin, int row_end, int n_cubes, const float4* __restrict__ colours,
    void* __restrict__ out, SceneDev scene, float4 dir, int n_tiles_x, int out_format) {
    // (unsigned: the divisions by powers of two are shifts and masks)
    const unsigned bid = blockIdx.x;
    const int cbx = (int)(bid / kTiles), cby = (int)blockIdx.y;
    const int cb = cby * n_cx + cbx;
    const unsigned t = bid % kTiles;  // the tile of the bin (wave-uniform)
#if RT_TIMELINE
    const int tile = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
#endif
    const int lane = threadIdx.x & 63;
    const int n_tri = 12 * n_cubes;
    (void)n_tiles_x;
    (void)out_format;
    TL_MARK(tl0);
#if RT_TIMELINE
    const unsigned long long tlc0 = __builtin_amdgcn_s_memtime();
    unsigned tl1 = 0, tl2 = 0;
#endif
    const int rel_x = cbx * kCoarseW + (int)(t % kTilesX) * kWaveTile;
    const int rel_y = cby * kCoarseH + (int)(t / kTilesX) * kWaveTileH;  // vs row_begin
    const int tile_x = rel_x, tile_y = row_begin + rel_y;
    const int x = tile_x + (lane % kLanesX);  // the lane's pixel 0
    const int y0 = tile_y + (lane / kLanesX);
    // wave-uniform: tiles past the frame's right or bottom edge render nothing
    const bool tile_in = rel_x < width && rel_y < row_end - row_begin;

    // the bin's count (-1: non-finite scene data, see coarse3_kernel) is the
    // wave's first data load
    const int count_raw = kMode == 1 ? 0 : counts[cb];
    if (tile_in && kMode == 0 && count_raw < 0) {
        // Non-finite scene data: run the reference algorithm verbatim.
        RT_REFERENCE_PIXELS()
    } else if (tile_in) {
        int4v pix[kRowsPerLane];  // assigned after the walk (not live during it)
        float closest[kRowsPerLane];
        int hit[kRowsPerLane];
        double px[kRowsPerLane], py[kRowsPerLane];
        float pxf[kRowsPerLane], pyf[kRowsPerLane];
        RT_INIT_ROWS()
        // order_key of the largest `closest` in the tile, refreshed lazily
        unsigned tile_max_key = order_key(kFar);
        bool dirty = false;
        const int count = count_raw < 0 ? 0 : count_raw;
        const int* __restrict__ ids = lists + (int64_t)cb * kListStride * half_cap;
        const int* __restrict__ tms = ids + (1 + (int)(t / kTilesPerWord)) * half_cap;  // its word
        const int tm_shift = kTileBits * (int)(t % kTilesPerWord);
#if RT_TIMELINE
        tl1 = rt_now();
#endif
        for (int i0 = 0; i0 < count; i0 += 8) {
            int idv[8], tmv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                idv[k] = ids[i0 + k];  // half_cap is a multiple of 8 past the count
                tmv[k] = tms[i0 + k];
            }
            const int n = min(8, count - i0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k >= n) break;
                const unsigned bits = ((unsigned)tmv[k] >> tm_shift) & kTileMask;
                if (!(bits & kKeepMask)) continue;
                const int p = idv[k];
                if (kMode == 2) {
                    hit[0] = hit[0] > p ? hit[0] : -1;
                    continue;
                }
                RT_TEST_CANDIDATE(RT_TRI_MEM, RT_SPH_MEM, n_cubes);
            }
        }
#if RT_TIMELINE
        tl2 = rt_now();
#endif
        shade_pixels<kMode, kFmt>(colours, closest, hit, pix);
        const bool full = rel_x + kWaveTile <= width && tile_y + kWaveTileH <= row_end;
        store_rows<kMode, kFmt, kAux>(pix, rel_x, rel_y, lane, width, row_end - row_begin, full,
                                      out);
    }  // finite scene, tile inside the frame
#if RT_TIMELINE
    {
        const unsigned tl3 = rt_now();
        const unsigned long long tlc3 = __builtin_amdgcn_s_memtime();
        if (lane == 0) {
            unsigned* o = g_timeline + 8 * (int64_t)tile;
            o[0] = tl0; o[1] = tl1; o[2] = tl2; o[3] = tl3;
            o[4] = (unsigned)tlc0; o[5] = (unsigned)tlc3;
            o[6] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
            o[7] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        }
    }
#endif
}


// Small frames: the same walk as trace3_kernel with one WORKGROUP of
// n_waves (2 or 4) waves per wave tile.  Every wave reads the tile's whole
// list (scalar loads, shared in the CU's scalar cache) and tests every
// n_waves-th candidate the tile keeps (by kept ordinal), so a tile's chain of
// record -> test -> compare is n_waves times shorter: in frames with few
// tiles (a few thousand waves, one generation) the kernel lasts as long as
// its heaviest tile's walk.  Merge (wave 0, through LDS): per pixel the
// smallest t, ties to the smallest slot.  That is the sequential walk's
// result: it takes the first candidate in primitive order reaching the
// minimum (strict <, MainState.cpp:386-391), every wave's walk takes the
// first of its own, and slots (p / 12 for triangles, then n_cubes + sphere)
// never decrease along primitive order (equal slots: the same colour).
// NaN never enters (a taken t passed t < closest).  A wave's sphere depth
// cull uses its own closest values, which bound the tile's from above, so
// it skips no sphere the sequential walk would have taken.
constexpr int kSplitMax = 4;  // waves per tile (workgroup of 256 lanes; 8 measured slower)
template <int kFmt, int kAux>
__global__ void __launch_bounds__(64 * kSplitMax) RT_TRACE_ATTR trace3_split_kernel(
    SceneDev scene, const TriRec* __restrict__ tri, const SphRec* __restrict__ sph,
    const float4* __restrict__ colours, const int* __restrict__ counts,
    const int* __restrict__ lists, int half_cap, float4 dir, int width, int row_begin,
    int row_end, int n_cx, void* __restrict__ out) {
    const unsigned bid = blockIdx.x;
    const int cbx = (int)(bid / kTiles), cby = (int)blockIdx.y;
    const int cb = cby * n_cx + cbx;
    const unsigned t = bid % kTiles;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_waves = (int)(blockDim.x >> 6);
    const int lane = threadIdx.x & 63;
    const int n_tri = 12 * scene.n_cubes;
    const int rel_x = cbx * kCoarseW + (int)(t % kTilesX) * kWaveTile;
    const int rel_y = cby * kCoarseH + (int)(t / kTilesX) * kWaveTileH;
    const int tile_x = rel_x, tile_y = row_begin + rel_y;
    const int x = tile_x + (lane % kLanesX);
    const int y0 = tile_y + (lane / kLanesX);
    // workgroup-uniform: the whole workgroup leaves together (no barrier pending)
    if (!(rel_x < width && rel_y < row_end - row_begin)) return;
    const int count_raw = counts[cb];
    if (count_raw < 0) {  // non-finite scene data: the reference verbatim (wave 0)
        if (wave != 0) return;
        RT_REFERENCE_PIXELS()
        return;
    }
    float closest[kRowsPerLane];
    int hit[kRowsPerLane];
    double px[kRowsPerLane], py[kRowsPerLane];
    float pxf[kRowsPerLane], pyf[kRowsPerLane];
    RT_INIT_ROWS()
    unsigned tile_max_key = order_key(kFar);
    bool dirty = false;
    const int* __restrict__ ids = lists + (int64_t)cb * kListStride * half_cap;
    const int* __restrict__ tms = ids + (1 + (int)(t / kTilesPerWord)) * half_cap;
    const int tm_shift = kTileBits * (int)(t % kTilesPerWord);
    int turn = 0;  // whose kept candidate is next: 0 .. n_waves - 1 (every wave counts all)
    // The bin's list 64 entries at a time as vector loads (entry e on lane
    // e), this tile's keep bits in one ballot, and only the kept entries
    // visited (s_ff1 over the mask, id and bits by v_readlane), in primitive
    // order; every wave visits every kept entry to count turns.
    for (int c0 = 0; c0 < count_raw; c0 += 64) {
        const int e = c0 + lane;
        int idl = 0;
        unsigned bl = 0u;
        if (e < count_raw) {
            idl = ids[e];
            bl = ((unsigned)tms[e] >> tm_shift) & kTileMask;
        }
        unsigned long long keep = __ballot((bl & kKeepMask) != 0u);
        while (keep) {
            const int k = __builtin_ctzll(keep);
            keep &= keep - 1ull;
            const bool mine = turn == wave;
            turn = turn + 1 == n_waves ? 0 : turn + 1;
            if (!mine) continue;
            const int p = __builtin_amdgcn_readlane(idl, k);
            const unsigned bits = (unsigned)__builtin_amdgcn_readlane((int)bl, k);
            RT_TEST_CANDIDATE(RT_TRI_MEM, RT_SPH_MEM, scene.n_cubes);
        }
    }
    // merge into wave 0: the other waves' closest / hit through LDS
    __shared__ float s_close[kSplitMax - 1][kRowsPerLane][64];
    __shared__ int s_hit[kSplitMax - 1][kRowsPerLane][64];
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) {
            s_close[wave - 1][j][lane] = closest[j];
            s_hit[wave - 1][j][lane] = hit[j];
        }
    }
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < n_waves; ++w) {
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) {
            const float c = s_close[w - 1][j][lane];
            const int h = s_hit[w - 1][j][lane];
            const bool take = h >= 0 && (c < closest[j] || (c == closest[j] && h < hit[j]));
            closest[j] = take ? c : closest[j];
            hit[j] = take ? h : hit[j];
        }
    }
    int4v pix[kRowsPerLane];
    shade_pixels<0, kFmt>(colours, closest, hit, pix);
    const bool full = rel_x + kWaveTile <= width && tile_y + kWaveTileH <= row_end;
    store_rows<0, kFmt, kAux>(pix, rel_x, rel_y, lane, width, row_end - row_begin, full, out);
}


// Small scenes (at most 64 x RT_SMALL_CHUNKS primitives, that many prep
// chunks): no coarse kernel and no candidate lists.  Each tile wave ANDs its
// bin row's and bin column's mask words per chunk (the candidates, in
// primitive order), lets lane i classify candidate 64 c + i against the tile
// exactly as coarse3_kernel does, and walks the kept candidates from the
// ballots, chunk by chunk.  Saves the coarse launch and
// one kernel boundary, which dominate small frames (config 2).
#ifndef RT_FUSED_WG
#define RT_FUSED_WG 4  // frame_small_kernel: wave tiles per workgroup (each preps the scene once)
#endif
#ifndef RT_FUSED_WAVES
#define RT_FUSED_WAVES 8  // frame_small_kernel's waves per SIMD (VGPR budget)
#endif
#if RT_FUSED_WAVES > 0
// (the two-chunk instance needs 86 VGPRs, so it gets the 5 waves that allow)
#define RT_FUSED_ATTR                                                              \
    __attribute__((amdgpu_waves_per_eu(kChunks == 1 ? RT_FUSED_WAVES : 5,         \
                                       kChunks == 1 ? RT_FUSED_WAVES : 5)))
#else
#define RT_FUSED_ATTR
#endif
#ifndef RT_FUSED_CHUNKS
#define RT_FUSED_CHUNKS 2  // frame_small_kernel takes scenes of up to 64 x this many primitives
#endif
#ifndef RT_SMALL_CHUNKS
#define RT_SMALL_CHUNKS 8  // the small-scene path takes scenes of up to 64 x this many primitives
#endif
template <int kFmt, int kChunks>
__global__ void __launch_bounds__(64) RT_TRACE_ATTR trace_small_kernel(
    const unsigned long long* __restrict__ row_masks,
    const unsigned long long* __restrict__ col_masks, const int4* __restrict__ boxes,
    const Cls* __restrict__ cls, const TriRec* __restrict__ tri, const SphRec* __restrict__ sph,
    const float4* __restrict__ colours, const unsigned* __restrict__ nonfinite_flag,
    unsigned gen, int n_cubes, int n_cx, int n_chunks, int width, int row_begin, int row_end,
    SceneDev scene, float4 dir, void* __restrict__ out) {
    const int bid = (int)blockIdx.x;
    const int cb = bid / kTiles;
    const int t = __builtin_amdgcn_readfirstlane(bid % kTiles);
    const int lane = threadIdx.x & 63;
    const int n_tri = 12 * n_cubes;
    const int rel_x = (cb % n_cx) * kCoarseW + (t % kTilesX) * kWaveTile;
    const int rel_y = (cb / n_cx) * kCoarseH + (t / kTilesX) * kWaveTileH;
    if (!(rel_x < width && rel_y < row_end - row_begin)) return;  // outside: no stores
    const int tile_x = rel_x, tile_y = row_begin + rel_y;
    const int x = tile_x + (lane % kLanesX);  // the lane's pixel 0
    const int y0 = tile_y + (lane / kLanesX);
    unsigned long long cand[kChunks];
#pragma unroll
    for (int c = 0; c < kChunks; ++c)
        cand[c] = c < n_chunks ? row_masks[(int64_t)(cb / n_cx) * n_chunks + c] &
                                     col_masks[(int64_t)(cb % n_cx) * n_chunks + c]
                               : 0ull;
    const bool nonfinite = *nonfinite_flag == gen;
    int4v pix[kRowsPerLane];
    if (nonfinite) {  // the reference algorithm verbatim
        RT_REFERENCE_PIXELS()
        return;
    }
    // lane i: candidate 64 c + i against this tile (coarse3_kernel's test).
    // With one chunk (<= 64 primitives) every lane's box and classifier are
    // loaded up front, beside the mask words, instead of after them: one
    // dependent round trip less per wave.
    int4 pb0 = make_int4(1 << 30, 1 << 30, -(1 << 30), -(1 << 30));
    Cls k0{};
    if (kChunks == 1 && lane < n_tri + scene.n_spheres) {
        pb0 = boxes[lane];
        k0 = cls[lane];
    }
    unsigned long long keep[kChunks], inside[kChunks];
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const int q = 64 * c + lane;
        bool keep_l = false, inside_l = false;
        if ((cand[c] >> lane) & 1ull) {
            const int4 pb = kChunks == 1 ? pb0 : boxes[q];
            const int tx = tile_x, ty = tile_y;
            if (pb.x <= tx + kWaveTile - 1 && pb.z >= tx && pb.y <= ty + kWaveTileH - 1 &&
                pb.w >= ty)
                classify(kChunks == 1 ? k0 : cls[q], q < n_tri, (float)tx, (float)ty, &keep_l,
                         &inside_l);
        }
        keep[c] = __ballot(keep_l);
        inside[c] = __ballot(keep_l && inside_l);
    }
    float closest[kRowsPerLane];
    int hit[kRowsPerLane];
    double px[kRowsPerLane], py[kRowsPerLane];
    float pxf[kRowsPerLane], pyf[kRowsPerLane];
    RT_INIT_ROWS()
    unsigned tile_max_key = order_key(kFar);
    bool dirty = false;
#pragma unroll
    for (int c = 0; c < kChunks; ++c)
    while (keep[c]) {  // kept candidates in primitive order
        const int b = __builtin_ctzll(keep[c]);
        keep[c] &= keep[c] - 1ull;
        const int p = 64 * c + b;
        const unsigned bits = ((inside[c] >> b) & 1ull) ? kTileMask : kKeepMask;
        RT_TEST_CANDIDATE(RT_TRI_MEM, RT_SPH_MEM, n_cubes);
    }
    shade_pixels<0, kFmt>(colours, closest, hit, pix);
    const bool full = rel_x + kWaveTile <= width && tile_y + kWaveTileH <= row_end;
    store_rows<0, kFmt>(pix, rel_x, rel_y, lane, width, row_end - row_begin, full, out);
}


// Binned frames without the coarse kernel (round 4 experiment, merged in
// round 5 as the automatic path for frames of low box overdraw: launch()):
// each wave tile ANDs its bin's row and column mask words (one chunk per
// lane), packs the candidates' ids in primitive order into LDS rounds of 64,
// classifies a round's candidates against its own tile (one vector load of
// boxes and classifiers per round, as coarse3_kernel's per-tile test),
// compacts the kept ones in place and walks them in order.  No coarse depth
// cull (a per-tile one measured slower, DESIGN.md §3.5); the walk's own
// sphere cull stays.  Non-finite scene data: the reference verbatim.
constexpr int kBinCap = 1024;  // trace_bin_kernel: scenes of at most this many primitives

template <int kFmt, int kAux>
__global__ void __launch_bounds__(64) RT_TRACE_ATTR trace_bin_kernel(
    // (the first 14 argument dwords arrive preloaded in SGPRs: the ones a
    // wave needs before its first data loads; the rest load in their shadow)
    int n_chunks, int width, int row_begin, int row_end, unsigned gen, int n_cx,
    const unsigned* __restrict__ nonfinite_flag, const unsigned long long* __restrict__ row_masks,
    const unsigned long long* __restrict__ col_masks, const int4* __restrict__ boxes,
    const Cls* __restrict__ cls, const TriRec* __restrict__ tri, const SphRec* __restrict__ sph,
    const float4* __restrict__ colours, SceneDev scene, float4 dir, void* __restrict__ out,
    const unsigned long long* __restrict__ overdraw, unsigned long long* __restrict__ overdraw_next,
    unsigned long long od_lo, unsigned long long od_hi, unsigned* __restrict__ od_verdict) {
    const unsigned bid = blockIdx.x;
    const int cbx = (int)(bid / kTiles), cby = (int)blockIdx.y;
    const unsigned t = bid % kTiles;
    const int lane = threadIdx.x & 63;
    const int n_tri = 12 * scene.n_cubes;
    (void)n_cx;
    if (bid == 0 && blockIdx.y == 0 && lane == 0) {
        // coarse3_kernel's duties for the frame's overdraw: zero the other
        // slot for the next binned launch, report the verdict to the host
        const unsigned long long od =
            __hip_atomic_load(overdraw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *overdraw_next = 0ull;
        store_verdict(od_verdict, od < od_lo ? 1u : od < od_hi ? 2u : 3u);
    }
    const int rel_x = cbx * kCoarseW + (int)(t % kTilesX) * kWaveTile;
    const int rel_y = cby * kCoarseH + (int)(t / kTilesX) * kWaveTileH;
    if (!(rel_x < width && rel_y < row_end - row_begin)) return;  // outside: no stores
    const int tile_x = rel_x, tile_y = row_begin + rel_y;
    const int x = tile_x + (lane % kLanesX);
    const int y0 = tile_y + (lane / kLanesX);
    const unsigned long long* rw = row_masks + (int64_t)cby * n_chunks;
    const unsigned long long* cw = col_masks + (int64_t)cbx * n_chunks;
    const bool nonfinite = *nonfinite_flag == gen;
    if (nonfinite) {  // the reference algorithm verbatim
        RT_REFERENCE_PIXELS()
        return;
    }
    // (1) the bin's candidate ids in primitive order into LDS (launch() takes
    // this kernel only for scenes of at most kBinCap primitives: they fit)
    __shared__ int s_ids[kBinCap];
    int n_cand = 0;
    {
        const unsigned long long w = lane < n_chunks ? rw[lane] & cw[lane] : 0ull;
        unsigned long long nz = __ballot(w != 0ull);
        while (nz) {  // the nonzero chunks in order; their ids in bit order
            const int c = __builtin_ctzll(nz);
            nz &= nz - 1ull;
            const unsigned long long wc =
                (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)w, c) |
                ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(w >> 32), c)
                 << 32);
            if ((wc >> lane) & 1ull)
                s_ids[n_cand + (int)__builtin_amdgcn_mbcnt_hi(
                                   (unsigned)(wc >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)wc, 0u))] =
                    c * 64 + lane;
            n_cand += __popcll(wc);
        }
    }
    __builtin_amdgcn_wave_barrier();
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    // (2) classify them against this tile, 64 at a time, compacting the kept
    // ones in place (bit 31: u,v proven inside); a round's ids are read
    // before any of its writes, which land at or below its first slot
    int n_kept = 0;
    for (int base = 0; base < n_cand; base += 64) {
        const int e = base + lane;
        const int id = e < n_cand ? s_ids[e] : 0;
        bool keep_l = false, inside_l = false;
        if (e < n_cand) {
            // the classifier loaded beside the box (one round trip, not two:
            // round 5, trace 46.9 -> 46.2 us int32x4, 43.4 -> 43.0 RGBA8)
            const Cls k = cls[id];
            const int4 pb = boxes[id];
            if (pb.x <= tile_x + kWaveTile - 1 && pb.z >= tile_x &&
                pb.y <= tile_y + kWaveTileH - 1 && pb.w >= tile_y)
                classify(k, id < n_tri, (float)tile_x, (float)tile_y, &keep_l, &inside_l);
        }
        const unsigned long long keep = __ballot(keep_l);
        __builtin_amdgcn_wave_barrier();
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        if (keep_l)
            s_ids[n_kept + (int)__builtin_amdgcn_mbcnt_hi(
                               (unsigned)(keep >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)keep, 0u))] =
                id | (inside_l ? (int)0x80000000 : 0);
        n_kept += __popcll(keep);
        __builtin_amdgcn_wave_barrier();
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
    }
    // (3) walk the kept candidates in order, 8 entries per LDS read round
    float closest[kRowsPerLane];
    int hit[kRowsPerLane];
    double px[kRowsPerLane], py[kRowsPerLane];
    float pxf[kRowsPerLane], pyf[kRowsPerLane];
    RT_INIT_ROWS()
    unsigned tile_max_key = order_key(kFar);
    bool dirty = false;
    for (int i0 = 0; i0 < n_kept; i0 += 8) {
        const int ent = lane < 8 && i0 + lane < n_kept ? s_ids[i0 + lane] : 0;
        const int n = min(8, n_kept - i0);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k >= n) break;
            const int e = __builtin_amdgcn_readlane(ent, k);
            const int p = e & 0x7fffffff;
            const unsigned bits = e < 0 ? kTileMask : kKeepMask;
            RT_TEST_CANDIDATE(RT_TRI_MEM, RT_SPH_MEM, scene.n_cubes);
        }
    }
    int4v pix[kRowsPerLane];
    shade_pixels<0, kFmt>(colours, closest, hit, pix);
    const bool full = rel_x + kWaveTile <= width && tile_y + kWaveTileH <= row_end;
    store_rows<0, kFmt, kAux>(pix, rel_x, rel_y, lane, width, row_end - row_begin, full, out);
}


// Small scenes in ONE kernel (at most 64 x kChunks primitives): workgroups
// of RT_FUSED_WG wave tiles of one coarse bin.  Its first kChunks waves prep
// the triangles and the next kChunks the spheres into LDS (records, boxes,
// classifiers, colours; one primitive per lane, the same prep_triangle /
// prep_sphere as prep_kernel), then, after one barrier, every wave
// classifies its own wave tile against every primitive (box overlap +
// classify, as coarse3_kernel does), walks the kept ones in primitive order
// with their records read from LDS, shades and stores.  No prep kernel, no
// bin masks, no records in global memory: the frame is one launch with one
// memory round trip (the scene) in front of the stores.  Non-finite scene
// data: the reference algorithm verbatim (RT_REFERENCE_PIXELS).
constexpr int kFusedWaves = RT_FUSED_WG;  // wave tiles (waves) per workgroup
static_assert(kTiles % kFusedWaves == 0, "a workgroup's tiles lie in one bin");
template <int kFmt, int kChunks>
__global__ void __launch_bounds__(64 * kFusedWaves) RT_FUSED_ATTR frame_small_kernel(
    SceneDev scene, float4 dir, int n_cx, int width, int row_begin, int row_end,
    void* __restrict__ out) {
    constexpr int kCap = 64 * kChunks;
    __shared__ TriRec s_tri[kCap];
    __shared__ SphRec s_sph[kCap];
    __shared__ int4 s_box[kCap];
    __shared__ Cls s_cls[kCap];
    __shared__ float4 s_col[kCap];
    // Prep: triangles and spheres on different waves (no divergent wave
    // runs both preps one after the other): waves [0, kChunks) take
    // triangles 64 w + lane, waves [kChunks, 2 kChunks) spheres.
    constexpr int kPrepWaves = 2 * kChunks;
    __shared__ unsigned s_bad[kPrepWaves];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    constexpr int kGroups = kTiles / kFusedWaves;  // workgroups per bin
    const int cb = blockIdx.x / kGroups;
    const int n_tri = 12 * scene.n_cubes;
    const int n_prims = n_tri + scene.n_spheres;
    static_assert(kPrepWaves <= kFusedWaves, "one prep chunk per wave");
    if (wave < kPrepWaves) {
        const bool tri_wave = wave < kChunks;  // (wave-uniform)
        const int i = tri_wave ? 64 * wave + lane : n_tri + 64 * (wave - kChunks) + lane;
        Box b = empty_box();
        Cls k{};
        bool bad = false;
        if (tri_wave && i < n_tri) {
            const float4* v = scene.cube_vertices + 3 * i;
            const float4 a = v[0], bb = v[1], c = v[2];
            const float fa[3] = {a.x, a.y, a.z}, fb[3] = {bb.x, bb.y, bb.z},
                        fc[3] = {c.x, c.y, c.z};
            if (i % 12 == 0) s_col[i / 12] = scene.cube_colours[i / 12];
            // (the record goes straight into LDS as prep computes it, not
            // held in registers through the box and classifier arithmetic:
            // no spills at 64 VGPRs, DESIGN.md §3.5; a triangle that can
            // never hit is never a candidate, its record is zeroed only for
            // determinism)
            if (!prep_triangle(fa, fb, fc, (double)dir.x, (double)dir.y, (double)dir.z, width,
                               row_begin, row_end, &s_tri[i], &b, &k, &bad))
                s_tri[i] = TriRec{};
        } else if (!tri_wave && i < n_prims) {
            const int sp = i - n_tri;
            const float4 o = scene.sphere_origins[sp];
            s_col[scene.n_cubes + sp] = scene.sphere_colours[sp];
            const float fo[4] = {o.x, o.y, o.z, o.w};
            prep_sphere(fo, scene.sphere_radius[sp], dir.x, dir.y, dir.z, dir.w, width, row_begin,
                        row_end, &s_sph[sp], &b, &k, &bad);  // (writes every field)
        }
        if (tri_wave ? i < n_tri : i < n_prims) {
            s_box[i] = make_int4(b.x0, b.y0, b.x1, b.y1);
            s_cls[i] = k;
        }
        const unsigned any_bad = __ballot(bad) != 0ull ? 1u : 0u;
        if (lane == 0) s_bad[wave] = any_bad;
    }
    __syncthreads();
    const int t = (blockIdx.x % kGroups) * kFusedWaves + wave;  // this wave's tile of the bin
    const int rel_x = (cb % n_cx) * kCoarseW + (t % kTilesX) * kWaveTile;
    const int rel_y = (cb / n_cx) * kCoarseH + (t / kTilesX) * kWaveTileH;
    if (!(rel_x < width && rel_y < row_end - row_begin)) return;  // outside: no stores
    const int tile_x = rel_x, tile_y = row_begin + rel_y;
    const int x = tile_x + (lane % kLanesX);  // the lane's pixel 0
    const int y0 = tile_y + (lane / kLanesX);
    bool nonfinite = false;
#pragma unroll
    for (int c = 0; c < kPrepWaves; ++c) nonfinite |= s_bad[c] != 0u;
    if (nonfinite) {
        RT_REFERENCE_PIXELS()
        return;
    }
    unsigned long long keep[kChunks], inside[kChunks];
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const int q = 64 * c + lane;
        bool keep_l = false, inside_l = false;
        if (q < n_prims) {
            const int4 pb = s_box[q];
            if (pb.x <= tile_x + kWaveTile - 1 && pb.z >= tile_x &&
                pb.y <= tile_y + kWaveTileH - 1 && pb.w >= tile_y)
                classify(s_cls[q], q < n_tri, (float)tile_x, (float)tile_y, &keep_l, &inside_l);
        }
        keep[c] = __ballot(keep_l);
        inside[c] = __ballot(keep_l && inside_l);
    }
    float closest[kRowsPerLane];
    int hit[kRowsPerLane];
    double px[kRowsPerLane], py[kRowsPerLane];
    float pxf[kRowsPerLane], pyf[kRowsPerLane];
    RT_INIT_ROWS()
    unsigned tile_max_key = order_key(kFar);
    bool dirty = false;
#pragma unroll
    for (int c = 0; c < kChunks; ++c)
    while (keep[c]) {  // kept candidates in primitive order
        const int b = __builtin_ctzll(keep[c]);
        keep[c] &= keep[c] - 1ull;
        const int p = 64 * c + b;
        const unsigned bits = ((inside[c] >> b) & 1ull) ? kTileMask : kKeepMask;
        RT_TEST_CANDIDATE(RT_TRI_LDS, RT_SPH_LDS, scene.n_cubes);  // records from LDS
    }
    int4v pix[kRowsPerLane];
    shade_pixels<0, kFmt>(s_col, closest, hit, pix);
    const bool full = rel_x + kWaveTile <= width && tile_y + kWaveTileH <= row_end;
    store_rows<0, kFmt>(pix, rel_x, rel_y, lane, width, row_end - row_begin, full, out);
}

// the tile kernels' shared text ends here: none of it reaches the host half
#undef RT_REFERENCE_PIXELS
#undef RT_INIT_ROWS
#undef RT_TRI_MEM
#undef RT_SPH_MEM
#undef RT_TRI_LDS
#undef RT_SPH_LDS
#undef RT_TEST_CANDIDATE

}  // namespace

namespace {

// What this tile build contributes to the dispatch policy (rt_dispatch.h).
constexpr rt_dispatch::Geometry kGeometry{
    kCoarseW, kCoarseH, kTiles, kListStride, kPrepThreads,
    RT_FUSED_WG, RT_FUSED_CHUNKS, RT_SMALL_CHUNKS, kBinCap, kMaskBinsMax,
    128, 32, 32, 48};  // TriRec, SphRec, Cls, TriDepth
static_assert(kGeometry.tri_rec_bytes == sizeof(TriRec) &&
                  kGeometry.sph_rec_bytes == sizeof(SphRec) &&
                  kGeometry.cls_bytes == sizeof(Cls) &&
                  kGeometry.tri_depth_bytes == sizeof(TriDepth) && sizeof(int4) == 16 &&
                  sizeof(float4) == 16,
              "the workspace plan's record sizes");

// Grow the binned path's workspace to what a launch over `rows` rows needs
// (rt_reserve, and rt_render before its timed region): the launch then
// allocates nothing.  The plan is the one choose() hands launch() for that
// band: the same function of the same arguments.
int reserve(rt_ctx* ctx, int n_spheres, int n_cubes, int32_t width, int32_t rows) {
    const int64_t per = rt_dispatch::band_rows_of(
        kGeometry, ctx->knobs, 12 * (int64_t)n_cubes + n_spheres, width, rows);
    const rt_dispatch::Plan p = rt_dispatch::plan(kGeometry, ctx->knobs, n_spheres, n_cubes, width,
                                                  (int32_t)std::min<int64_t>(per, rows));
    int rc = ensure(&ctx->rec_buf, &ctx->rec_cap, p.rec_need);
    if (rc) return rc;
    return ensure(&ctx->list_buf, &ctx->list_cap, p.list_need);
}

// Load every kernel of this build onto the current device now (rt_init),
// instead of inside the first render: HIP loads a code object on its first
// use, which otherwise lands between the first render's events.
template <typename K>
int preload_one(K kernel) {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(kernel)) == hipSuccess
               ? RT_OK
               : RT_ERR_HIP;
}

// every output format's instance of KERNEL<format, ...>
#undef RT_PRELOAD_FMTS
#define RT_PRELOAD_FMTS(KERNEL, ...)                              \
    one(preload_one(KERNEL<RT_FORMAT_I32X4, ##__VA_ARGS__>));     \
    one(preload_one(KERNEL<RT_FORMAT_RGBA8, ##__VA_ARGS__>));     \
    one(preload_one(KERNEL<RT_FORMAT_HIT, ##__VA_ARGS__>))
// The kernels that write whole frames on the binned path, by format and the
// store policy's cache bits (trace3_kernel's as <format, bits, mode>).
template <int kFmt, int kAux, int kMode = 0>
constexpr auto trace3_of = trace3_kernel<kMode, kFmt, kAux>;
// every format's instances of KERNEL<format, bits of each store policy>
#undef RT_PRELOAD_STORES
#define RT_PRELOAD_STORES(KERNEL)                                                \
    RT_PRELOAD_FMTS_AUX(KERNEL, RT_STORE_DEFAULT);                               \
    RT_PRELOAD_FMTS_AUX(KERNEL, RT_STORE_LARGE)
#undef RT_PRELOAD_FMTS_AUX
#define RT_PRELOAD_FMTS_AUX(KERNEL, POLICY)                                              \
    one(preload_one(KERNEL<RT_FORMAT_I32X4, store_aux(RT_FORMAT_I32X4, POLICY)>));       \
    one(preload_one(KERNEL<RT_FORMAT_RGBA8, store_aux(RT_FORMAT_RGBA8, POLICY)>));       \
    one(preload_one(KERNEL<RT_FORMAT_HIT, store_aux(RT_FORMAT_HIT, POLICY)>))
int preload() {
    int rc = RT_OK;
    auto one = [&rc](int r) { if (r != RT_OK) rc = r; };
    one(preload_one(generic_kernel));
    one(preload_one(prep_kernel));
    one(preload_one(coarse3_kernel<1>));
    one(preload_one(coarse3_kernel<2>));
    one(preload_one(coarse3_kernel<4>));
    one(preload_one(coarse3_kernel<8>));
    RT_PRELOAD_STORES(trace3_of);
    RT_PRELOAD_STORES(trace3_split_kernel);
    RT_PRELOAD_STORES(trace_bin_kernel);
    RT_PRELOAD_FMTS(trace_small_kernel, 1);
    RT_PRELOAD_FMTS(trace_small_kernel, 2);
    RT_PRELOAD_FMTS(trace_small_kernel, 4);
    RT_PRELOAD_FMTS(trace_small_kernel, RT_SMALL_CHUNKS);
    RT_PRELOAD_FMTS(frame_small_kernel, 1);
    RT_PRELOAD_FMTS(frame_small_kernel, 2);
    RT_PRELOAD_FMTS(frame_small_kernel, RT_FUSED_CHUNKS);
    return rc;
}

// Where the kernels cannot write the host's verdict word themselves
// (no od_verdict_dev): the overdraw verdict of a binned launch (flag word 6)
// to the host's page-locked word, on the first binned launch of a context
// and every 8th after: an asynchronous 4-byte copy behind the frame's
// kernels, read by a later launch's automatic path choice (whatever copy
// has landed by then).  (rt_render defers it behind its frame download:
// defer_verdict.)
#ifndef RT_VERDICT_EVERY
#define RT_VERDICT_EVERY 8  // binned launches per verdict copy (a power of two)
#endif
static_assert((RT_VERDICT_EVERY & (RT_VERDICT_EVERY - 1)) == 0, "verdict period");
unsigned* verdict_word(rt_ctx* ctx) { return ctx->od_verdict_dev ? ctx->od_verdict_dev : ctx->flag + 6; }
int copy_verdict(rt_ctx* ctx, hipStream_t stream) {
    constexpr unsigned kPeriod = RT_VERDICT_EVERY;
    if (ctx->od_verdict_dev) return RT_OK;  // the kernels wrote it themselves
    if (!ctx->od_verdict || (ctx->od_launches & (kPeriod - 1u)) != (1u & (kPeriod - 1u)))
        return RT_OK;
    if (ctx->defer_verdict) {
        ctx->verdict_due = true;
        return RT_OK;
    }
    return enqueue_verdict_copy(ctx, stream);
}

// KERNEL<format, ...> of launch()'s `fmt` (checked by the callers: one of
// the three formats), and trace3_kernel<MODE, format>.
#undef RT_BY_FMT
#define RT_BY_FMT(KERNEL, ...)                                        \
    (fmt == RT_FORMAT_I32X4 ? KERNEL<RT_FORMAT_I32X4, ##__VA_ARGS__>  \
     : fmt == RT_FORMAT_HIT ? KERNEL<RT_FORMAT_HIT, ##__VA_ARGS__>    \
                            : KERNEL<RT_FORMAT_RGBA8, ##__VA_ARGS__>)
// KERNEL<format, the cache bits of the band's store policy, ...> (the frame
// writers of the binned path; dc.store_policy is rt_dispatch::choose()'s)
#undef RT_BY_STORE
#define RT_BY_STORE(KERNEL, FMT, ...)                                            \
    (b.dc.store_policy == RT_STORE_LARGE                                         \
         ? KERNEL<FMT, store_aux(FMT, RT_STORE_LARGE), ##__VA_ARGS__>            \
         : KERNEL<FMT, store_aux(FMT, RT_STORE_DEFAULT), ##__VA_ARGS__>)
#undef RT_BY_FMT_STORE
#define RT_BY_FMT_STORE(KERNEL, ...)                                                \
    (fmt == RT_FORMAT_I32X4 ? RT_BY_STORE(KERNEL, RT_FORMAT_I32X4, ##__VA_ARGS__)   \
     : fmt == RT_FORMAT_HIT ? RT_BY_STORE(KERNEL, RT_FORMAT_HIT, ##__VA_ARGS__)     \
                            : RT_BY_STORE(KERNEL, RT_FORMAT_RGBA8, ##__VA_ARGS__))
#undef RT_TRACE3_BY_FMT
#define RT_TRACE3_BY_FMT(MODE) RT_BY_FMT_STORE(trace3_of, MODE)
#ifndef RT_SKIP_DIAG
#define RT_SKIP_DIAG 0  // diagnostics (RT_DIAG builds): after a context's first 16 binned launches skip prep (1) / coarse (2)
#endif

// The typed pointers of one binned launch's workspace, from its plan.
struct Workspace {
    TriRec* tri;
    TriDepth* tdep;
    SphRec* sph;
    int4* boxes;
    Cls* cls;
    float4* colours;
    int* counts;
    unsigned long long *row_masks, *col_masks;  // null without bin masks
    int* lists;
};
Workspace carve(const rt_ctx* ctx, const rt_dispatch::Plan& pl) {
    char* base = static_cast<char*>(ctx->rec_buf);
    Workspace w;
    w.tri = reinterpret_cast<TriRec*>(base + pl.tri_off);
    w.tdep = reinterpret_cast<TriDepth*>(base + pl.dep_off);
    w.sph = reinterpret_cast<SphRec*>(base + pl.sph_off);
    w.boxes = reinterpret_cast<int4*>(base + pl.box_off);
    w.cls = reinterpret_cast<Cls*>(base + pl.cls_off);
    w.colours = reinterpret_cast<float4*>(base + pl.col_off);
    w.counts = reinterpret_cast<int*>(base + pl.cnt_off);
    w.row_masks =
        pl.use_masks ? reinterpret_cast<unsigned long long*>(base + pl.mask_off) : nullptr;
    w.col_masks = pl.use_masks ? w.row_masks + (size_t)pl.n_chunks * pl.n_cy : nullptr;
    w.lists = static_cast<int*>(ctx->list_buf);
    return w;
}

// What the kernels of one binned band launch share: the launch's arguments,
// its decision and workspace, and its profiling events (a (start, stop) pair
// per kernel slot: prep, coarse, trace; null without profiling).
struct Band {
    rt_ctx* ctx;
    hipStream_t stream;
    SceneDev sd;
    float4 dir;
    int32_t width, row_begin, row_end, fmt;
    void* out;
    const hipEvent_t *pe_prep, *pe_coarse, *pe_trace;
    const rt_dispatch::Decision& dc;
    Workspace ws;
};

// prep_kernel over the band's primitives, the first kernel of its chain.
// `overdraw`: the slot it sums the frame's box overdraw into (null: the
// small path, which has no use for it).
int enqueue_prep(const Band& b, unsigned long long* overdraw) {
    const rt_dispatch::Plan& pl = b.dc.plan;
    const Workspace& ws = b.ws;
    return launch_k(prep_kernel, dim3((unsigned)pl.n_chunks), dim3(kPrepThreads), b.stream,
                    kernel_events(b.ctx, b.pe_prep, true, false), b.sd, b.dir, b.width,
                    b.row_begin, b.row_end, ws.tri, ws.tdep, ws.sph, ws.boxes, ws.cls, ws.colours,
                    b.ctx->flag, b.ctx->gen, ws.row_masks, ws.col_masks, pl.n_cx, pl.n_cy,
                    overdraw);
}

// The box-overdraw slots of a launch that feeds them (flag words 2-3 / 4-5,
// alternating per such launch): prep adds into `word`, coarse (or
// trace_bin_kernel) reads it and zeroes `next` for the next launch.
struct OdSlots {
    unsigned long long *word, *next;
};
OdSlots take_od_slots(rt_ctx* ctx, unsigned long long area_units) {
    ctx->od_area = area_units;  // (rt_debug_last_overdraw: the launch that sums it)
    const unsigned slot = ctx->od_launches++ & 1u;
    return OdSlots{reinterpret_cast<unsigned long long*>(ctx->flag + 2 + 2 * slot),
                   reinterpret_cast<unsigned long long*>(ctx->flag + 4 - 2 * slot)};
}

// RT_KERNEL_FRAME_SMALL: frame_small_kernel alone.
int enqueue_fused(const Band& b) {
    rt_ctx* ctx = b.ctx;
    const rt_dispatch::Plan& pl = b.dc.plan;
    const int32_t fmt = b.fmt;
    int rc;
    if ((rc = skip_k(ctx, b.pe_prep)) || (rc = skip_k(ctx, b.pe_coarse))) return rc;
    auto fused = pl.n_chunks == 1 ? RT_BY_FMT(frame_small_kernel, 1)
                 : pl.n_chunks == 2 || RT_FUSED_CHUNKS <= 2
                     ? RT_BY_FMT(frame_small_kernel, 2)
                     : RT_BY_FMT(frame_small_kernel, RT_FUSED_CHUNKS);
    ctx->last_kernel = RT_KERNEL_FRAME_SMALL;
    return launch_k(fused, dim3((unsigned)(pl.n_coarse * (kTiles / kFusedWaves))),
                    dim3(64 * kFusedWaves), b.stream, kernel_events(ctx, b.pe_trace, true, true),
                    b.sd, b.dir, pl.n_cx, b.width, b.row_begin, b.row_end, b.out);
}

// RT_KERNEL_TRACE_SMALL: prep_kernel -> trace_small_kernel.
int enqueue_small(const Band& b) {
    rt_ctx* ctx = b.ctx;
    const rt_dispatch::Plan& pl = b.dc.plan;
    const Workspace& ws = b.ws;
    const int32_t fmt = b.fmt;
    int rc;
    if ((rc = enqueue_prep(b, nullptr)) || (rc = skip_k(ctx, b.pe_coarse))) return rc;
    // the instance with the fewest chunk slots that holds n_chunks
    auto small = pl.n_chunks == 1   ? RT_BY_FMT(trace_small_kernel, 1)
                 : pl.n_chunks == 2 ? RT_BY_FMT(trace_small_kernel, 2)
                 : pl.n_chunks <= 4 || RT_SMALL_CHUNKS <= 4
                     ? RT_BY_FMT(trace_small_kernel, 4)
                     : RT_BY_FMT(trace_small_kernel, RT_SMALL_CHUNKS);
    ctx->last_kernel = RT_KERNEL_TRACE_SMALL;
    return launch_k(small, dim3((unsigned)(pl.n_coarse * kTiles)), dim3(64), b.stream,
                    kernel_events(ctx, b.pe_trace, true, true),
                    (const unsigned long long*)ws.row_masks,
                    (const unsigned long long*)ws.col_masks, (const int4*)ws.boxes,
                    (const Cls*)ws.cls, (const TriRec*)ws.tri, (const SphRec*)ws.sph,
                    (const float4*)ws.colours, (const unsigned*)ctx->flag, ctx->gen,
                    b.sd.n_cubes, pl.n_cx, pl.n_chunks, b.width, b.row_begin, b.row_end, b.sd,
                    b.dir, b.out);
}

// RT_KERNEL_TRACE_BIN: prep_kernel -> trace_bin_kernel.
int enqueue_trace_bin(const Band& b) {
    rt_ctx* ctx = b.ctx;
    const rt_dispatch::Plan& pl = b.dc.plan;
    const Workspace& ws = b.ws;
    const int32_t fmt = b.fmt;
    const OdSlots od = take_od_slots(ctx, b.dc.area_units);
    int rc;
    if ((rc = enqueue_prep(b, od.word)) || (rc = skip_k(ctx, b.pe_coarse))) return rc;
    auto bk = RT_BY_FMT_STORE(trace_bin_kernel);
    ctx->last_kernel = RT_KERNEL_TRACE_BIN;
    rc = launch_k(bk, dim3((unsigned)(pl.n_cx * kTiles), (unsigned)pl.n_cy), dim3(64), b.stream,
                  kernel_events(ctx, b.pe_trace, true, true), pl.n_chunks, b.width, b.row_begin,
                  b.row_end, ctx->gen, pl.n_cx, (const unsigned*)ctx->flag,
                  (const unsigned long long*)ws.row_masks,
                  (const unsigned long long*)ws.col_masks, (const int4*)ws.boxes,
                  (const Cls*)ws.cls, (const TriRec*)ws.tri, (const SphRec*)ws.sph,
                  (const float4*)ws.colours, b.sd, b.dir, b.out,
                  (const unsigned long long*)od.word, od.next, b.dc.od_lo, b.dc.od_hi,
                  verdict_word(ctx));
    return rc ? rc : copy_verdict(ctx, b.stream);
}

// RT_KERNEL_TRACE_SPLIT, RT_KERNEL_TRACE: prep_kernel -> coarse3_kernel ->
// trace3_split_kernel or trace3_kernel; without primitives, empty lists and
// the trace alone.
int enqueue_coarse(const Band& b) {
    rt_ctx* ctx = b.ctx;
    const rt_dispatch::Decision& dc = b.dc;
    const rt_dispatch::Plan& pl = dc.plan;
    const Workspace& ws = b.ws;
    const int32_t fmt = b.fmt;
    const int n_coarse = (int)pl.n_coarse;  // (choose(): the trace grid fits 32 bits)
    int rc;
    // (diagnostic builds only: the workspace keeps the last lists, so frames
    // of an unchanged scene stay exact while the skipped kernels cost nothing)
    const bool skip_prep = RT_SKIP_DIAG & 1 && ctx->od_launches > 16;
    const bool skip_coarse = RT_SKIP_DIAG & 2 && ctx->od_launches > 16;
    if (dc.feeds_overdraw) {
        const OdSlots od = take_od_slots(ctx, dc.area_units);
        if ((rc = skip_prep ? skip_k(ctx, b.pe_prep) : enqueue_prep(b, od.word))) return rc;
        const int cw = dc.coarse_waves;
        auto ck = cw == 8   ? coarse3_kernel<8>
                  : cw == 4 ? coarse3_kernel<4>
                  : cw == 2 ? coarse3_kernel<2>
                            : coarse3_kernel<1>;
        rc = skip_coarse
                 ? skip_k(ctx, b.pe_coarse)
                 : launch_k(ck, dim3((unsigned)n_coarse), dim3(64 * cw), b.stream,
                            kernel_events(ctx, b.pe_coarse, true, false), (const int4*)ws.boxes,
                            (const Cls*)ws.cls, (const SphRec*)ws.sph, (const TriDepth*)ws.tdep,
                            pl.n_prims, pl.n_tri, pl.n_cx, n_coarse,
                            (const unsigned long long*)ws.row_masks,
                            (const unsigned long long*)ws.col_masks, b.row_begin, pl.half_cap,
                            (const unsigned*)ctx->flag, ctx->gen, ctx->knobs.coarse_cull,
                            dc.cull_tri, (const unsigned long long*)od.word, dc.od_min, od.next,
                            ws.counts, ws.lists, dc.od_lo, dc.od_hi, verdict_word(ctx));
        if (rc) return rc;
    } else {
        if ((rc = skip_k(ctx, b.pe_prep))) return rc;
        HIP_TRY(hipMemsetAsync(ws.counts, 0, sizeof(int) * (size_t)n_coarse, b.stream));
        if ((rc = skip_k(ctx, b.pe_coarse))) return rc;
    }
    const dim3 trace_grid((unsigned)(pl.n_cx * kTiles), (unsigned)pl.n_cy);
    ctx->last_kernel = dc.chain;
    if (dc.chain == RT_KERNEL_TRACE_SPLIT) {
        auto sk = RT_BY_FMT_STORE(trace3_split_kernel);
        rc = launch_k(sk, trace_grid, dim3(64 * dc.split), b.stream,
                      kernel_events(ctx, b.pe_trace, true, true), b.sd, (const TriRec*)ws.tri,
                      (const SphRec*)ws.sph, (const float4*)ws.colours, (const int*)ws.counts,
                      (const int*)ws.lists, pl.half_cap, b.dir, b.width, b.row_begin, b.row_end,
                      pl.n_cx, b.out);
    } else {
#if RT_DIAG
        // diagnostics build: the trace-kernel ablations (rt_debug_set_trace_mode)
        auto kern = ctx->trace_mode == 1   ? RT_TRACE3_BY_FMT(1)
                    : ctx->trace_mode == 2 ? RT_TRACE3_BY_FMT(2)
                    : ctx->trace_mode == 3 ? RT_TRACE3_BY_FMT(3)
                    : ctx->trace_mode == 4 ? RT_TRACE3_BY_FMT(4)
                                           : RT_TRACE3_BY_FMT(0);
#else
        auto kern = RT_TRACE3_BY_FMT(0);
#endif
        const int n_tiles_x = (b.width + kWaveTile - 1) / kWaveTile;
        rc = launch_k(kern, trace_grid, dim3(64), b.stream,
                      kernel_events(ctx, b.pe_trace, true, true), (const int*)ws.counts,
                      (const int*)ws.lists, (const TriRec*)ws.tri, (const SphRec*)ws.sph, pl.n_cx,
                      pl.half_cap, b.width, b.row_begin, b.row_end, b.sd.n_cubes,
                      (const float4*)ws.colours, b.out, b.sd, b.dir, n_tiles_x, fmt);
    }
    return rc ? rc : copy_verdict(ctx, b.stream);
}

// Enqueue one render of rows [row_begin, row_end) on `stream`: the chain
// rt_dispatch::choose() picks.  All scene pointers are device pointers.
int launch(rt_ctx* ctx, const rt_scene* s, const float d[4], const float* origins,
           int32_t width, int32_t row_begin, int32_t row_end, int32_t fmt,
           int32_t path, void* out, hipStream_t stream, int32_t* used_path) {
    const int32_t rows = row_end - row_begin;
    const unsigned verdict =
        ctx->od_verdict ? *reinterpret_cast<volatile unsigned*>(ctx->od_verdict) : 0u;
    rt_dispatch::Decision dc;
    int rc = rt_dispatch::choose(kGeometry, ctx->knobs, ctx->n_cu, fmt, s->num_spheres,
                                 s->num_cubes, width, rows, binned_ok(d, origins), path, verdict,
                                 ctx->trace_mode, &dc, ctx->working_set);
    if (rc) return rc;
    if (dc.chain != RT_KERNEL_NONE) ctx->last_store_policy = dc.store_policy;
    if (used_path) *used_path = dc.chain == RT_KERNEL_GENERIC ? RT_PATH_GENERIC : RT_PATH_BINNED;
    if (dc.band_rows < rows) {
        // internal bands, each a band render, in order on the same stream
        const size_t px_bytes = rt_args::pixel_bytes(fmt);
        const int32_t prof_count0 = ctx->prof_count;
        for (int64_t rb = row_begin; rb < row_end; rb += dc.band_rows) {
            const int32_t re = (int32_t)std::min<int64_t>(rb + dc.band_rows, row_end);
            char* dst = static_cast<char*>(out) + (size_t)(rb - row_begin) * width * px_bytes;
            rc = launch(ctx, s, d, origins, width, (int32_t)rb, re, fmt, path, dst, stream, nullptr);
            if (rc) return rc;
        }
        if (ctx->profile) ctx->prof_count = prof_count0 + 1;  // one render, summed bands
        return RT_OK;
    }
    const hipEvent_t* pe = nullptr;  // 6 events: prep, coarse, trace (start, stop)
    if (ctx->profile) {
        while (ctx->prof_events.size() < ctx->prof_used + 6) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            ctx->prof_events.push_back(e);
        }
        ctx->prof_skipped.resize(ctx->prof_events.size() / 2);
        for (int k = 0; k < 3; ++k) ctx->prof_skipped[ctx->prof_used / 2 + k] = 0;
        pe = &ctx->prof_events[ctx->prof_used];
        ctx->prof_used += 6;
        ++ctx->prof_count;
    }
    const hipEvent_t* pe_coarse = pe ? pe + 2 : nullptr;
    const hipEvent_t* pe_trace = pe ? pe + 4 : nullptr;
    const SceneDev sd{reinterpret_cast<const float4*>(s->sphere_origins), s->sphere_radius,
                      reinterpret_cast<const float4*>(s->sphere_colours),
                      reinterpret_cast<const float4*>(s->cube_vertices),
                      reinterpret_cast<const float4*>(s->cube_colours), s->num_spheres,
                      s->num_cubes};
    const float4 dir = make_float4(d[0], d[1], d[2], d[3]);
    if (dc.chain == RT_KERNEL_GENERIC) {
        const int64_t n = (int64_t)width * rows;
        const int64_t blocks = std::min<int64_t>((n + kThreads - 1) / kThreads, (int64_t)1 << 20);
        if ((rc = skip_k(ctx, pe)) || (rc = skip_k(ctx, pe_coarse))) return rc;
        ctx->last_kernel = RT_KERNEL_GENERIC;
        return launch_k(generic_kernel, dim3((unsigned)blocks), dim3(kThreads), stream,
                        kernel_events(ctx, pe_trace, true, true), sd, dir,
                        reinterpret_cast<const float4*>(origins), width, row_begin, row_end, fmt,
                        out);
    }
    // the workspace (grow-only: after rt_reserve, or a first frame, no allocation)
    if ((rc = ensure(&ctx->rec_buf, &ctx->rec_cap, dc.plan.rec_need)) ||
        (rc = ensure(&ctx->list_buf, &ctx->list_cap, dc.plan.list_need)))
        return rc;
    // generation-stamped non-finite flag: no per-launch memset needed
    if (++ctx->gen == 0) {
        HIP_TRY(hipMemsetAsync(ctx->flag, 0, sizeof(unsigned), stream));
        ctx->gen = 1;
    }
    const Band band{ctx, stream, sd, dir, width, row_begin, row_end, fmt, out,
                    pe, pe_coarse, pe_trace, dc, carve(ctx, dc.plan)};
    switch (dc.chain) {
    case RT_KERNEL_FRAME_SMALL: return enqueue_fused(band);
    case RT_KERNEL_TRACE_SMALL: return enqueue_small(band);
    case RT_KERNEL_TRACE_BIN: return enqueue_trace_bin(band);
    default: return enqueue_coarse(band);  // RT_KERNEL_TRACE_SPLIT, RT_KERNEL_TRACE
    }
}

}  // namespace
