/*
 * rt_accel_impl.h -- the cube cull of the ray queries, rt_accel_build* and
 * rt_cast_rays_accel* / rt_occlude_rays_accel* / rt_cast_camera_accel*
 * (DESIGN.md §3.1g): the record of one cube, the keep test and the cull policy
 * that puts it into the walks of rt_light_impl.h, one text for the host
 * functions (csrc/rt_accel.cpp) and the kernels (csrc/rt_accel.hip and the
 * culled light pass), and their shared argument checks.  The exact
 * tests are rt_light_impl.h's bounce_tri, occluded_by_tri and the sphere tests,
 * as they are.  Internal: not installed, not part of the ABI.
 *
 * The conventions are rt_light_impl.h's: every operation is written on its own
 * and rounds once, no contraction, sums in the written order.  Why the keep
 * test never drops a cube the exact test accepts is DESIGN.md §4.
 */
#ifndef RT_ACCEL_IMPL_H
#define RT_ACCEL_IMPL_H

#include "rt_rays_impl.h"

namespace rt_light {

/* The checks of rt_accel_build* (RT_OK or RT_ERR_INVALID_ARG): a NULL scene,
 * the scene checks of check_rays(), and with num_cubes > 0 a NULL or
 * misaligned (16 bytes) `out`.  csrc/rt_accel.cpp. */
int check_accel_build(const rt_scene* scene, const rt_cube_bound* out);
/* What the *_accel calls check after their unculled call's checks: with
 * num_cubes > 0 a NULL or misaligned (16 bytes) `accel`.  `scene` is not NULL. */
int check_accel(const rt_scene* scene, const rt_cube_bound* accel);

// The constants of the keep test.  eta = 2^-53.
constexpr double kAccelInf = __builtin_huge_val();
constexpr double kAccelEps = 0x1p-48;           // 32 eta: a det's error in units of |d|_1 * emax2
constexpr double kAccelCoarseEps = 0.5e-6;      // the coarse stage is tried up to this error
constexpr double kAccelK1 = 0x1p-46;            // 128 eta: the margin's part over |det|
constexpr double kAccelK2 = 0x1p-50;            // 8 eta: its additive part
constexpr double kAccelSlab = 0x1p-50;          // 8 eta: the slab test's own rounding
constexpr double kAccelEdgeUp = 1.0 + 0x1p-20;  // sqrtf(emax2) to an upper bound of the edge

// A double to float, rounded up: to nearest, then one ulp up where that is
// below the double.  For x >= 0 (NaN stays NaN, +inf stays +inf).
RT_LIGHT_FN float float_up(double x) {
    float f = static_cast<float>(x);
    if (static_cast<double>(f) < x) {
        // (f >= 0 and finite: the next float up is the next bit pattern)
        union {
            float f;
            uint32_t u;
        } b;
        b.f = f;
        b.u += 1u;
        f = b.f;
    }
    return f;
}

// The squared length of the edge from vertex a to vertex b (float4 each), in double.
RT_LIGHT_FN double edge_len2(const float* a, const float* b) {
    const double ex = static_cast<double>(b[0]) - static_cast<double>(a[0]);
    const double ey = static_cast<double>(b[1]) - static_cast<double>(a[1]);
    const double ez = static_cast<double>(b[2]) - static_cast<double>(a[2]);
    return (ex * ex + ey * ey) + ez * ez;
}

// e1 x e2 of one triangle (three float4 at `tri`), e1 = v1 - v0 and
// e2 = v2 - v0 as intersect_tri forms them, in double.
RT_LIGHT_FN void tri_normal(const float* tri, double* n) {
    const double e1[3] = {static_cast<double>(tri[4]) - static_cast<double>(tri[0]),
                          static_cast<double>(tri[5]) - static_cast<double>(tri[1]),
                          static_cast<double>(tri[6]) - static_cast<double>(tri[2])};
    const double e2[3] = {static_cast<double>(tri[8]) - static_cast<double>(tri[0]),
                          static_cast<double>(tri[9]) - static_cast<double>(tri[1]),
                          static_cast<double>(tri[10]) - static_cast<double>(tri[2])};
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

RT_LIGHT_FN bool finite_f(float x) { return x - x == 0.0f; }

// The record of one cube (float4[36] at `verts`): a pure function of its 36
// vertices.  The kernel of rt_accel.hip computes the same values across the
// lanes of a wave: min, max and the largest edge do not depend on the order.
RT_LIGHT_FN rt_cube_bound cube_bound(const float* verts) {
    rt_cube_bound b;
    bool finite = true;
    for (int i = 0; i < 36; ++i)
        for (int c = 0; c < 3; ++c) finite = finite && finite_f(verts[4 * i + c]);
    if (!finite) {  // always kept: emax2 fails the keep test's precondition
        const float inf = static_cast<float>(kAccelInf);
        b = rt_cube_bound{{-inf, -inf, -inf}, inf, {inf, inf, inf}, 0.0f, {}};  // normals 0
        return b;
    }
    for (int c = 0; c < 3; ++c) b.lo[c] = b.hi[c] = verts[c];
    for (int i = 1; i < 36; ++i)
        for (int c = 0; c < 3; ++c) {
            const float x = verts[4 * i + c];
            if (x < b.lo[c]) b.lo[c] = x;
            if (x > b.hi[c]) b.hi[c] = x;
        }
    // (+ 0.0f: a zero bound is +0 whichever of -0 and +0 the order met first)
    for (int c = 0; c < 3; ++c) b.lo[c] = b.lo[c] + 0.0f, b.hi[c] = b.hi[c] + 0.0f;
    double emax = 0.0;
    for (int k = 0; k < 12; ++k) {
        const float* t = verts + 12 * k;
        const double l1 = edge_len2(t, t + 4), l2 = edge_len2(t, t + 8);
        if (l1 > emax) emax = l1;
        if (l2 > emax) emax = l2;
        tri_normal(t, b.normal[k]);
    }
    b.emax2 = float_up(emax);
    b.reserved = 0.0f;
    return b;
}

RT_LIGHT_FN double abs_d(double x) { return fabs(x); }

// How the loop over the record's twelve normals in cube_kept is compiled:
// nothing (the compiler's choice: unrolled whole, the record in flight at once)
// or a loop pragma of the including translation unit, which changes the
// instruction schedule and nothing that is computed.
#ifndef RT_ACCEL_NORMALS_LOOP
#define RT_ACCEL_NORMALS_LOOP
#endif

// Is it proven that the parameter range [0, inf) (segment: [0, 1]) of the ray
// misses the record's box grown by `delta` on every side?  The slab test, one
// reciprocal per axis; a comparison that meets a NaN proves nothing.
RT_LIGHT_FN bool slab_misses(const double* o, const double* d, const rt_cube_bound& b,
                             double delta, bool segment) {
    double tn = 0.0, tf = segment ? 1.0 : kAccelInf;
    bool miss = false;
    for (int c = 0; c < 3; ++c) {
        const double L = static_cast<double>(b.lo[c]) - delta;
        const double H = static_cast<double>(b.hi[c]) + delta;
        if (d[c] == 0.0) {
            if (o[c] < L || o[c] > H) miss = true;
        } else {
            const double inv = 1.0 / d[c];  // (three roundings per t)
            const double t1 = (L - o[c]) * inv;
            const double t2 = (H - o[c]) * inv;
            const double lo_t = t1 < t2 ? t1 : t2;
            const double hi_t = t1 < t2 ? t2 : t1;
            if (lo_t > tn) tn = lo_t;
            if (hi_t < tf) tf = hi_t;
        }
    }
    if (tn - tf > kAccelSlab * (abs_d(tn) + abs_d(tf))) miss = true;
    return miss;
}

// May any of the cube's 12 triangles be accepted by bounce_tri (segment =
// false: td > 0) or occluded_by_tri (segment = true: 0 < td < 1) for the ray
// (o, d), the doubles of the ray's floats?  Never false where the exact test
// accepts one; true whenever a miss is not proven: outside the
// fallback domain, and wherever a comparison meets a NaN.
RT_LIGHT_FN bool cube_kept(const double* o, const double* d, const rt_cube_bound& b,
                           bool segment) {
    const double E2 = static_cast<double>(b.emax2);
    const double D1 = (abs_d(d[0]) + abs_d(d[1])) + abs_d(d[2]);
    const double O1 = (abs_d(o[0]) + abs_d(o[1])) + abs_d(o[2]);
    // what the computed det of a triangle and d . n can each be off the true det by, together
    const double eps = kAccelEps * (D1 * E2);
    // the fallback domain, first part: a non-finite ray, an always-kept
    // record, magnitudes whose error bound overflows
    if (!(D1 < kAccelInf) || !(O1 < kAccelInf) || !(eps < kAccelInf)) return true;
    double T1 = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double a = abs_d(o[c] - static_cast<double>(b.lo[c]));
        const double h = abs_d(o[c] - static_cast<double>(b.hi[c]));
        T1 = T1 + (a > h ? a : h);
    }
    const double E = static_cast<double>(sqrtf(b.emax2)) * kAccelEdgeUp;
    const double M = (T1 + E) + (segment ? D1 : 0.0);  // (the end point's slack is the segment's)
    const double load = kAccelK1 * ((D1 * E2) * M);    // the margin is load / |det| + slack
    const double slack = kAccelK2 * (M + O1);
    // first with the margin of the smallest |det| any accepted triangle can
    // have, 1e-6 less the error of the computed det: no normal is read.  Tried
    // only where that margin is below the cube's edge (camera rays; not the
    // long shadow segments, whose margin of this kind exceeds the scene).
    if (eps <= kAccelCoarseEps && load <= (kEpsilon - eps) * E &&
        slab_misses(o, d, b, load / (kEpsilon - eps) + slack, segment))
        return false;
    // the smallest |d . n| among the triangles whose computed |det| can reach
    // 1e-6; second part of the fallback domain: one of them so close to
    // grazing that d . n says nothing about its det
    const double skip_below = kEpsilon - eps;
    const double graze_below = 4.0 * eps;
    double g = kAccelInf, asum = 0.0;
    bool graze = false;
    RT_ACCEL_NORMALS_LOOP
    for (int k = 0; k < 12; ++k) {
        const double q = (d[0] * b.normal[k][0] + d[1] * b.normal[k][1]) + d[2] * b.normal[k][2];
        const double a = abs_d(q);
        asum = asum + a;
        if (a < skip_below) continue;
        if (!(a >= graze_below)) graze = true;
        if (a < g) g = a;
    }
    if (!(asum < kAccelInf) || graze) return true;  // (NaN or inf normals: a foreign record)
    if (g == kAccelInf) return false;  // every triangle's |det| is below 1e-6: none accepts
    g = g - eps;
    return !slab_misses(o, d, b, load / g + slack, segment);
}

// The cull policy of rt_light_impl.h's walks over the prebuilt records: a cube
// the keep test drops is left out; the same order, the same rule, the unculled
// sphere loop.
struct CubeCull {
    static constexpr bool kGroups = false;
    const rt_cube_bound* accel;
    RT_LIGHT_FN bool cube(const double* o, const double* d, int32_t j, bool segment) const {
        return cube_kept(o, d, accel[j], segment);
    }
};
RT_LIGHT_FN CubeCull cull_of(const rt_cube_bound* accel) { return CubeCull{accel}; }
inline int check_cull(const rt_scene* scene, CubeCull cull) {
    return check_accel(scene, cull.accel);
}

// rt_light_impl.h's Walks over the two culled walks: what the pixel functions
// of the *_accel light pass take.  CulledWalks{accel}.
using CulledWalks = WalksOver<CubeCull>;

}  // namespace rt_light

#endif /* RT_ACCEL_IMPL_H */
