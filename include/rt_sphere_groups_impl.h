/*
 * rt_sphere_groups_impl.h -- the sphere cull of the ray queries,
 * rt_sphere_groups_build* and rt_cast_rays_grouped* / rt_occlude_rays_grouped* /
 * rt_cast_camera_grouped* (DESIGN.md §3.1j): the key, the order and the record
 * of a group of nearby spheres, the keep test and the host's cull policy that
 * puts it into the walks of rt_light_impl.h, one text for the host functions
 * (csrc/rt_sphere_groups.cpp) and the kernels (csrc/rt_sphere_groups.hip, whose
 * policy has the wave's group loop), and their shared argument checks.  The cube
 * phase is rt_accel_impl.h's, the exact sphere tests are rt_light_impl.h's
 * bounce_sphere and occluded_by_sphere, as they are.  Internal: not installed,
 * not part of the ABI.
 *
 * The conventions are rt_light_impl.h's: every operation is written on its own
 * and rounds once, no contraction, sums in the written order.  Why the keep
 * test never drops a group with a member the exact test accepts is DESIGN.md §4.
 */
#ifndef RT_SPHERE_GROUPS_IMPL_H
#define RT_SPHERE_GROUPS_IMPL_H

#include "rt_accel_impl.h"

namespace rt_light {

/* The checks of rt_sphere_groups_build* (RT_OK or RT_ERR_INVALID_ARG): a NULL
 * scene, the scene checks of check_rays(), group_size outside 1..8, and with
 * num_spheres > 0 a NULL or misaligned (16 bytes) `out`.
 * csrc/rt_sphere_groups.cpp. */
int check_sphere_groups_build(const rt_scene* scene, int32_t group_size,
                              const rt_sphere_group* out);
/* What the *_grouped calls check after the *_accel call's checks: num_groups
 * is the record count of some group_size in 1..8 (0 without spheres), and with
 * num_spheres > 0 `groups` is neither NULL nor misaligned (16 bytes).  `scene`
 * is not NULL. */
int check_sphere_groups(const rt_scene* scene, const rt_sphere_group* groups, int32_t num_groups);

constexpr int32_t kGroupMax = 8;                 // members of a record
constexpr uint32_t kGroupKeyLast = 0x7fffffffu;  // a non-finite sphere's key: behind every cell's
// The constants of the keep test.
constexpr double kGroupC = 0x1p-9;      // the margin over (T1 + rmax); the proof needs 1.39e-3
constexpr double kGroupSmall = 0x1p-29; // below it a product of the fp32 test can underflow
constexpr double kGroupBig = 0x1p62;    // from it on one can overflow

RT_LIGHT_FN int32_t sphere_groups_count(int32_t num_spheres, int32_t group_size) {
    if (num_spheres < 0 || group_size < 1 || group_size > kGroupMax) return -1;
    return static_cast<int32_t>((static_cast<int64_t>(num_spheres) + (group_size - 1)) /
                                group_size);
}

RT_LIGHT_FN int64_t sphere_groups_workspace_bytes(int32_t num_spheres) {
    if (num_spheres < 0) return -1;
    return (16 + 8 * static_cast<int64_t>(num_spheres) + 15) / 16 * 16;
}

// One float step towards -inf (f not NaN, not -inf): the next bit pattern for a
// negative f, the previous one for a positive f, the smallest negative
// subnormal for a zero.
RT_LIGHT_FN float float_pred(float f) {
    union {
        float f;
        uint32_t u;
    } b;
    b.f = f;
    if ((b.u << 1) == 0u)
        b.u = 0x80000001u;
    else if (b.u >> 31)
        b.u += 1u;
    else
        b.u -= 1u;
    return b.f;
}

// A double of either sign to float, rounded down: to nearest, then one step
// down where that is above the double.  NaN stays NaN, -inf stays -inf.
RT_LIGHT_FN float float_floor(double x) {
    const float f = static_cast<float>(x);
    return static_cast<double>(f) > x ? float_pred(f) : f;
}

// ... rounded up: the mirror image.
RT_LIGHT_FN float float_ceil(double x) { return -float_floor(-x); }

RT_LIGHT_FN bool sphere_finite(const float* centre, float r) {
    return finite_f(centre[0]) && finite_f(centre[1]) && finite_f(centre[2]) && finite_f(r);
}

// What the keys are scaled by: the per-axis minimum of the finite spheres'
// centres and the largest of the three extents max - min (fp32 subtractions).
// No finite sphere: all 0.
struct GroupFrame {
    float mn[3];
    float ext;
};

// `mn` / `mx`: the minima and maxima; `any`: is there a finite sphere.
RT_LIGHT_FN GroupFrame group_frame(const float* mn, const float* mx, bool any) {
    GroupFrame f{{0.0f, 0.0f, 0.0f}, 0.0f};
    if (!any) return f;
    for (int c = 0; c < 3; ++c) {
        f.mn[c] = mn[c];
        const float e = mx[c] - mn[c];
        if (e > f.ext) f.ext = e;
    }
    return f;
}

// The 10-bit cell of one coordinate: floor(((x - mn) / ext) * 1023), clamped
// to 0..1023; extent 0 (and a NaN or negative quotient) gives cell 0.
RT_LIGHT_FN uint32_t group_cell(float x, float mn, float ext) {
    if (!(ext > 0.0f)) return 0u;
    const float rel = x - mn;
    const float q = rel / ext;
    const float s = q * 1023.0f;
    if (s >= 1023.0f) return 1023u;
    return s >= 0.0f ? static_cast<uint32_t>(static_cast<int32_t>(s)) : 0u;
}

// Bit i of a 10-bit cell to bit 3 i.
RT_LIGHT_FN uint32_t spread3(uint32_t v) {
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// The 30-bit Morton key of a sphere: x in bits 0, 3, ..., y in 1, 4, ..., z in
// 2, 5, ...; a sphere with a non-finite centre or radius sorts last.
RT_LIGHT_FN uint32_t sphere_key(const float* centre, float r, const GroupFrame& f) {
    if (!sphere_finite(centre, r)) return kGroupKeyLast;
    return spread3(group_cell(centre[0], f.mn[0], f.ext)) |
           (spread3(group_cell(centre[1], f.mn[1], f.ext)) << 1) |
           (spread3(group_cell(centre[2], f.mn[2], f.ext)) << 2);
}

// One member's box along one axis: centre -+ |r| in double (one rounding),
// then outwards to float.
RT_LIGHT_FN float member_lo(float c, float r) {
    return float_floor(static_cast<double>(c) - abs_d(static_cast<double>(r)));
}
RT_LIGHT_FN float member_hi(float c, float r) {
    return float_ceil(static_cast<double>(c) + abs_d(static_cast<double>(r)));
}

// The record of the `count` (1..8) spheres at positions `order[0 .. count)` of
// the sorted order: a pure function of those spheres and their indices.  The
// kernel of rt_sphere_groups.hip computes the same values across eight lanes:
// min, max and the ascending order of distinct indices do not depend on the
// order they are met in.
RT_LIGHT_FN rt_sphere_group sphere_group(const float* sphere_origins, const float* sphere_radius,
                                         const int32_t* order, int32_t count) {
    rt_sphere_group g;
    const float inf = static_cast<float>(kAccelInf);
    g.count = count;
    for (int k = 0; k < kGroupMax; ++k) g.member[k] = -1;
    for (int k = 0; k < count; ++k) {  // insertion into ascending order
        int at = k;
        while (at > 0 && g.member[at - 1] > order[k]) {
            g.member[at] = g.member[at - 1];
            --at;
        }
        g.member[at] = order[k];
    }
    bool finite = true;
    for (int k = 0; k < count; ++k) {
        const int64_t i = order[k];
        finite = finite && sphere_finite(sphere_origins + 4 * i, sphere_radius[i]);
    }
    if (!finite) {  // always kept: rmax fails the keep test's precondition
        for (int c = 0; c < 3; ++c) g.lo[c] = -inf, g.hi[c] = inf;
        g.rmax = inf;
        return g;
    }
    g.rmax = 0.0f;
    for (int c = 0; c < 3; ++c) g.lo[c] = inf, g.hi[c] = -inf;
    for (int k = 0; k < count; ++k) {
        const int64_t i = order[k];
        const float* ctr = sphere_origins + 4 * i;
        const float r = sphere_radius[i];
        const float ar = fabsf(r);
        if (ar > g.rmax) g.rmax = ar;
        for (int c = 0; c < 3; ++c) {
            const float l = member_lo(ctr[c], r), h = member_hi(ctr[c], r);
            if (l < g.lo[c]) g.lo[c] = l;
            if (h > g.hi[c]) g.hi[c] = h;
        }
    }
    // (+ 0.0f: a zero bound is +0 whichever of -0 and +0 the order met first)
    for (int c = 0; c < 3; ++c) g.lo[c] = g.lo[c] + 0.0f, g.hi[c] = g.hi[c] + 0.0f;
    return g;
}

// slab_misses of rt_accel_impl.h for any box lo / hi (three floats each) and
// any parameter range [t_near, t_far]: is it proven that that range of the ray
// misses the box grown by `delta` on every side?  The same operations in the
// same order; a comparison that meets a NaN proves nothing.
RT_LIGHT_FN bool slab_misses(const double* o, const double* d, const float* lo, const float* hi,
                             double delta, double t_near, double t_far) {
    double tn = t_near, tf = t_far;
    bool miss = false;
    for (int c = 0; c < 3; ++c) {
        const double L = static_cast<double>(lo[c]) - delta;
        const double H = static_cast<double>(hi[c]) + delta;
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

// May any member of the group be accepted by bounce_sphere (segment = false)
// or occluded_by_sphere (segment = true) for the ray (o, d), the doubles of the
// ray's floats?  Never false where either accepts one; true
// whenever a miss is not proven: outside the fallback domain, and wherever a
// comparison meets a NaN.
//
// The one ground for a rejection is that the whole LINE of the ray misses the
// grown box: then the fp32 discriminant of every member is negative, whatever
// the roots would have been, so the cast's and the segment's test are the same
// and `segment` changes nothing.  The grounds that look at the parameters of
// the box (wholly behind the origin, wholly past the segment's end) are not
// built: DESIGN.md §8.
RT_LIGHT_FN bool group_kept(const double* o, const double* d, const rt_sphere_group& g,
                            bool segment) {
    (void)segment;
    const double D1 = (abs_d(d[0]) + abs_d(d[1])) + abs_d(d[2]);
    const double O1 = (abs_d(o[0]) + abs_d(o[1])) + abs_d(o[2]);
    double T1 = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double a = abs_d(o[c] - static_cast<double>(g.lo[c]));
        const double h = abs_d(o[c] - static_cast<double>(g.hi[c]));
        T1 = T1 + (a > h ? a : h);
    }
    const double M = T1 + static_cast<double>(g.rmax);
    const double margin = kGroupC * M;
    // the fallback domain: a non-finite ray or an always-kept record (M is inf
    // or NaN), a = 0 and every magnitude at which a product of the fp32 test
    // can underflow or overflow
    if (!(D1 >= kGroupSmall) || !(D1 < kGroupBig) || !(O1 < kAccelInf) || !(M < kGroupBig) ||
        !(D1 * M < kGroupBig) || !(margin >= kGroupSmall))
        return true;
    const double delta = margin + kAccelK2 * (M + O1);
    return !slab_misses(o, d, g.lo, g.hi, delta, -kAccelInf, kAccelInf);
}

// Does a sphere candidate (parameter sf, object id `id`) replace the best so
// far?  Iff it is closer, or as close and the best is a sphere of larger index:
// the first minimum in index order, in whatever order the groups come (§4).
// Cubes come first and keep their ties.
RT_LIGHT_FN bool sphere_takes(const Bounce& b, float sf, int32_t id, int32_t num_cubes) {
    return sf < b.best || (sf == b.best && b.obj2 >= num_cubes && b.obj2 > id);
}

// CubeCull's cube phase, and the sphere phase of both walks with the groups the
// keep test drops left out.
struct GroupCull {
    static constexpr bool kGroups = true;
    const rt_cube_bound* accel;
    const rt_sphere_group* groups;
    int32_t num_groups;
    RT_LIGHT_FN bool cube(const double* o, const double* d, int32_t j, bool segment) const {
        return cube_kept(o, d, accel[j], segment);
    }
    // bounce_walk's sphere phase: `b` is the best of the cubes.
    RT_LIGHT_FN Bounce bounce_spheres(const rt_scene& s, const double* pd, const double* Rd,
                                      int32_t obj, Vec3 p, Vec3 R, Bounce b) const {
        float sf;
        for (int32_t g = 0; g < num_groups; ++g) {
            const rt_sphere_group& G = groups[g];
            if (!group_kept(pd, Rd, G, false)) continue;
            for (int k = 0; k < kGroupMax && k < G.count; ++k) {
                const int32_t i = G.member[k];
                // (a foreign record's index is no sphere)
                if (static_cast<uint32_t>(i) >= static_cast<uint32_t>(s.num_spheres)) continue;
                if (static_cast<int64_t>(s.num_cubes) + i == obj) continue;
                if (bounce_sphere(p, R, s.sphere_origins + 4 * static_cast<int64_t>(i),
                                  s.sphere_radius[i], &sf) &&
                    sphere_takes(b, sf, s.num_cubes + i, s.num_cubes))
                    b = Bounce{sf, s.num_cubes + i, -1};
            }
        }
        return b;
    }
    // light_occluded's sphere phase.
    RT_LIGHT_FN bool occluded_by_spheres(const rt_scene& s, const double* pd, const double* Ld,
                                         int32_t obj, Vec3 p, Vec3 L) const {
        for (int32_t g = 0; g < num_groups; ++g) {
            const rt_sphere_group& G = groups[g];
            if (!group_kept(pd, Ld, G, true)) continue;
            for (int k = 0; k < kGroupMax && k < G.count; ++k) {
                const int32_t i = G.member[k];
                if (static_cast<uint32_t>(i) >= static_cast<uint32_t>(s.num_spheres)) continue;
                if (static_cast<int64_t>(s.num_cubes) + i == obj) continue;
                if (occluded_by_sphere(p, L, s.sphere_origins + 4 * static_cast<int64_t>(i),
                                       s.sphere_radius[i]))
                    return true;
            }
        }
        return false;
    }
};

// The pair of walks of the *_grouped calls.  GroupedWalks{accel, groups, num_groups}.
using GroupedWalks = WalksOver<GroupCull>;

}  // namespace rt_light

#endif /* RT_SPHERE_GROUPS_IMPL_H */
