"""The culled ray queries -- TEST INFRASTRUCTURE ONLY.

A numpy restatement of DESIGN.md §3.1g / §4 for rt_accel_build / rt_accel_kept /
rt_cast_rays_accel / rt_occlude_rays_accel: the record of a cube, the keep test
(one ufunc per written operation of include/rt_accel_impl.h, float64 where the
text is double, in the written order; numpy never contracts) and the culled
walks as thin layers over `reflect_ref.tri_sf` / `sphere_sf` and
`shadow_ref.tri_occludes` / `sphere_occludes`, as they are.

`ref_line_hits_box` is a deliberately independent, loose yardstick in plain
float64 (parametric clipping, not the keep test's slabs): the tests hold the
keep test between the exact triangle tests from below and this from above.
"""
import numpy as np

import rays_ref as yr
import reflect_ref as rr
import shadow_ref as sr
from gpu_support import F32
from hit_ref import K_FAR, hit_dtype

F64 = np.float64
INF = np.inf
EPS = 2.0 ** -48
K_EPSILON = 0.000001
COARSE_EPS = 0.5e-6
K1, K2, SLAB = 2.0 ** -46, 2.0 ** -50, 2.0 ** -50
EDGE_UP = 1.0 + 2.0 ** -20


def bound_dtype():
    return np.dtype([("lo", "<f4", (3,)), ("emax2", "<f4"), ("hi", "<f4", (3,)),
                     ("reserved", "<f4"), ("normal", "<f8", (12, 3))])


def float_up(x):
    """double -> float, to nearest, then one ulp up where that is below."""
    with np.errstate(all="ignore"):
        f = x.astype(F32)
        low = f.astype(F64) < x
        return np.where(low, (f.view(np.uint32) + np.uint32(1)).view(F32), f).astype(F32)


def records(cube_vertices):
    """rt_accel_build: one record per cube of float4[36] vertices."""
    v = np.ascontiguousarray(cube_vertices, F32).reshape(-1, 36, 4)
    out = np.zeros(len(v), bound_dtype())
    if not len(v):
        return out
    with np.errstate(all="ignore"):
        xyz = v[:, :, :3]
        finite = np.isfinite(xyz).all((1, 2))
        lo, hi = xyz.min(1) + F32(0.0), xyz.max(1) + F32(0.0)
        d = xyz.astype(F64)
        v0, v1, v2 = d[:, 0::3], d[:, 1::3], d[:, 2::3]  # (cubes, 12, 3)
        e1, e2 = v1 - v0, v2 - v0
        l1 = (e1[..., 0] * e1[..., 0] + e1[..., 1] * e1[..., 1]) + e1[..., 2] * e1[..., 2]
        l2 = (e2[..., 0] * e2[..., 0] + e2[..., 1] * e2[..., 1]) + e2[..., 2] * e2[..., 2]
        emax = np.maximum(l1, l2).max(1)
        n = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1],
                      e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                      e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], -1)
        emax2 = float_up(np.where(finite, emax, 0.0))
    f = finite[:, None]
    out["lo"] = np.where(f, lo, F32(-INF))
    out["hi"] = np.where(f, hi, F32(INF))
    out["emax2"] = np.where(finite, emax2, F32(INF))
    out["normal"] = np.where(finite[:, None, None], n, 0.0)
    return out


def _terms(o, d, rec, segment):
    """The keep test's quantities up to delta, for rays (o, d: three float32
    arrays each) and one record."""
    o = [np.asarray(a, F32).astype(F64) for a in o]
    d = [np.asarray(a, F32).astype(F64) for a in d]
    lo, hi = rec["lo"].astype(F64), rec["hi"].astype(F64)
    with np.errstate(all="ignore"):
        E2 = F64(rec["emax2"])
        D1 = (np.abs(d[0]) + np.abs(d[1])) + np.abs(d[2])
        O1 = (np.abs(o[0]) + np.abs(o[1])) + np.abs(o[2])
        eps = EPS * (D1 * E2)
        finite = (D1 < INF) & (O1 < INF) & (eps < INF)
        fallback = ~finite
        T1 = np.zeros_like(D1)
        for c in range(3):
            a, h = np.abs(o[c] - lo[c]), np.abs(o[c] - hi[c])
            T1 = T1 + np.where(a > h, a, h)
        skip_below, graze_below = K_EPSILON - eps, 4.0 * eps
        g, asum = np.full_like(D1, INF), np.zeros_like(D1)
        graze = np.zeros(D1.shape, bool)
        for k in range(12):
            n = rec["normal"][k]
            q = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]
            a = np.abs(q)
            asum = asum + a
            counts = ~(a < skip_below)
            graze |= counts & ~(a >= graze_below)
            g = np.where(counts & (a < g), a, g)
        fallback = fallback | ~(asum < INF) | graze
        none = g == INF
        g = g - eps
        E = F64(np.sqrt(F32(rec["emax2"]))) * EDGE_UP
        M = (T1 + E) + (D1 if segment else 0.0)
        load = K1 * ((D1 * E2) * M)
        slack = K2 * (M + O1)
        tried = (eps <= COARSE_EPS) & (load <= (K_EPSILON - eps) * E)
        coarse = np.where(tried, load / (K_EPSILON - eps) + slack, np.nan)
        delta = load / g + slack
    return o, d, lo, hi, fallback, none, delta, finite, coarse


def slab_misses(o, d, lo, hi, delta, segment):
    with np.errstate(all="ignore"):
        tn = np.zeros_like(delta)
        tf = np.full_like(delta, 1.0 if segment else INF)
        miss = np.zeros(delta.shape, bool)
        for c in range(3):
            L, H = lo[c] - delta, hi[c] + delta
            still = d[c] == 0.0
            miss |= still & ((o[c] < L) | (o[c] > H))
            inv = 1.0 / d[c]
            t1, t2 = (L - o[c]) * inv, (H - o[c]) * inv
            lo_t, hi_t = np.where(t1 < t2, t1, t2), np.where(t1 < t2, t2, t1)
            tn = np.where(~still & (lo_t > tn), lo_t, tn)
            tf = np.where(~still & (hi_t < tf), hi_t, tf)
        miss |= tn - tf > SLAB * (np.abs(tn) + np.abs(tf))
    return miss


def kept(o, d, rec, segment):
    """rt_light::cube_kept per ray."""
    o, d, lo, hi, fallback, none, delta, finite, coarse = _terms(o, d, rec, segment)
    early = slab_misses(o, d, lo, hi, coarse, segment)  # (a NaN margin proves nothing)
    fine = slab_misses(o, d, lo, hi, delta, segment)
    return ~finite | (~early & (fallback | (~none & ~fine)))


def in_fallback(o, d, rec, segment=False):
    return _terms(o, d, rec, segment)[4]


def delta_of(o, d, rec, segment=False):
    return _terms(o, d, rec, segment)[6]


def kept_count(scene, accel, rays, segment):
    """rt_accel_kept."""
    o, d, skip = yr.origins(rays), yr.directions(rays), rays["skip"]
    n = np.zeros(rays.shape, np.int32)
    for j in range(len(accel)):
        n += ((skip != j) & kept(o, d, accel[j], segment)).astype(np.int32)
    return n


def cast(scene, accel, rays):
    """rt_cast_rays_accel: (hits, triangles): reflect_ref.walk's loop with
    `mine = own != j and kept`."""
    cubes = np.ascontiguousarray(scene.cube_vertices, F32).reshape(-1, 36, 4)
    centres = np.ascontiguousarray(scene.sphere_origins, F32).reshape(-1, 4)
    radius = np.ascontiguousarray(scene.sphere_radius, F32).reshape(-1)
    p, R, skip = yr.origins(rays), yr.directions(rays), rays["skip"]
    nc = len(cubes)
    best = np.full(rays.shape, K_FAR, F32)
    obj2, tri2 = np.full(rays.shape, -1, np.int32), np.full(rays.shape, -1, np.int32)
    with np.errstate(all="ignore"):
        for j in range(nc):
            mine = (skip != j) & kept(p, R, accel[j], False)
            if not mine.any():
                continue
            for k in range(12):
                ok, sf = rr.tri_sf(p, R, *cubes[j, 3 * k:3 * k + 3])
                take = mine & ok & (sf < best)
                best, obj2, tri2 = (np.where(take, sf, best), np.where(take, j, obj2),
                                    np.where(take, k, tri2))
        for s in range(len(radius)):
            ok, sf, _ = rr.sphere_sf(p, R, centres[s], radius[s])
            take = (skip != nc + s) & ok & (sf < best)
            best, obj2, tri2 = (np.where(take, sf, best), np.where(take, nc + s, obj2),
                                np.where(take, -1, tri2))
    hits = np.empty(rays.shape, hit_dtype())
    hits["t"], hits["object"] = best.astype(F32), obj2
    return hits, tri2.astype(np.int32)


def occlude(scene, accel, rays):
    """rt_occlude_rays_accel: uint8 per ray."""
    cubes = np.ascontiguousarray(scene.cube_vertices, F32).reshape(-1, 36, 4)
    centres = np.ascontiguousarray(scene.sphere_origins, F32).reshape(-1, 4)
    radius = np.ascontiguousarray(scene.sphere_radius, F32).reshape(-1)
    p, L, skip = yr.origins(rays), yr.directions(rays), rays["skip"]
    occ = np.zeros(rays.shape, bool)
    for j in range(len(cubes)):
        mine = (skip != j) & kept(p, L, accel[j], True)
        if not mine.any():
            continue
        for k in range(12):
            occ |= mine & sr.tri_occludes(p, L, *cubes[j, 3 * k:3 * k + 3])
    for s in range(len(radius)):
        occ |= (skip != len(cubes) + s) & sr.sphere_occludes(p, L, centres[s], radius[s])
    return occ.astype(np.uint8)


def accepted(verts, rays, segment):
    """Does the exact test accept any of the 12 triangles of one cube (36 x 4
    vertices) per ray: td > 0, or 0 < td < 1."""
    p, R = yr.origins(rays), yr.directions(rays)
    yes = np.zeros(rays.shape, bool)
    for k in range(12):
        ok, td = sr.tri_td(p, R, *verts[3 * k:3 * k + 3])
        with np.errstate(all="ignore"):
            yes |= ok & (td > 0.0) & ((td < 1.0) if segment else True)
    return yes


def ref_line_hits_box(o, d, lo, hi, inflate, tmin, tmax):
    """Does the point set {o + t d : tmin <= t <= tmax} meet the box [lo, hi]
    grown by `inflate` on every side?  Plain float64 parametric clipping
    (Liang-Barsky), per ray; o, d: (n, 3) arrays; lo, hi: 3-vectors."""
    o, d = np.asarray(o, F64), np.asarray(d, F64)
    lo, hi = np.asarray(lo, F64) - inflate, np.asarray(hi, F64) + inflate
    t0 = np.full(len(o), float(tmin))
    t1 = np.full(len(o), float(tmax))
    inside = np.ones(len(o), bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            for p, q in ((-d[:, a], o[:, a] - lo[a]), (d[:, a], hi[a] - o[:, a])):
                # p t <= q
                r = q / p
                inside &= ~((p == 0) & (q < 0))
                t0 = np.where((p < 0) & (r > t0), r, t0)
                t1 = np.where((p > 0) & (r < t1), r, t1)
    return inside & (t0 <= t1)
