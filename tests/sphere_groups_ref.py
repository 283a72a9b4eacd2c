"""The ray queries culled by grouped sphere bounds -- TEST INFRASTRUCTURE ONLY.

A numpy restatement of DESIGN.md §3.1j / §4 for rt_sphere_groups_build /
rt_sphere_groups_kept / rt_cast_rays_grouped / rt_occlude_rays_grouped: the key,
the order and the record of a group (one ufunc per written operation of
include/rt_sphere_groups_impl.h, float32 / float64 where the text is float /
double, in the written order; numpy never contracts), the keep test, and the
grouped walks as thin layers over `accel_ref` (the cube phase and its slab test)
and `reflect_ref.sphere_sf` / `shadow_ref.sphere_occludes`, as they are.

`line_hits_box` is a deliberately independent yardstick in plain float64
(parametric clipping of the whole line, not the keep test's slabs).
"""
import numpy as np

import accel_ref as ar
import rays_ref as yr
import reflect_ref as rr
import shadow_ref as sr
from gpu_support import F32
from hit_ref import hit_dtype

F64 = np.float64
INF = np.inf
C = 2.0 ** -9          # kGroupC
SMALL = 2.0 ** -29     # kGroupSmall
BIG = 2.0 ** 62        # kGroupBig
KEY_LAST = np.uint32(0x7FFFFFFF)


def group_dtype():
    return np.dtype([("lo", "<f4", (3,)), ("rmax", "<f4"), ("hi", "<f4", (3,)),
                     ("count", "<i4"), ("member", "<i4", (8,))])


def count(num_spheres, group_size):
    return -(-num_spheres // group_size)


def float_floor(x):
    """double -> float, to nearest, then one step down where that is above."""
    with np.errstate(all="ignore"):
        f = np.asarray(x, F64).astype(F32)
        high = f.astype(F64) > x
        return np.where(high, np.nextafter(f, F32(-INF)), f).astype(F32)


def float_ceil(x):
    return -float_floor(-np.asarray(x, F64))


def spread3(v):
    v = v.astype(np.uint32)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def keys(centres, radius):
    """sphere_key per sphere: (keys, finite)."""
    c = np.ascontiguousarray(centres, F32).reshape(-1, 4)[:, :3]
    r = np.ascontiguousarray(radius, F32).reshape(-1)
    finite = np.isfinite(c).all(1) & np.isfinite(r)
    key = np.full(len(r), KEY_LAST, np.uint32)
    if not finite.any():
        return key, finite
    with np.errstate(all="ignore"):
        mn, mx = c[finite].min(0), c[finite].max(0)
        ext = F32(max(F32(0.0), *(mx - mn)))   # fp32 subtractions, the largest of three
        cells = []
        for a in range(3):
            if ext > 0:
                s = ((c[:, a] - mn[a]) / ext) * F32(1023.0)
                inside = np.where((s >= 0) & (s < 1023.0), s, F32(0.0))  # (NaN: cell 0)
                cell = np.where(s >= 1023.0, 1023, np.trunc(inside)).astype(np.uint32)
            else:
                cell = np.zeros(len(r), np.uint32)
            cells.append(spread3(cell))
    morton = cells[0] | (cells[1] << np.uint32(1)) | (cells[2] << np.uint32(2))
    return np.where(finite, morton, KEY_LAST).astype(np.uint32), finite


def order(centres, radius):
    key, _ = keys(centres, radius)
    return np.lexsort((np.arange(len(key)), key)).astype(np.int32)  # by (key, index)


def records(centres, radius, group_size):
    """rt_sphere_groups_build."""
    c = np.ascontiguousarray(centres, F32).reshape(-1, 4)[:, :3]
    r = np.ascontiguousarray(radius, F32).reshape(-1)
    n = len(r)
    out = np.zeros(count(n, group_size), group_dtype())
    if not n:
        return out
    _, finite = keys(c2 := np.concatenate([c, np.zeros((n, 1), F32)], 1), r)
    srt = order(c2, r)
    with np.errstate(all="ignore"):
        ar_ = np.abs(r)
        lo = float_floor(c.astype(F64) - ar_.astype(F64)[:, None])
        hi = float_ceil(c.astype(F64) + ar_.astype(F64)[:, None])
    for g in range(len(out)):
        m = np.sort(srt[g * group_size:(g + 1) * group_size])
        out["count"][g] = len(m)
        out["member"][g] = -1
        out["member"][g, :len(m)] = m
        if finite[m].all():
            out["lo"][g] = lo[m].min(0) + F32(0.0)
            out["hi"][g] = hi[m].max(0) + F32(0.0)
            out["rmax"][g] = ar_[m].max()
        else:
            out["lo"][g], out["hi"][g], out["rmax"][g] = -INF, INF, INF
    return out


def line_slab_misses(o, d, lo, hi, delta):
    """The overload of slab_misses over the whole line (-inf, +inf)."""
    with np.errstate(all="ignore"):
        tn = np.full_like(delta, -INF)
        tf = np.full_like(delta, INF)
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
        miss |= tn - tf > ar.SLAB * (np.abs(tn) + np.abs(tf))
    return miss


def terms(o, d, rec):
    """(o, d as float64 lists, lo, hi, fallback, M) of group_kept."""
    o = [np.asarray(a, F32).astype(F64) for a in o]
    d = [np.asarray(a, F32).astype(F64) for a in d]
    lo, hi = rec["lo"].astype(F64), rec["hi"].astype(F64)
    with np.errstate(all="ignore"):
        D1 = (np.abs(d[0]) + np.abs(d[1])) + np.abs(d[2])
        O1 = (np.abs(o[0]) + np.abs(o[1])) + np.abs(o[2])
        T1 = np.zeros_like(D1)
        for c in range(3):
            a, h = np.abs(o[c] - lo[c]), np.abs(o[c] - hi[c])
            T1 = T1 + np.where(a > h, a, h)
        M = T1 + F64(rec["rmax"])
        margin = C * M
        fallback = (~(D1 >= SMALL) | ~(D1 < BIG) | ~(O1 < INF) | ~(M < BIG) | ~(D1 * M < BIG) |
                    ~(margin >= SMALL))
    return o, d, lo, hi, fallback, M, O1


def kept(o, d, rec, segment=False, c=C):
    """rt_light::group_kept per ray (`c`: the margin's constant; 0 for the
    test that shows the margin is needed)."""
    o, d, lo, hi, fallback, M, O1 = terms(o, d, rec)
    with np.errstate(all="ignore"):
        delta = c * M + (ar.K2 * (M + O1) if c else 0.0)
    return fallback | ~line_slab_misses(o, d, lo, hi, delta)


def in_fallback(o, d, rec):
    return terms(o, d, rec)[4]


def kept_count(groups, rays, segment=False):
    """rt_sphere_groups_kept."""
    o, d = yr.origins(rays), yr.directions(rays)
    n = np.zeros(rays.shape, np.int32)
    for rec in groups:
        n += kept(o, d, rec, segment).astype(np.int32)
    return n


def cast(scene, accel, groups, rays):
    """rt_cast_rays_grouped: accel_ref.cast's cube phase, then the groups."""
    spheres_off = type("S", (), dict(cube_vertices=scene.cube_vertices,
                                     sphere_origins=np.zeros((0, 4), F32),
                                     sphere_radius=np.zeros(0, F32)))
    hits, tri2 = ar.cast(spheres_off, accel, rays)
    centres = np.ascontiguousarray(scene.sphere_origins, F32).reshape(-1, 4)
    radius = np.ascontiguousarray(scene.sphere_radius, F32).reshape(-1)
    p, R, skip = yr.origins(rays), yr.directions(rays), rays["skip"]
    nc = len(accel)
    best, obj2 = hits["t"].copy(), hits["object"].copy()
    with np.errstate(all="ignore"):
        for rec in groups:
            mine = kept(p, R, rec, False)
            if not mine.any():
                continue
            for s in rec["member"][:rec["count"]]:
                ok, sf, _ = rr.sphere_sf(p, R, centres[s], radius[s])
                closer = (sf < best) | ((sf == best) & (obj2 >= nc) & (obj2 > nc + s))
                take = mine & (skip != nc + s) & ok & closer
                best, obj2, tri2 = (np.where(take, sf, best), np.where(take, nc + s, obj2),
                                    np.where(take, -1, tri2))
    out = np.empty(rays.shape, hit_dtype())
    out["t"], out["object"] = best.astype(F32), obj2
    return out, tri2.astype(np.int32)


def occlude(scene, accel, groups, rays):
    """rt_occlude_rays_grouped: uint8 per ray."""
    spheres_off = type("S", (), dict(cube_vertices=scene.cube_vertices,
                                     sphere_origins=np.zeros((0, 4), F32),
                                     sphere_radius=np.zeros(0, F32)))
    occ = ar.occlude(spheres_off, accel, rays).astype(bool)
    centres = np.ascontiguousarray(scene.sphere_origins, F32).reshape(-1, 4)
    radius = np.ascontiguousarray(scene.sphere_radius, F32).reshape(-1)
    p, L, skip = yr.origins(rays), yr.directions(rays), rays["skip"]
    nc = len(accel)
    for rec in groups:
        mine = kept(p, L, rec, True)
        for s in rec["member"][:rec["count"]]:
            occ |= mine & (skip != nc + s) & sr.sphere_occludes(p, L, centres[s], radius[s])
    return occ.astype(np.uint8)


def accepted(centre, r, rays, segment):
    """Does the exact fp32 test accept the sphere per ray: bounce_sphere, or
    occluded_by_sphere."""
    p, R = yr.origins(rays), yr.directions(rays)
    if segment:
        return sr.sphere_occludes(p, R, centre, r)
    return rr.sphere_sf(p, R, centre, r)[0]


def line_hits_box(o, d, lo, hi, inflate):
    """Does the whole line {o + t d} meet the box [lo, hi] grown by `inflate`
    (one value per ray) on every side?  Plain float64 parametric clipping
    (Liang-Barsky over an unbounded range), per ray; o, d: (n, 3) arrays."""
    o, d = np.asarray(o, F64), np.asarray(d, F64)
    grow = np.asarray(inflate, F64).reshape(-1, 1)
    lo, hi = np.asarray(lo, F64) - grow, np.asarray(hi, F64) + grow
    t0, t1 = np.full(len(o), -INF), np.full(len(o), INF)
    inside = np.ones(len(o), bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            for p, q in ((-d[:, a], o[:, a] - lo[:, a]), (d[:, a], hi[:, a] - o[:, a])):
                r = q / p  # p t <= q
                inside &= ~((p == 0) & (q < 0))
                t0 = np.where((p < 0) & (r > t0), r, t0)
                t1 = np.where((p > 0) & (r < t1), r, t1)
    return inside & (t0 <= t1)
