"""Exact geometry for the ray queries and the surfaces -- TEST INFRASTRUCTURE ONLY.

Not a restatement: nothing here follows the operation order of
include/rt_light_impl.h, and nothing is imported from the `*_ref.py`
restatements.  The float32 inputs are taken as exact reals.

Triangles: exact rational arithmetic.  Every float is a dyadic rational, so the
coordinates of one ray and one triangle are brought to a common power-of-two
denominator and `det`, and the numerators of `u`, `v`, `t`, are computed in
Python integers; the quotients are `fractions.Fraction`s.  A pair is a *clear
candidate*, a *clear non-candidate*, or *borderline*: within a relative 2^-40
of one of the library's thresholds (|det| = 1e-6, u = 0, v = 0, u + v = 1,
t = 0, t = 1 for segments, and t = 300000, the miss value a candidate has to
beat).  "Relative" is to the size of the sum the fp64 code under test rounds:
the same expression with every term's absolute value (`M*` below), since at a
threshold of 0 the quantity itself is no scale.

Spheres: long double on the floats (products of two floats are exact in
float64 already).  The discriminant D = B^2 - A*Q is classified by D > +E,
D < -E or borderline, E = 32u*S, S = A(|m|^2 + r^2), u = 2^-24;
the roots against 0, 1 and 300000 with the tolerance of t ("the
tolerance of t"), which `sphere_pairs` and `tri_pair` compute per pair.

Closest hit: the first minimum over clear candidates.  A ray is *decided*
when its nearest clear candidate beats every other clear or borderline
candidate by more than the sum of their tolerances and no borderline candidate
could be nearer.  Candidates on bit-identical primitives (the twin cubes, two
equal spheres) tie exactly, in the library too since equal inputs give equal
words: the documented rule decides them, cubes before spheres, lower slot
first.
"""
from fractions import Fraction

import numpy as np

U32 = 2.0 ** -24           # the unit roundoff of float32
ETA = 2.0 ** -53           # of float64
REL = 2.0 ** -40           # the borderline band of the triangle thresholds
K_FAR = 300000.0
EPSILON = Fraction(0.000001)  # the library's double constant, exactly
NON, CLEAR, BORDER = 0, 1, 2
LD = np.longdouble


# ---------------------------------------------------------------------------
# Scenes and rays as plain arrays
# ---------------------------------------------------------------------------
class Geometry:
    """The arrays of a scene: cubes (nc, 12, 3, 3) float32 triangles, centres
    (ns, 3), radius (ns,); slots are cubes 0 .. nc-1, then spheres."""

    def __init__(self, scene):
        cv = np.ascontiguousarray(scene.cube_vertices, np.float32).reshape(-1, 36, 4)
        self.tris = cv[:, :, :3].reshape(-1, 12, 3, 3)
        self.centres = np.ascontiguousarray(scene.sphere_origins, np.float32).reshape(-1, 4)[:, :3]
        self.radius = np.ascontiguousarray(scene.sphere_radius, np.float32).reshape(-1)
        self.nc, self.ns = len(self.tris), len(self.radius)
        # bit-identical primitives share a key: they tie exactly
        self.tri_key = [[self.tris[j, k].tobytes() for k in range(12)] for j in range(self.nc)]
        self.sphere_key = [self.centres[i].tobytes() + self.radius[i].tobytes()
                           for i in range(self.ns)]


def ray_arrays(rays):
    """(origins (n, 3), directions (n, 3), skip (n,)) of a flat RAY_DTYPE array."""
    rays = np.asarray(rays).reshape(-1)
    o = np.stack([rays[f] for f in ("ox", "oy", "oz")], -1)
    d = np.stack([rays[f] for f in ("dx", "dy", "dz")], -1)
    return o, d, rays["skip"].astype(np.int64)


# ---------------------------------------------------------------------------
# Triangles, exactly
# ---------------------------------------------------------------------------
def _ints(values):
    """Floats as integers over a common denominator 2^k: (ints, k)."""
    ratios = [float(v).as_integer_ratio() for v in values]
    k = max(den.bit_length() - 1 for _, den in ratios)
    return [num << (k - (den.bit_length() - 1)) for num, den in ratios], k


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _abs_cross(a, b):
    return (abs(a[1] * b[2]) + abs(a[2] * b[1]), abs(a[2] * b[0]) + abs(a[0] * b[2]),
            abs(a[0] * b[1]) + abs(a[1] * b[0]))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _abs_dot(a, b):
    return abs(a[0]) * b[0] + abs(a[1]) * b[1] + abs(a[2]) * b[2]


class TriPair:
    """One ray against one triangle: the exact det, u, v, t (Fractions; u, v,
    t None where det == 0), the class as a cast candidate (t in (0, 300000))
    and as an occluder (t in (0, 1)), t as a float and its tolerance."""
    __slots__ = ("det", "u", "v", "t", "cast", "segment", "tf", "tol")


def tri_pair(o, d, v0, v1, v2):
    return _tri_pair(_ints(o), _ints(d), _ints([*v0, *v1, *v2]))


def _tri_pair(origin, direction, triangle):
    """tri_pair on (ints, k) triples: the origin's and the triangle's are
    brought to one denominator here."""
    (O, k0), (D, kd), (T, k1) = origin, direction, triangle
    ko = max(k0, k1)
    O, T = [x << (ko - k0) for x in O], [x << (ko - k1) for x in T]
    A, B, C = T[0:3], T[3:6], T[6:9]
    e1 = tuple(B[i] - A[i] for i in range(3))
    e2 = tuple(C[i] - A[i] for i in range(3))
    tv = tuple(O[i] - A[i] for i in range(3))
    pv, qv = _cross(D, e2), _cross(tv, e1)
    det, un, vn, tn = _dot(e1, pv), _dot(tv, pv), _dot(D, qv), _dot(e2, qv)
    scale = 1 << (2 * ko + kd)          # of det, un, vn; tn is over 2^(3 ko)
    r = TriPair()
    r.det = Fraction(det, scale)
    r.u = r.v = r.t = None
    r.tf, r.tol = float("nan"), 0.0
    if det == 0:
        r.cast = r.segment = NON
        return r
    r.u, r.v, r.t = Fraction(un, det), Fraction(vn, det), Fraction(tn << kd, det << ko)
    # the sums the fp64 code rounds, with absolute values term by term
    adet = abs(det)
    m_det = _abs_dot(e1, _abs_cross(D, e2)) / adet
    m_u = _abs_dot(tv, _abs_cross(D, e2)) / adet
    m_v = _abs_dot(D, _abs_cross(tv, e1)) / adet
    m_t = (_abs_dot(e2, _abs_cross(tv, e1)) << kd) / (adet << ko)
    u, v, t = float(r.u), float(r.v), float(r.t)
    r.tf = t
    # (float)td: one rounding to float32, and the fp64 numerator and det bounds
    r.tol = U32 * abs(t) + 16 * ETA * (m_t + abs(t) * m_det)
    band_u = REL * (1 + m_u + abs(u) * m_det)
    band_v = REL * (1 + m_v + abs(v) * m_det)
    band_t = REL * (m_t + abs(t) * m_det)
    band_det = REL * (1 + m_det)          # relative to |det| itself
    eps = float(EPSILON * scale / adet)   # the threshold in units of |det|
    non = eps > 1 + band_det or u < -band_u or v < -band_v or u + v > 1 + band_u + band_v
    border = (eps > 1 - band_det or u < band_u or v < band_v or u + v > 1 - band_u - band_v)
    if non:
        r.cast = r.segment = NON
        return r
    far_band = REL * K_FAR + band_t + r.tol
    if t < -band_t or t > K_FAR + far_band:
        r.cast = NON
    else:
        r.cast = BORDER if border or t < band_t or t > K_FAR - far_band else CLEAR
    if t < -band_t or t > 1 + REL + band_t:
        r.segment = NON
    else:
        r.segment = BORDER if border or t < band_t or t > 1 - REL - band_t else CLEAR
    return r


def tri_normal(v0, v1, v2):
    """The exact unit normal (e1 x e2 rounded once to float64, then scaled),
    and sin of the angle between the edges."""
    pts, _ = _ints([*v0, *v1, *v2])
    e1 = tuple(pts[3 + i] - pts[i] for i in range(3))
    e2 = tuple(pts[6 + i] - pts[i] for i in range(3))
    n = _cross(e1, e2)
    nn, l1, l2 = _dot(n, n), _dot(e1, e1), _dot(e2, e2)
    if nn == 0:
        return np.zeros(3), 0.0
    big = max(abs(c) for c in n)
    unit = np.array([c / big for c in n])
    return unit / np.linalg.norm(unit), float(Fraction(nn, l1 * l2)) ** 0.5


# ---------------------------------------------------------------------------
# Spheres, in long double
# ---------------------------------------------------------------------------
class SpherePairs:
    """n rays against one sphere.  A, B, Q, S, disc (= B^2 - A*Q), E, the
    roots s0 <= s1 and their tolerances (NaN where disc < 0); `cast`,
    `segment`: the classes; `t`, `tol`: the candidate's parameter (for a
    borderline one a lower bound of it) and tolerance; `far`: the far root."""


def sphere_pairs(o, d, centre, r):
    o, d = np.asarray(o, LD), np.asarray(d, LD)
    m = np.asarray(centre, LD)[None, :] - o
    rr = LD(r) * LD(r)
    p = SpherePairs()
    with np.errstate(all="ignore"):
        A, B, mm = (d * d).sum(-1), (m * d).sum(-1), (m * m).sum(-1)
        Q, S = mm - rr, A * (mm + rr)
        disc, E = B * B - A * Q, 32 * LD(U32) * S
        sq = np.sqrt(np.maximum(disc, 0))
        big = np.where(B >= 0, B + sq, B - sq)       # the root numerator without cancellation
        other = np.where(big != 0, Q / np.where(big != 0, big, 1), 0)
        s0 = np.where(B >= 0, other, big / A)
        s1 = np.where(B >= 0, big / A, other)
        # the tolerance of a root: the error of b, the band through
        # the square root, the subtraction and the division
        e_b = 4.1 * U32 * np.sqrt(mm * A)
        e_sq = E / (np.sqrt(np.maximum(disc - E, 0)) + sq) + 1.12 * U32 * np.sqrt(np.abs(disc) + E)
        base = (1 + 5 * U32) * (e_b + e_sq) / A
        tol0, tol1 = base + 6 * U32 * np.abs(s0), base + 6 * U32 * np.abs(s1)
        hit, miss = disc > E, disc < -E
        # the range the roots of a borderline discriminant can lie in
        spread = np.sqrt(np.maximum(disc, 0) + E)
        slack = (1 + 5 * U32) * (e_b + np.sqrt(E) + 1.12 * U32 * spread) / A
        lo = (B - spread) / A - slack - 6 * U32 * np.abs((B - spread) / A)
        hi = (B + spread) / A + slack + 6 * U32 * np.abs((B + spread) / A)
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    p.A, p.B, p.Q, p.S, p.disc, p.E = f(A), f(B), f(Q), f(S), f(disc), f(E)
    p.s0, p.s1 = f(np.where(disc >= 0, s0, np.nan)), f(np.where(disc >= 0, s1, np.nan))
    p.tol0, p.tol1 = f(tol0), f(tol1)
    n = len(o)
    cast, t, tol = np.full(n, BORDER, np.int8), f(np.maximum(lo, 0)), f(tol0 + tol1)
    far = np.zeros(n, bool)
    near_ok, near_behind = hit & (s0 > tol0), hit & (s0 < -tol0)
    far_ok, far_behind = near_behind & (s1 > tol1), near_behind & (s1 < -tol1)
    cast[near_ok], cast[far_ok] = CLEAR, CLEAR
    t[near_ok], tol[near_ok] = f(s0)[near_ok], f(tol0)[near_ok]
    t[far_ok], tol[far_ok], far[far_ok] = f(s1)[far_ok], f(tol1)[far_ok], True
    cast[miss | far_behind | (~hit & ~miss & (hi < 0))] = NON
    # against 300000, the value a candidate has to beat
    clear = cast == CLEAR
    cast[clear & (t > K_FAR + tol)] = NON
    cast[clear & (np.abs(t - K_FAR) <= tol)] = BORDER
    cast[(cast == BORDER) & (t > K_FAR + tol)] = NON
    p.cast, p.t, p.tol, p.far = cast, t, tol, far
    # a segment: any root strictly inside (0, 1)
    inside0 = hit & (s0 > tol0) & (s0 < 1 - tol0)
    inside1 = hit & (s1 > tol1) & (s1 < 1 - tol1)
    out0 = (s0 < -tol0) | (s0 > 1 + tol0)
    out1 = (s1 < -tol1) | (s1 > 1 + tol1)
    seg = np.full(n, BORDER, np.int8)
    seg[inside0 | inside1] = CLEAR
    seg[miss | (hit & out0 & out1) | (~hit & ~miss & ((hi < 0) | (lo > 1)))] = NON
    p.segment = seg
    return p


# ---------------------------------------------------------------------------
# Closest hits and occlusion of a ray set
# ---------------------------------------------------------------------------
DECIDED_HIT, DECIDED_MISS, UNDECIDED = 0, 1, 2


class Pairs:
    """Every ray of a set against every primitive of a scene, without regard
    to `skip`: tri[i][j][k] a TriPair, spheres[s] a SpherePairs."""

    def __init__(self, geometry, rays):
        self.g = geometry
        self.o, self.d, self.skip = ray_arrays(rays)
        self.n = len(self.o)
        g = geometry
        tris = [[_ints(g.tris[j, k].reshape(-1)) for k in range(12)] for j in range(g.nc)]
        self.tri = []
        for i in range(self.n):
            origin, direction = _ints(self.o[i]), _ints(self.d[i])
            self.tri.append([[_tri_pair(origin, direction, tris[j][k]) for k in range(12)]
                             for j in range(g.nc)])
        self.spheres = [sphere_pairs(self.o, self.d, g.centres[s], g.radius[s])
                        for s in range(g.ns)]


class Closest:
    """Per ray: status, and for a decided hit the object, t, its tolerance and
    the triangles that may be named; for every ray `tri_ok`: the triangles of
    each cube that are clear or borderline candidates, with their t."""


def closest(pairs, skip=None):
    g, n = pairs.g, pairs.n
    skip = pairs.skip if skip is None else np.broadcast_to(np.asarray(skip), (n,))
    c = Closest()
    c.status = np.full(n, UNDECIDED, np.int8)
    c.obj, c.t, c.tol = np.full(n, -1, np.int64), np.full(n, K_FAR), np.zeros(n)
    c.far = np.zeros(n, bool)
    c.tris = [dict() for _ in range(n)]   # cube -> [(k, t, tol)] clear or borderline
    for i in range(n):
        cands = []  # (t or its lower bound, tol, slot, class, key, far)
        for j in range(g.nc):
            if j == skip[i]:
                continue
            for k in range(12):
                tp = pairs.tri[i][j][k]
                if tp.cast != NON:
                    cands.append((tp.tf, tp.tol, j, tp.cast, g.tri_key[j][k], False))
                    c.tris[i].setdefault(j, []).append((k, tp.tf, tp.tol))
        for s in range(g.ns):
            if g.nc + s == skip[i]:
                continue
            sp = pairs.spheres[s]
            if sp.cast[i] != NON:
                cands.append((sp.t[i], sp.tol[i], g.nc + s, sp.cast[i], g.sphere_key[s],
                              bool(sp.far[i])))
        clear = [x for x in cands if x[3] == CLEAR]
        if not cands:
            c.status[i] = DECIDED_MISS
            continue
        if not clear:
            continue
        best = min(clear, key=lambda x: (x[0], x[2]))
        decided, winner = True, best[2]
        for x in cands:
            if x is best:
                continue
            if x[4] == best[4] and x[3] == CLEAR:  # the same primitive again: an exact tie
                winner = min(winner, x[2])
                continue
            # another triangle of the same cube at the same t: the same hit
            if x[2] == best[2] and x[2] < g.nc and abs(x[0] - best[0]) <= x[1] + best[1]:
                continue
            if not x[0] - best[0] > x[1] + best[1]:
                decided = False
                break
        if decided:
            c.status[i], c.obj[i], c.t[i], c.tol[i], c.far[i] = DECIDED_HIT, winner, best[0], \
                best[1], best[5]
    return c


class Occlusion:
    """Per segment: status (DECIDED_HIT = occluded, DECIDED_MISS = free), and
    the kind of a clear occluder ("cube", "sphere")."""


def occlusion(pairs, skip=None):
    g, n = pairs.g, pairs.n
    skip = pairs.skip if skip is None else np.broadcast_to(np.asarray(skip), (n,))
    clear_cube, border = np.zeros(n, bool), np.zeros(n, bool)
    for i in range(n):
        for j in range(g.nc):
            if j == skip[i]:
                continue
            for k in range(12):
                cls = pairs.tri[i][j][k].segment
                clear_cube[i] |= cls == CLEAR
                border[i] |= cls == BORDER
    clear_sphere = np.zeros(n, bool)
    for s in range(g.ns):
        on = skip != g.nc + s
        clear_sphere |= on & (pairs.spheres[s].segment == CLEAR)
        border |= on & (pairs.spheres[s].segment == BORDER)
    r = Occlusion()
    r.by_cube, r.by_sphere = clear_cube, clear_sphere
    r.status = np.where(clear_cube | clear_sphere, DECIDED_HIT,
                        np.where(border, UNDECIDED, DECIDED_MISS)).astype(np.int8)
    return r


# ---------------------------------------------------------------------------
# Judging an answer by its meaning
# ---------------------------------------------------------------------------
def judge_cast(pairs, ref, t, obj, tri=None, limit=5, count=None):
    """The violations (strings; at most `limit`) of a cast's answer against
    `ref` = closest(pairs): on a decided hit the object, t within tolerance and
    a triangle that is a candidate at that t; on a decided miss (300000, -1);
    on every ray no NaN and no id outside the scene.  `count`: judge the first
    `count` rays only."""
    g, bad = pairs.g, []
    t, obj = np.asarray(t, np.float64), np.asarray(obj)
    for i in range(pairs.n if count is None else count):
        why = None
        if np.isnan(t[i]) or not -1 <= obj[i] < g.nc + g.ns:
            why = "NaN or a foreign id"
        elif tri is not None and not (-1 <= tri[i] < 12 and (tri[i] >= 0) == (0 <= obj[i] < g.nc)):
            why = f"triangle {tri[i]} for object {obj[i]}"
        elif ref.status[i] == DECIDED_MISS:
            if obj[i] != -1 or t[i] != K_FAR:
                why = "a clear miss"
        elif ref.status[i] == DECIDED_HIT:
            if obj[i] != ref.obj[i]:
                why = f"object {ref.obj[i]} at {ref.t[i]!r}"
            elif not abs(t[i] - ref.t[i]) <= ref.tol[i]:
                why = f"t {ref.t[i]!r} +- {ref.tol[i]:.3g}"
            elif tri is not None and obj[i] < g.nc:
                near = [k for k, tk, tolk in ref.tris[i].get(int(obj[i]), ())
                        if abs(tk - ref.t[i]) <= tolk + ref.tol[i]]
                if tri[i] not in near:
                    why = f"one of the triangles {near}"
        if why:
            bad.append(f"ray {i}: got ({t[i]!r}, {obj[i]}"
                       f"{'' if tri is None else ', ' + str(tri[i])}), exact: {why}")
            if len(bad) >= limit:
                break
    return bad


def judge_occlude(ref, flags, limit=5):
    flags = np.asarray(flags)
    wrong = ((ref.status == DECIDED_HIT) & (flags != 1)) | \
        ((ref.status == DECIDED_MISS) & (flags != 0)) | ~np.isin(flags, (0, 1))
    return [f"segment {i}: got {flags[i]}, exact: "
            f"{'occluded' if ref.status[i] == DECIDED_HIT else 'free'}"
            for i in np.nonzero(wrong)[0][:limit]]


def t_errors(ref, t):
    """(the worst |t - exact| / |exact| over the decided hits, the worst
    |t - exact| / tolerance)."""
    on = ref.status == DECIDED_HIT
    if not on.any():
        return 0.0, 0.0
    err = np.abs(np.asarray(t, np.float64)[on] - ref.t[on])
    return float((err / np.abs(ref.t[on])).max()), float((err / ref.tol[on]).max())


# ---------------------------------------------------------------------------
# Surfaces
# ---------------------------------------------------------------------------
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def sphere_normal(point, centre):
    """(p - c) / |p - c|."""
    return unit(np.asarray(point, np.float64) - np.asarray(centre, np.float64))


def faced(n, d):
    """n turned against d, and the cosine between them before the turn."""
    n, d = np.asarray(n, np.float64), np.asarray(d, np.float64)
    c = (n * d).sum(-1) / np.linalg.norm(d, axis=-1)
    return np.where((c > 0)[..., None], -n, n), c


def mirror(n, d):
    """d mirrored at the unit normal n: d - 2 (n . d) n."""
    n, d = np.asarray(n, np.float64), np.asarray(d, np.float64)
    return d - 2 * (n * d).sum(-1, keepdims=True) * n


def angle(a, b):
    """The angle between unit vectors, accurate near 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 2 * np.arcsin(np.minimum(np.linalg.norm(a - b, axis=-1) / 2, 1.0))
