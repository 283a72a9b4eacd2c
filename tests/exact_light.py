"""Exact light and colour for the lit frames -- TEST INFRASTRUCTURE ONLY.

Not a restatement: nothing here follows the operation order of
include/rt_light_impl.h and nothing is imported from the `*_ref.py`
restatements.  It states what DESIGN.md §3.1a-e and §3.1i mean (Lambert light
summed over the lights and clamped at 1, a depth ramp, a mirror blend run
backwards over the levels of a chain) in float64 on top of `exact_ref`, and
gives per channel a value `v` and a bound `d` of what the float32 library may
differ from it by.  A channel's admissible integers are trunc(v - d) ..
trunc(v + d), since the library truncates.

A quantity is a pair (v, d) of float64 arrays.  Every float32 operation of the
library on such a quantity is one call of `rounded`: it adds u * (|v| + d),
u = 2^-24, to d.  The operation counts behind each bound are derived in
DESIGN.md §5 ("the bound of a lit channel"); none of them was tuned on the
library's output.

A *level* is one point of a pixel's chain: the object, the float32 point `p`
(taken as an exact real: it is recomputed from the library's own, judged `t` by
the documented two-operation formula), the exact faced unit normal `n` with
its angle bound, the accumulated depth `T`, and per light the verdict of
`exact_ref.occlusion` on the segment p -> light with the level's object left
out.
"""
from types import SimpleNamespace

import numpy as np

import exact_ref as ex

U = ex.U32
# The float32 cosine n.L / |L| against the real one, beyond the normal's angle
# bound, in units of u: the three subtractions of L (1 on the dot product, 1 on
# the length), the dot product (3 products and 2 sums: 3), the length (3
# products, 2 sums, halved by the root, and the root: 2.5), the division (1),
# and the library's normal not being exactly of length 1 (a root of a sum of
# squares and a division per component: 3.5).
COS_ROUNDING = 12 * U
FREE, HIDDEN, OPEN = ex.DECIDED_MISS, ex.DECIDED_HIT, ex.UNDECIDED
MAX_DELTA = 0.01
MIN_SHARP = 0.95


def rounded(v, d):
    """The bound after one more float32 rounding of v +- d."""
    return d + U * (np.abs(v) + d)


def times(a, b):
    """One float32 product of two quantities."""
    (va, da), (vb, db) = a, b
    v = va * vb
    return v, rounded(v, np.abs(va) * db + np.abs(vb) * da + da * db)


def between(q, lo=None, hi=None):
    """A quantity clamped into [lo, hi]: what its ends become."""
    a, b = q[0] - q[1], q[0] + q[1]
    if lo is not None:
        a, b = np.maximum(a, lo), np.maximum(b, lo)
    if hi is not None:
        a, b = np.minimum(a, hi), np.minimum(b, hi)
    return (a + b) / 2, (b - a) / 2


# ---------------------------------------------------------------------------
# One level
# ---------------------------------------------------------------------------
def cosines(n, p, lights):
    """cos_i = n . (l_i - p) / |l_i - p|: (lights, points)."""
    L = np.asarray(lights, np.float64)[:, None, :3] - np.asarray(p, np.float64)[None, :, :]
    return (L * n[None]).sum(-1) / np.linalg.norm(L, axis=-1)


def factor(cos, bound, free=None):
    """k = min(1, sum of the positive cosines) as a quantity, over the lights
    (axis 0).  `bound` (points,): each cosine's rounding bound.  A cosine at or
    below its bound is not decided either way: it adds only to the bound.
    `free` (lights, points) of FREE / HIDDEN / OPEN: with shadows, a facing
    light counts where its segment is FREE; OPEN segments of facing lights are
    reported in the third result (the pixel cannot be judged).  Returns
    (k, the unclamped sum, open)."""
    facing = cos > bound[None]
    vague = np.abs(cos) <= bound[None]
    counts = facing if free is None else facing & (free == FREE)
    undecided = np.zeros(cos.shape[1], bool) if free is None else (facing & (free == OPEN)).any(0)
    total = np.where(counts, cos, 0.0).sum(0)
    d = (counts * bound[None]).sum(0) + 2 * (vague * bound[None]).sum(0)
    d = d + len(cos) * U * (total + d)  # the float32 sums k = k + c
    return between((total, d), 0.0, 1.0), total, undecided


def ramp(T, clamped):
    """255 - 255 T / 180 as the library's three float32 operations leave it;
    `clamped`: at 0 from below (levels >= 1)."""
    v, d = T
    v, d = v / 180.0, rounded(v / 180.0, d / 180.0)
    v, d = v * 255.0, rounded(v * 255.0, d * 255.0)
    v, d = 255.0 - v, rounded(255.0 - v, d)
    return between((v, d), 0.0) if clamped else (v, d)


def own_colour(T, k, colour, clamped):
    """(ramp * k) * colour per channel: quantities of shape (points, 3)."""
    lit = times(ramp(T, clamped), k)
    lit = lit[0][:, None], lit[1][:, None]
    return times(lit, (np.asarray(colour, np.float64), 0.0))


def blend(a, r, C):
    """a + r (C - a) per channel, r (points,) exact: the value is the convex
    combination, its bound the combination of the bounds plus the three
    float32 roundings (the difference, the product, the sum)."""
    r = np.asarray(r, np.float64)[:, None]
    diff = C[0] - a[0]
    e = U * (np.abs(diff) + C[1] + a[1])
    e = r * e + U * (np.abs(r * diff) + r * (C[1] + a[1] + e))
    v = a[0] + r * diff
    d = (1 - r) * a[1] + r * C[1] + e
    return v, d + U * (np.abs(v) + d)


def chain(steps):
    """The pixels' colours from `steps`, level 0 first: per level (reached
    (points,), goes on (points,), own colour, reflectivity (points,)).  A chain
    that ends at a level has that level's own colour there; black stands
    behind a level whose bounce met nothing; the blend runs backwards."""
    C = None
    for reached, goes, own, r in steps[::-1]:
        if C is None:
            C = (np.zeros_like(own[0]), np.zeros_like(own[1]))
        mixed = blend(own, r, C)
        C = tuple(np.where(goes[:, None], m, np.where(reached[:, None], a, 0.0))
                  for m, a in zip(mixed, own))
    return C


# ---------------------------------------------------------------------------
# A frame's reference and its judge
# ---------------------------------------------------------------------------
def admissible(C):
    """(lowest, highest) admissible integer per channel."""
    return np.trunc(C[0] - C[1]).astype(np.int64), np.trunc(C[0] + C[1]).astype(np.int64)


def reference(n, judged, miss, C, limit=MAX_DELTA):
    """The reference of a frame of `n` pixels: `judged` (n,) the hit pixels it
    states, `miss` (n,) the clear misses, `C` the quantity (n, 3) (anything
    where not judged).  A judged pixel with a channel's bound above `limit` is
    excluded.  `excluded`: the share of the pixels that are neither judged nor
    a miss; `sharp`: the share of the judged channels that admit one integer."""
    wide = (C[1] > limit).any(-1)
    judged = judged & ~wide
    on = judged[:, None]
    lo, hi = admissible((np.where(on, C[0], 0.0), np.where(on, C[1], 0.0)))
    f = SimpleNamespace(n=n, judged=judged, miss=miss, lo=lo, hi=hi, v=C[0], d=C[1])
    f.excluded = float(1 - (judged | miss).mean())
    f.sharp = float((lo == hi)[judged].mean()) if judged.any() else 0.0
    f.delta = float(C[1][judged].max()) if judged.any() else 0.0
    return f


def check_reference(f, cap):
    """The two conditions and the cap, on the reference alone."""
    assert f.excluded <= cap, f.excluded
    assert f.delta <= MAX_DELTA, f.delta
    assert f.sharp >= MIN_SHARP, f.sharp


def rejected(f, frame):
    """The pixels of `frame` ((n, 4) int32, or (n,) uint32 RGBA8) that the
    reference `f` rejects: a channel outside its admissible integers (for RGBA8
    their low bytes), an alpha other than 255, a clear miss that is not
    (0, 0, 0, 255)."""
    frame = np.asarray(frame)
    if frame.ndim == 1:  # RGBA8: bytes, compared modulo 256
        px = np.stack([(frame >> s) & 0xFF for s in (0, 8, 16, 24)], -1).astype(np.int64)
        inside = ((px[:, :3] - f.lo) % 256) <= (f.hi - f.lo)
    else:
        px = frame.astype(np.int64)
        inside = (px[:, :3] >= f.lo) & (px[:, :3] <= f.hi)
    bad = (px[:, 3] != 255) | (f.judged & ~inside.all(-1)) | (f.miss & px[:, :3].any(-1))
    return np.nonzero(bad)[0]


def describe(f, frame, limit=3):
    frame = np.asarray(frame)
    return [f"pixel {i}: got {frame[i]!r}, admissible {f.lo[i]} .. {f.hi[i]} "
            f"(v {f.v[i]}, d {f.d[i]}){', a miss' if f.miss[i] else ''}"
            for i in rejected(f, frame)[:limit]]
