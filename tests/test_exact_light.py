"""The lit frames of the host functions against exact light and colour
(tests/exact_light.py), without a GPU.

Every colour the light pass writes is judged by what it means: Lambert light
summed over the lights and clamped at 1, with shadows only the lights whose
segment `exact_ref.occlusion` finds free, the depth ramp of the accumulated
depth, the mirror blend run backwards over the levels.  The reference gives a
value and a derived bound per channel; a frame passes where every
judged channel is one of the admissible integers, every clear miss is
(0, 0, 0, 255) and every alpha is 255.  Pixels that cannot be stated (an
undecided hit, bounce or segment of a facing light, a bounce onto a cube's edge
between two faces, a normal within its bound of perpendicular to the arriving
ray, a bound above 0.01) are excluded and counted; the cap, the bound of 0.01
and the share of channels that admit one integer (at least 95 %) are asserted
on the reference alone, before the library is called.

Each level's point is recomputed in float32 from the library's own `t` of that
level by the documented two-operation formula, after that `t` has passed
`judge_cast`; so chains do not compound.  Mirrors are axis-aligned slabs: their
normals and every mirrored direction are exact in float32 (asserted).  Curved
or rotated mirrors beyond the first bounce stay with the word-for-word suites.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import exact_light as el
import exact_ref as ex
import gpu_support as gs
import test_exact_geometry as te
from test_gpu_exact_geometry import pinhole_view

F32 = np.float32
FW, FH = te.FW, te.FH
N = FW * FH
HIT, MISS, OPEN = ex.DECIDED_HIT, ex.DECIDED_MISS, ex.UNDECIDED
CAP = te.CAPS["mixed"]
FORMATS = ("i32x4", "rgba8")

# One colour per slot (cubes, then spheres): channels distinct, in (0, 1], no
# value twice in the table.
PALETTE = [(1.0, 0.55, 0.2), (0.3, 0.85, 0.6), (0.7, 0.25, 0.95), (0.9, 0.4, 0.15),
           (0.45, 0.65, 0.35), (0.8, 0.1, 0.5)]


def coloured(pkg, scene, lights):
    nc, ns = scene.num_cubes, scene.num_spheres
    table = np.array([(*c, 255) for c in PALETTE[:nc + ns]], F32)
    rgb = table[:, :3]
    assert len(np.unique(rgb)) == rgb.size and (rgb > 0).all() and (rgb <= 1).all()
    return pkg.Scene(scene.sphere_origins, scene.sphere_radius, table[nc:], scene.cube_vertices,
                     table[:nc], np.asarray(lights, F32).reshape(-1, 4)), rgb.astype(np.float64)


# ---------------------------------------------------------------------------
# Scenes
# ---------------------------------------------------------------------------
SLAB = ([("scale", 64, 64, 2), ("translate", 16, 16, -40)], te.WHITE)
WHITE = te.WHITE


def bounce_scene(pkg):
    """flat_mirror_scene and a matte sphere so far behind the plane of the
    origins that what the slab mirrors of it lies past the ramp's end."""
    return gs.scene_from(pkg, spheres=[((40, 8, 30, 1), 7, WHITE), ((55, -5, 115, 1), 9, WHITE)],
                         cubes=[SLAB, ([("scale", 5, 4, 3), ("rotate", 0.4, 0.6, 0.2),
                                        ("translate", 30, 2, 35)], WHITE)])


def corridor_scene(pkg):
    """Two facing axis-aligned slabs, the flat-mirror slab and one behind the
    plane of the origins, and between them a matte rotated cube and a matte
    sphere.  The second slab ends inside the frame's mirrored rays, so that
    chains leave the corridor at the first and at the third bounce."""
    return gs.scene_from(pkg, spheres=[((30, 2, 10, 1), 5, WHITE)],
                         cubes=[SLAB, ([("scale", 64, 17, 2), ("translate", 40, -5.3, 22)], WHITE),
                                ([("scale", 5, 4, 3), ("rotate", 0.4, 0.6, 0.2),
                                  ("translate", 45, 0, 8)], WHITE)])


A_LIGHTS = ((40, 14, 20, 1), (-40, 14, -33, 1))
SLANTED_LIGHTS = ((-10, 40, 20, 1), (45, 5, -12, 1))
B_LIGHTS = ((5, 25, 12, 1), (20, 10, -60, 1))   # the second behind the slab
C_LIGHTS = ((10, 20, 12, 1), (50, 5, -20, 1))
D_LIGHTS = ((-10, 40, 20, 1), (45, 5, -12, 1))


def own_view(pkg, name, scene, d):
    key = ("light view", name)
    if key not in te._CACHE:
        rays = np.ascontiguousarray(te.frame_rays(d), pkg.RAY_DTYPE)
        geometry = ex.Geometry(scene)
        pairs = ex.Pairs(geometry, rays)
        te._CACHE[key] = SimpleNamespace(scene=scene, rays=rays, d=d, geometry=geometry,
                                         pairs=pairs, ref=ex.closest(pairs), name=name)
    return te._CACHE[key]


def case(pkg, name):
    """A case: the view `f` (rays and exact hits), the coloured, lit scene, the
    colour table, the slots that mirror, the camera."""
    key = ("light case", name)
    if key in te._CACHE:
        return te._CACHE[key]
    if name == "shadow":
        f, lights, mirrors = te.frame(pkg, "shadow", te.FRAME_DIRS["reference"]), A_LIGHTS, ()
    elif name == "slanted":
        f, lights, mirrors = te.frame(pkg, "frame", te.FRAME_DIRS["slanted"]), SLANTED_LIGHTS, ()
    elif name == "bounce":
        f, lights, mirrors = own_view(pkg, name, bounce_scene(pkg), te.MIRROR_DIR), B_LIGHTS, (0,)
    elif name == "corridor":
        f = own_view(pkg, name, corridor_scene(pkg), te.MIRROR_DIR)
        lights, mirrors = C_LIGHTS, (0, 1)
    elif name == "pinhole":
        f, lights, mirrors = pinhole_view(pkg), D_LIGHTS, ()
    scene, colours = coloured(pkg, f.scene, lights)
    cam = f.cam if name == "pinhole" else pkg.Camera.reference(f.d)
    c = SimpleNamespace(name=name, f=f, scene=scene, colours=colours, mirrors=mirrors, cam=cam,
                        d=None if name == "pinhole" else f.d,
                        lights=np.asarray(lights, np.float64)[:, :3])
    te._CACHE[key] = c
    return c


def reflectivity(c, **by_slot):
    r = np.zeros(len(c.colours), F32)
    for slot, value in by_slot.items():
        r[int(slot[1:])] = value
    return r


# ---------------------------------------------------------------------------
# The host functions as the cases call them (the GPU file has the kernels' twin)
# ---------------------------------------------------------------------------
class Host:
    def __init__(self, pkg):
        self.pkg = pkg

    def cast(self, c):
        return self.pkg.cast_camera(c.cam, c.scene, FW, FH)

    def bounce(self, c, hits, j):
        return self.pkg.bounce_hits(hits, c.scene, j, ray_dir=c.d)

    def lit(self, c, hits, call, fmt, refl=None, depth=0, shadows=False):
        pkg, kw = self.pkg, dict(ray_dir=c.d)
        if call == "light":
            out = pkg.light_hits(hits, c.scene, fmt, shadows=shadows, **kw)
        elif call == "reflected":  # one reflectivity everywhere
            fn = pkg.light_hits_shadowed_reflected if shadows else pkg.light_hits_reflected
            out = fn(hits, c.scene, float(refl), fmt, **kw)
        elif call == "mirrored":
            out = pkg.light_hits_mirrored(hits, c.scene, refl, depth, fmt, shadows, **kw)
        elif call == "mirrored_accel":
            out = pkg.light_hits_mirrored_accel(hits, c.scene, pkg.build_accel(c.scene), refl,
                                                depth, fmt, shadows, **kw)
        else:
            accel = pkg.build_accel(c.scene) if call == "camera_accel" else None
            out = pkg.light_camera(c.cam, c.scene, FW, FH, refl, depth, shadows, fmt, accel=accel)
        return out.reshape(N, 4) if fmt == "i32x4" else out.reshape(N)


# ---------------------------------------------------------------------------
# Levels: the exact geometry of a chain, from the library's own judged t
# ---------------------------------------------------------------------------
def spread(idx, values, fill=0):
    values = np.asarray(values)
    out = np.full((N,) + values.shape[1:], fill, values.dtype)
    out[idx] = values
    return out


def make_level(c, idx, rays, ref, t, T, D):
    """The level that the rays `rays` of the pixels `idx` reach at the
    library's parameters `t`: hit / miss / open, and for the hits the object,
    the float32 point, the exact faced normal with the bound of a cosine taken
    with it, the depth `T` and the arriving direction `D`; `out`: on a cube's
    edge between two faces, or a normal perpendicular to the ray within its
    bound."""
    g = c.f.geometry
    s = SimpleNamespace(geometry=g, rays=rays, ref=ref)
    te.exact_surfaces(s)
    o, d, _ = ex.ray_arrays(rays)
    p32 = (o.astype(F32) + np.asarray(t, F32)[:, None] * d.astype(F32)).astype(F32)
    hit = ref.status == HIT
    out, angle = np.zeros(len(idx), bool), s.angle.copy()
    for i in np.nonzero(hit)[0]:
        obj = int(ref.obj[i])
        if obj < g.nc:
            near = [k for k, tk, tolk in ref.tris[i][obj]
                    if abs(tk - ref.t[i]) <= tolk + ref.tol[i]]
            if len(near) > 1:  # the two triangles of a face, or an edge between faces
                normals = [ex.tri_normal(*g.tris[obj, k])[0] for k in near]
                worst = max(min(float(ex.angle(normals[0], m)), float(ex.angle(normals[0], -m)))
                            for m in normals[1:])
                out[i] |= worst > 1e-3
                angle[i] += worst
        else:
            # a sphere's normal is that of the point: (p - c) / |p - c| of the float32
            # point itself, which leaves the three subtractions and the normalisation
            # (exact_surfaces' 8u) and not the point's displacement along a grazing ray
            centre = g.centres[obj - g.nc].astype(np.float64)
            s.normal[i], s.cos[i] = ex.faced(ex.sphere_normal(p32[i], centre), d[i])
            angle[i] = 8 * ex.U32
        out[i] |= abs(s.cos[i]) <= angle[i] + 4 * ex.U32
    L = SimpleNamespace(hit=spread(idx, hit), miss=spread(idx, ref.status == MISS),
                        open=spread(idx, ref.status == OPEN), out=spread(idx, out & hit),
                        obj=spread(idx, np.where(hit, ref.obj, -1), -1), p32=spread(idx, p32),
                        n=spread(idx, s.normal), bound=spread(idx, angle + el.COS_ROUNDING),
                        T=(spread(idx, T[0]), spread(idx, T[1])), D=spread(idx, D),
                        t=spread(idx, np.asarray(t, np.float64)), free=None)
    L.cos = el.cosines(L.n, L.p32, c.lights)
    return L


def segments(pkg, c, L):
    """Per light and pixel of the level: FREE, HIDDEN or OPEN for the segment
    from the point to the light with the level's object left out (facing lights
    only; the others stay FREE and are never asked)."""
    if L.free is None:
        L.free = np.full(L.cos.shape, el.FREE, np.int8)
        for i, light in enumerate(c.lights):
            at = np.nonzero(L.hit & (L.cos[i] > L.bound))[0]
            if len(at):
                to = (light.astype(F32)[None, :] - L.p32[at]).astype(F32)
                rays = np.ascontiguousarray(te.rays_of(L.p32[at], to, L.obj[at]), pkg.RAY_DTYPE)
                L.free[i, at] = ex.occlusion(ex.Pairs(c.f.geometry, rays)).status
    return L.free


AXES = np.concatenate([np.eye(3), -np.eye(3)])


def levels_of(pkg, backend, c, hits, depth):
    """Levels 0 .. depth of the chains of the hit frame `hits` (the library's,
    judged here first) over the slots `c.mirrors`."""
    flat = hits.ravel()
    key = ("light levels", c.name, depth, flat["t"].tobytes())
    if key in te._CACHE:
        return te._CACHE[key]
    f = c.f
    bad = ex.judge_cast(f.pairs, f.ref, flat["t"], flat["object"])
    assert not bad, bad
    _, d, _ = ex.ray_arrays(f.rays)
    t0 = flat["t"].astype(np.float64)
    levels = [make_level(c, np.arange(N), f.rays, f.ref, flat["t"], (t0, np.zeros(N)),
                         d.astype(np.float64))]
    for j in range(1, depth + 1):
        prev = levels[-1]
        idx = np.nonzero(prev.hit & ~prev.out & np.isin(prev.obj, c.mirrors))[0]
        if not len(idx):
            break
        # a flat mirror: the normal and the mirrored direction are exact in float32
        assert (prev.n[idx][:, None, :] == AXES[None]).all(-1).any(-1).all()
        R = ex.mirror(prev.n[idx], prev.D[idx])
        assert (R.astype(F32) == R).all()
        rays = np.ascontiguousarray(te.rays_of(prev.p32[idx], R, prev.obj[idx]), pkg.RAY_DTYPE)
        pairs = ex.Pairs(f.geometry, rays)
        ref = ex.closest(pairs)
        got = backend.bounce(c, hits, j).ravel()[idx]
        bad = ex.judge_cast(pairs, ref, got["t"], got["object"])
        assert not bad, (j, bad)
        best = got["t"].astype(np.float64)
        T = prev.T[0][idx] + best
        levels.append(make_level(c, idx, rays, ref, got["t"],
                                 (T, el.rounded(T, prev.T[1][idx])), R))
    te._CACHE[key] = levels
    return levels


def lit_reference(pkg, c, levels, refl, depth, shadows):
    """The reference of one lit frame: chains of at most `depth` bounces with
    the reflectivities `refl` per slot (a number: that one everywhere)."""
    refl = np.broadcast_to(np.asarray(refl, F32), (len(c.colours),)).astype(np.float64)
    reached, bad, steps, totals = levels[0].hit.copy(), np.zeros(N, bool), [], []
    for j in range(depth + 1):
        L = levels[j]
        slot = np.maximum(L.obj, 0)
        k, total, undecided = el.factor(L.cos, L.bound, segments(pkg, c, L) if shadows else None)
        own = el.own_colour(L.T, k, c.colours[slot], j >= 1)
        r = refl[slot] if j < depth else np.zeros(N)
        goes = reached & (r != 0)
        bad |= reached & (L.out | undecided)
        steps.append((reached, goes, own, r))
        totals.append(total)
        if not goes.any():
            break
        nxt = levels[j + 1]
        assert (nxt.hit | nxt.miss | nxt.open | L.out)[goes].all()  # the level was built
        bad |= goes & nxt.open
        reached = goes & nxt.hit
    f = el.reference(N, levels[0].hit & ~bad, levels[0].miss, el.chain(steps))
    f.steps, f.totals = steps, totals
    return f


def check(f, got, label):
    assert not len(el.rejected(f, got)), (label, len(el.rejected(f, got)), el.describe(f, got))


def report(label, f):
    print(f"{label}: excluded {f.excluded:.4f}, one integer {f.sharp:.4f}, "
          f"worst bound {f.delta:.3g}")


# ---------------------------------------------------------------------------
# The cases.  Each proves on the reference alone what it is there for, then
# runs every call of `backend` in both formats.
# ---------------------------------------------------------------------------
def case_lit(pkg, backend, name):
    """a. lit and shadowed frames."""
    c = case(pkg, name)
    hits = backend.cast(c)
    L0 = levels_of(pkg, backend, c, hits, 0)[0]
    kinds = te.kinds_of(c.f.geometry, L0.obj[L0.hit])
    assert min(kinds.values()) >= 100, kinds
    plain = lit_reference(pkg, c, [L0], 0, 0, False)
    el.check_reference(plain, CAP)
    total = plain.totals[0]
    if name == "slanted":
        te.exact_surfaces(c.f)  # far roots and normals that have to be turned
        assert (c.f.ref.far & L0.hit).sum() >= 30 and ((c.f.cos > 0) & L0.hit).sum() >= 30
        runs = [(plain, "light", False), (plain, "mirrored", False)]
    else:
        shadowed = lit_reference(pkg, c, [L0], 0, 0, True)
        el.check_reference(shadowed, CAP)
        judged = plain.judged & shadowed.judged
        changed = np.abs(shadowed.v - plain.v).max(-1) > 1.0  # (by a whole step of a channel)
        counts = {"0 < k < 1": int((judged & (total > 0.01) & (total < 0.99)).sum()),
                  "clamped": int((judged & (total > 1.01)).sum()),
                  "shadows change k": int((judged & changed).sum()),
                  "a light behind": int((judged & (L0.cos < -L0.bound).any(0)).sum())}
        print(f"{name}: {kinds}, {counts}")
        assert counts["0 < k < 1"] >= 200 and counts["clamped"] >= 100, counts
        assert counts["shadows change k"] >= 100 and counts["a light behind"] >= 20, counts
        runs = [(plain, "light", False), (shadowed, "light", True), (plain, "mirrored", False),
                (shadowed, "mirrored_accel", True)]
    refl = reflectivity(c)
    for f, call, shadows in runs:
        for fmt in FORMATS:
            check(f, backend.lit(c, hits, call, fmt, refl=refl, depth=0, shadows=shadows),
                  (name, call, shadows, fmt))
        report(f"{name} {call} shadows={shadows}", f)


def bounce_references(pkg, backend, c, hits, r):
    levels = levels_of(pkg, backend, c, hits, 1)
    L0, L1 = levels
    assert (L0.hit & (L0.obj == 0)).sum() == N  # the slab fills the frame
    refl = reflectivity(c, s0=r)
    plain = lit_reference(pkg, c, levels, refl, 1, False)
    shadowed = lit_reference(pkg, c, levels, refl, 1, True)
    for f in (plain, shadowed):
        el.check_reference(f, CAP)
    kinds = te.kinds_of(c.f.geometry, L1.obj[L1.hit])
    assert sum(kinds.values()) >= 100 and min(kinds.values()) >= 50, kinds  # something, both kinds
    assert L1.miss.sum() >= 100, L1.miss.sum()
    assert (L1.hit & (L1.T[0] > 181)).sum() >= 30  # past the ramp's end: the clamp at 0
    hidden = (L1.free == el.HIDDEN) & (L1.cos > L1.bound)
    print(f"bounce: meets {kinds}, nothing {L1.miss.sum()}, past the ramp "
          f"{(L1.hit & (L1.T[0] > 181)).sum()}, a hidden facing light at level 1 "
          f"{(shadowed.judged & hidden.any(0)).sum()}")
    assert (shadowed.judged & hidden.any(0)).sum() >= 30
    return refl, plain, shadowed


def case_bounce(pkg, backend, r):
    """b. one bounce at a flat mirror of reflectivity r."""
    c = case(pkg, "bounce")
    hits = backend.cast(c)
    refl, plain, shadowed = bounce_references(pkg, backend, c, hits, r)
    for f, call, shadows, value in ((plain, "reflected", False, r), (plain, "mirrored", False, refl),
                                    (shadowed, "reflected", True, r),
                                    (shadowed, "mirrored", True, refl),
                                    (shadowed, "mirrored_accel", True, refl)):
        for fmt in FORMATS:
            check(f, backend.lit(c, hits, call, fmt, refl=value, depth=1, shadows=shadows),
                  ("bounce", r, call, shadows, fmt))
    report(f"bounce r={r}", plain)
    report(f"bounce r={r} shadows", shadowed)
    return c, hits, refl, plain, shadowed


CORRIDOR_R = dict(s0=0.75, s1=0.25)


def corridor_reference(pkg, backend, c, hits, depth, shadows):
    levels = levels_of(pkg, backend, c, hits, 3)
    f = lit_reference(pkg, c, levels, reflectivity(c, **CORRIDOR_R), depth, shadows)
    el.check_reference(f, CAP)
    # how the chains end: by a matte object at levels 1 and 2, by the depth, by a miss
    ends = {}
    for j, (reached, goes, _, _) in enumerate(f.steps):
        matte = reached & ~goes & ~np.isin(levels[j].obj, c.mirrors) & f.judged
        ends[f"matte {j}"] = int(matte.sum())
        if j == depth:
            ends["depth"] = int((reached & np.isin(levels[j].obj, c.mirrors) & f.judged).sum())
        elif j + 1 < len(levels):
            ends["miss"] = ends.get("miss", 0) + int((goes & levels[j + 1].miss & f.judged).sum())
    print(f"corridor depth={depth}: chains end {ends}")
    assert min(ends["matte 1"], ends["matte 2"], ends["depth"], ends["miss"]) >= 30, ends
    return f


def case_corridor(pkg, backend, depth, shadows):
    """c. chains between two flat mirrors."""
    c = case(pkg, "corridor")
    hits = backend.cast(c)
    f = corridor_reference(pkg, backend, c, hits, depth, shadows)
    refl = reflectivity(c, **CORRIDOR_R)
    for call in ("mirrored", "mirrored_accel"):
        for fmt in FORMATS:
            check(f, backend.lit(c, hits, call, fmt, refl=refl, depth=depth, shadows=shadows),
                  ("corridor", depth, shadows, call, fmt))
    report(f"corridor depth={depth} shadows={shadows}", f)


def case_camera(pkg, backend):
    """d. camera views: a pinhole at depth 0, the reference camera at depth 1."""
    c = case(pkg, "pinhole")
    te.check_frame_caps(c.f)
    hits = backend.cast(c)
    L0 = levels_of(pkg, backend, c, hits, 0)[0]
    kinds = te.kinds_of(c.f.geometry, L0.obj[L0.hit])
    assert min(kinds.values()) >= 50, kinds
    for shadows in (False, True):
        f = lit_reference(pkg, c, [L0], 0, 0, shadows)
        el.check_reference(f, CAP)
        for call in ("camera", "camera_accel"):
            for fmt in FORMATS:
                check(f, backend.lit(c, hits, call, fmt, refl=reflectivity(c), depth=0,
                                     shadows=shadows), ("pinhole", call, shadows, fmt))
        report(f"pinhole shadows={shadows}", f)
    c = case(pkg, "bounce")
    hits = backend.cast(c)
    refl, plain, shadowed = bounce_references(pkg, backend, c, hits, 0.25)
    for f, shadows in ((plain, False), (shadowed, True)):
        for call in ("camera", "camera_accel"):
            for fmt in FORMATS:
                check(f, backend.lit(c, hits, call, fmt, refl=refl, depth=1, shadows=shadows),
                      ("reference camera", call, shadows, fmt))


@pytest.mark.parametrize("name", ["shadow", "slanted"])
def test_lit_and_shadowed_frames(pkg, name):
    case_lit(pkg, Host(pkg), name)


@pytest.mark.parametrize("r", [0.25, 0.75])
def test_one_bounce(pkg, r):
    case_bounce(pkg, Host(pkg), r)


@pytest.mark.parametrize("depth, shadows", [(2, False), (2, True), (3, False), (3, True)])
def test_chains_on_flat_mirrors(pkg, depth, shadows):
    case_corridor(pkg, Host(pkg), depth, shadows)


def test_camera_views(pkg):
    case_camera(pkg, Host(pkg))


# ---------------------------------------------------------------------------
# The judge can tell: a plain float64 pixel function and deliberately wrong
# variants of it (test code; nothing is patched into the library)
# ---------------------------------------------------------------------------
VARIANTS = ["normal_not_faced", "factor_not_clamped", "shadows_ignored", "own_object_occludes",
            "mirrored_object_occludes", "primary_object_left_out", "channels_reversed",
            "sphere_slots_first", "light_not_normalised", "ramp_from_the_bounce_alone",
            "ramp_not_clamped", "blend_weights_swapped", "blend_run_forwards",
            "one_reflectivity"]


def plain_occluded(g, p, to, *skips):
    """Any object but `skips` (arrays of slots) strictly inside the segments."""
    flags = np.zeros(len(p), bool)
    with np.errstate(all="ignore"):
        for j in range(g.nc + g.ns):
            on = np.ones(len(p), bool)
            for s in skips:
                on &= s != j
            if j < g.nc:
                for k in range(12):
                    ok, t = te.plain_triangle(p, to, g.tris[j, k], None)
                    flags |= on & ok & (t > 0) & (t < 1)
            else:
                s0, s1 = te.plain_sphere(p, to, g.centres[j - g.nc], g.radius[j - g.nc], None)
                flags |= on & (((s0 > 0) & (s0 < 1)) | ((s1 > 0) & (s1 < 1)))
    return flags


def plain_normals(g, obj, tri, p, D, variant):
    n = np.zeros((len(obj), 3))
    for i in np.nonzero(obj >= 0)[0]:
        if obj[i] < g.nc:
            v0, v1, v2 = g.tris[obj[i], tri[i]].astype(np.float64)
            n[i] = ex.unit(np.cross(v1 - v0, v2 - v0))
        else:
            n[i] = ex.unit(p[i] - g.centres[obj[i] - g.nc])
    if variant != "normal_not_faced":
        n = np.where(((n * D).sum(-1) > 0)[:, None], -n, n)
    return n


def plain_lit(pkg, c, hits, refl, depth, shadows, variant=None):
    """The (N, 4) frame of a plain float64 statement of DESIGN.md §3.1a-e over
    the hit frame `hits`; each level's point is the float32 one of the
    documented formula, as the library's."""
    g = c.f.geometry
    o, d, _ = ex.ray_arrays(c.f.rays)
    flat = hits.ravel()
    refl = np.asarray(refl, np.float64)
    colours = c.colours
    if variant == "channels_reversed":
        colours = colours[:, ::-1]
    if variant == "sphere_slots_first":
        colours = np.concatenate([colours[g.nc:], colours[:g.nc]])
    obj = flat["object"].astype(np.int64)
    tri = te.plain_cast(g, c.f.rays)[2]
    tri = np.where((obj >= 0) & (obj < g.nc), np.maximum(tri, 0), -1)
    p = (o.astype(F32) + flat["t"][:, None] * d.astype(F32)).astype(F32)
    D, T = d.astype(np.float64), flat["t"].astype(np.float64)
    reached, first = obj >= 0, obj.copy()
    steps = []
    for j in range(depth + 1):
        slot = np.maximum(obj, 0)
        n = plain_normals(g, np.where(reached, obj, -1), tri, p.astype(np.float64), D, variant)
        k = np.zeros(N)
        for light in c.lights:
            to = (light.astype(F32)[None] - p).astype(F32).astype(np.float64)
            cos = (n * to).sum(-1)
            if variant != "light_not_normalised":
                cos = cos / np.linalg.norm(to, axis=-1)
            lit = reached & (cos > 0)
            if shadows and variant != "shadows_ignored":
                skips = [obj]
                if (j == 0 and variant == "own_object_occludes") or \
                        (j == 1 and variant == "mirrored_object_occludes"):
                    skips = []
                if j == 1 and variant == "primary_object_left_out":
                    skips = [obj, first]
                lit &= ~plain_occluded(g, p.astype(np.float64), to, *skips)
            k += np.where(lit, cos, 0.0)
        if variant != "factor_not_clamped":
            k = np.minimum(k, 1.0)
        ramp = 255.0 - 255.0 * T / 180.0
        if j >= 1 and variant != "ramp_not_clamped":
            ramp = np.maximum(ramp, 0.0)
        own = (ramp * k)[:, None] * colours[slot]
        r = refl[np.maximum(first, 0) if variant == "one_reflectivity" else slot] \
            if j < depth else np.zeros(N)
        goes = reached & (r != 0)
        steps.append((reached, goes, own, r))
        if not goes.any():
            break
        R = D - 2 * (n * D).sum(-1, keepdims=True) * n
        rays = np.ascontiguousarray(te.rays_of(p, np.where(goes[:, None], R, 1.0),
                                               np.where(goes, obj, -1)), pkg.RAY_DTYPE)
        best, obj2, tri2 = te.plain_cast(g, rays)
        p = (p + best.astype(F32)[:, None] * R.astype(F32)).astype(F32)
        T = best if variant == "ramp_from_the_bounce_alone" else T + best
        reached, obj, tri, D = goes & (obj2 >= 0), np.where(goes, obj2, -1), tri2, R

    def mix(a, r, C):
        r = r[:, None]
        return C + r * (a - C) if variant == "blend_weights_swapped" else a + r * (C - a)

    if variant == "blend_run_forwards":
        # the chain's end, then the levels blended in the order they were reached
        C = np.zeros((N, 3))
        for reached, goes, own, r in steps:
            C = np.where((reached & ~goes)[:, None], own, C)
        for reached, goes, own, r in steps:
            C = np.where(goes[:, None], mix(own, r, C), C)
    else:
        C = np.zeros((N, 3))
        for reached, goes, own, r in steps[::-1]:
            C = np.where(goes[:, None], mix(own, r, C), np.where(reached[:, None], own, 0.0))
    out = np.full((N, 4), 255, np.int64)
    out[:, :3] = np.trunc(C)
    return out


def variant_cases(pkg):
    """(label, case, reference, reflectivities, depth, shadows) the variants
    are shown to, built with the host functions' judged t."""
    host = Host(pkg)
    a, s = case(pkg, "shadow"), case(pkg, "slanted")
    ha, hs = host.cast(a), host.cast(s)
    yield ("shadow", a, ha, lit_reference(pkg, a, levels_of(pkg, host, a, ha, 0), 0, 0, True),
           reflectivity(a), 0, True)
    yield ("slanted", s, hs, lit_reference(pkg, s, levels_of(pkg, host, s, hs, 0), 0, 0, False),
           reflectivity(s), 0, False)
    b = case(pkg, "bounce")
    hb = host.cast(b)
    refl, _, shadowed = bounce_references(pkg, host, b, hb, 0.25)
    yield "bounce", b, hb, shadowed, refl, 1, True
    k = case(pkg, "corridor")
    hk = host.cast(k)
    yield ("corridor", k, hk, corridor_reference(pkg, host, k, hk, 3, True),
           reflectivity(k, **CORRIDOR_R), 3, True)


def rejected_by(pkg, variant):
    """The first case that rejects `variant` on at least 20 judged pixels, and
    the counts of all that were asked."""
    counts = {}
    for label, c, hits, f, refl, depth, shadows in variant_cases(pkg):
        counts[label] = len(el.rejected(f, plain_lit(pkg, c, hits, refl, depth, shadows, variant)))
        if counts[label] >= 20:
            return label, counts
    return None, counts


def test_the_plain_pixel_passes(pkg):
    """The judge is not so strict that a correct float64 statement fails it."""
    for label, c, hits, f, refl, depth, shadows in variant_cases(pkg):
        check(f, plain_lit(pkg, c, hits, refl, depth, shadows), label)


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_wrong_pixel_is_rejected(pkg, variant):
    where, counts = rejected_by(pkg, variant)
    print(f"{variant}: rejected by {where}, pixels {counts}")
    assert where is not None, f"no case rejects {variant}: {counts}"
