"""Mirror chains with per-object reflectivity -- TEST INFRASTRUCTURE ONLY.

A numpy restatement of DESIGN.md §3.1e for rt_bounce_hits /
rt_light_hits_mirrored.  The pieces are tests/reflect_ref.py's (`mirror_dir`,
`walk`, `normal_at`, `factor_at`, `ramp`, `mix`) and tests/shadow_reflect_ref.py's
`shadow_at`; what is added here is the level loop (`chain_ref`: the geometry of
every level, followed without regard to reflectivity) and the backward blend
(`Chain.lit`), one ufunc per written operation (numpy never contracts), in the
written order, in float32.
"""
import numpy as np

import light_ref as lr
import reflect_ref as rr
import shadow_reflect_ref as srr
from gpu_support import F32
from hit_ref import K_FAR, REF_DIR, hit_dtype

MAX_BOUNCES = 8  # RT_MAX_BOUNCES
DEPTHS = (0, 1, 2, 3, 8)


# ---------------------------------------------------------------------------
# Scenes
# ---------------------------------------------------------------------------
CHAIN_W = CHAIN_H = srr.CLASS_W
CHAIN_KEY = "shadow_reflect_class"  # shadow_reflect_ref.class_scene's hit frame


def chain_scene(pkg, lights=srr.CLASS_LIGHTS):
    """shadow_reflect_ref.class_scene: cube 0 the face at z = -50, cube 1 the
    box, cube 2 the turned cube, then spheres (slots 3 .. 8): 0 at (64, 64,
    -30), 1 unseen in front of the ray origins, 2 and 3 side by side, 4 unseen
    left of the frame, 5 hovering 6 above the face.  With CHAIN_REFLECTIVITY
    the face, the side-by-side spheres and the hovering sphere are mirrors (1),
    the turned cube mirrors a quarter (0.25), the box, sphere 0 and the two
    unseen spheres are matte (0): the flanks of the hovering sphere mirror down
    onto the face, which mirrors on, and the spheres side by side throw rays
    to and fro, each back into the other (obj_2 == obj_0)."""
    return srr.class_scene(pkg, lights)


CHAIN_REFLECTIVITY = np.array([1, 0, 0.25, 0, 0, 1, 1, 0, 1], F32)

CORRIDOR_W, CORRIDOR_H = 64, 48
CORRIDOR_HALF_ANGLE = np.pi / 30  # 6 degrees: an opening of 12


def corridor_scene(pkg, lights=lr.THREE_LIGHTS):
    """Two slabs 200 long, turned by 6 degrees about y to either side, whose
    inner faces open towards the ray origins in a narrow V about x = 32 that
    closes near z = -200: a ray that enters is thrown from face to face more
    than eight times, and its depth is past the ramp's end (180) long before."""
    def slab(sign):
        return [("scale", 1, 40, 100), ("rotate", 0, sign * CORRIDOR_HALF_ANGLE, 0),
                ("translate", 32 + sign * (1.5 + 100 * np.sin(CORRIDOR_HALF_ANGLE)), 24, -100)]
    return rr.plus(pkg, pkg.Scene(lights=np.array(lights, F32).reshape(-1, 4)),
                   cubes=[(slab(-1), (1.0, 0.7, 0.3, 255)), (slab(1), (0.3, 0.7, 1.0, 255))])


CORRIDOR_REFLECTIVITY = np.array([1, 1], F32)

WAVE_W = WAVE_H = 128
WAVE_LIGHTS = [(64, 64, 300, 1)]


def wave_scene(pkg, lights=WAVE_LIGHTS):
    """Cube 0: a face at z = -50 far wider than the frame.  Cube 1: a matte
    strip in front of it over x >= 64 and rows 44 .. 84, on which sit spheres
    2 .. 6 (slots 4 .. 8), mirrors of r = 3.5 at x = 100: in those rows the
    right 64-pixel segment ends on the strip without a walk but for the at
    most seven lanes on a sphere, which go on alone.  In front of the ray
    origins, unseen: sphere 0 (slot 2), a mirror of r = 60 at (32, 40, 80),
    over the left segments of the upper rows: the face mirrors straight back
    into its underside, which throws the rays down onto the face again; sphere
    1 (slot 3), matte, r = 45 at (32, 110, 200), over the left segments of the
    lower rows: every chain there ends on it, at level 1."""
    face = [("scale", 400, 400, 10), ("translate", 64, 64, -60)]
    strip = [("scale", 32, 20, 2), ("translate", 96, 64, -42)]
    small = [((100, y, -36, 1), 3.5, (0.9, 0.2, 0.2, 255)) for y in (48, 56, 64, 72, 80)]
    return rr.plus(pkg, pkg.Scene(lights=np.array(lights, F32).reshape(-1, 4)),
                   spheres=[((32, 40, 80, 1), 60, (0.9, 0.9, 0.1, 255)),
                            ((32, 110, 200, 1), 45, (0.2, 0.9, 0.4, 255))] + small,
                   cubes=[(face, (1.0, 0.7, 0.3, 255)), (strip, (0.5, 0.5, 0.5, 255))])


WAVE_REFLECTIVITY = np.array([1, 0, 1, 0, 1, 1, 1, 1, 1], F32)


# ---------------------------------------------------------------------------
# The restatement
# ---------------------------------------------------------------------------
class Level:
    """One level of every pixel's chain: obj (-1: the chain did not get here),
    the point p, the faced normal n, the direction D it was reached along, the
    depth T; best: the parameter of the bounce that reached it (level >= 1)."""


class Chain:
    """levels[j]: Level j of the geometric chain (reflectivity ignored), j = 0
    .. depth.  bounce(b): rt_bounce_hits' frame.  lit(reflectivity, depth,
    shadows): rt_light_hits_mirrored's int32x4 frame; stats(...): how the
    chains of that frame end."""

    def bounce(self, b):
        lv = self.levels[b]
        out = np.empty(lv.obj.shape, hit_dtype())
        out["t"] = np.where(lv.obj >= 0, lv.best, K_FAR)
        out["object"] = lv.obj
        return out

    def factor(self, j, shadows):
        """k_j per pixel (1 without lights and where the chain did not get to j)."""
        key = (j, bool(shadows))
        if key not in self._k:
            lv = self.levels[j]
            lights = np.ascontiguousarray(self.scene.lights, F32).reshape(-1, 4)
            if not len(lights):
                k = np.ones(lv.obj.shape, F32)
            elif shadows:
                k = srr.shadow_at(self.scene, lv.obj, lv.n, lv.p).k
            else:
                k = np.where(lv.obj >= 0, rr.factor_at(lv.n, lv.p, lights), F32(1.0)).astype(F32)
            self._k[key] = k
        return self._k[key]

    def run(self, reflectivity, depth, shadows):
        """The forward pass: per level j <= depth the pixels whose chain
        reached it, went on from it, and the own colour a_j and r_j there."""
        refl = np.asarray(reflectivity, F32).reshape(-1)
        refl = np.where((refl >= 0) & (refl <= 1), refl, F32(0.0)).astype(F32)
        table = np.concatenate([np.ascontiguousarray(self.scene.cube_colours, F32).reshape(-1, 4),
                                np.ascontiguousarray(self.scene.sphere_colours, F32).reshape(-1, 4),
                                np.array([[0, 0, 0, 255]], F32)])
        rtable = np.concatenate([refl, np.zeros(1, F32)])  # [-1]: nothing
        reached = self.alive
        out = []
        with np.errstate(all="ignore"):
            for j in range(depth + 1):
                lv = self.levels[j]
                lit = rr.ramp(lv.T, j >= 1) * self.factor(j, shadows)
                colour = table[lv.obj]
                a = [lit * colour[..., ch] for ch in range(3)]
                r = rtable[lv.obj] if j < depth else np.zeros(lv.obj.shape, F32)
                goes = reached & (r != 0)
                out.append((reached, goes, a, r))
                if j < depth:
                    reached = goes & (self.levels[j + 1].obj >= 0)
        return out

    def lit(self, reflectivity, depth, shadows=False):
        lv0 = self.levels[0]
        k0 = np.where(self.hits["object"] >= 0, self.factor(0, shadows), F32(1.0)).astype(F32)
        out = np.array(lr.lit_ref(self.oracle, self.scene, self.hits, self.row_begin,
                                  self.ray_dir, surf=self.surf, k=k0))
        C = [np.zeros(lv0.obj.shape, F32) for _ in range(3)]
        with np.errstate(all="ignore"):
            for reached, goes, a, r in reversed(self.run(reflectivity, depth, shadows)):
                for ch in range(3):
                    C[ch] = np.where(reached & ~goes, a[ch], C[ch])
                    C[ch] = np.where(goes, rr.mix(a[ch], C[ch], r), C[ch])
            for ch in range(3):
                out[..., ch] = np.where(self.alive, lr.x86_int(C[ch]), out[..., ch])
        return out

    def stats(self, reflectivity, depth):
        """walks: the bounce walks of each pixel's chain.  last: the level the
        chain ended at (for a miss: the level the missing walk left).  cause:
        "miss" / "matte" / "depth" frames (False where there is no chain)."""
        steps = self.run(reflectivity, depth, False)
        walks = np.zeros(self.alive.shape, np.int32)
        last = np.full(self.alive.shape, -1, np.int32)
        cause = {c: np.zeros(self.alive.shape, bool) for c in ("miss", "matte", "depth")}
        for j, (reached, goes, _, _) in enumerate(steps):
            walks += goes
            ended = reached & ~goes
            last[ended] = j
            cause["depth" if j == depth else "matte"] |= ended
            if j < depth:
                missed = goes & (self.levels[j + 1].obj < 0)
                last[missed] = j
                cause["miss"] |= missed
        return walks, last, cause


def chain_ref(oracle, scene, hits, row_begin=0, ray_dir=REF_DIR, depth=MAX_BOUNCES):
    """The geometry of levels 0 .. depth of every pixel's chain."""
    c = Chain()
    c.oracle, c.scene, c.hits, c.row_begin, c.ray_dir = oracle, scene, hits, row_begin, ray_dir
    c._k = {}
    t, obj = hits["t"], hits["object"].astype(np.int32)
    c.alive = (obj >= 0) & ~(t == K_FAR)
    c.surf = lr.surfaces_ref(oracle, scene, hits, row_begin, ray_dir)
    d = np.asarray(ray_dir, F32)
    lv = Level()
    lv.obj, lv.p = obj, lr.hit_points(hits, row_begin, ray_dir)
    lv.n = [np.array(c.surf[a]) for a in ("nx", "ny", "nz")]
    lv.D = [np.full(obj.shape, d[a], F32) for a in range(3)]
    lv.T, lv.best = np.array(t), np.full(obj.shape, K_FAR, F32)
    c.levels = [lv]
    with np.errstate(all="ignore"):
        for _ in range(depth):
            R = rr.mirror_dir({"nx": lv.n[0], "ny": lv.n[1], "nz": lv.n[2]}, np.array(lv.D))
            best, obj2, tri2, _ = rr.walk(scene, lv.obj, lv.p, R)
            nx = Level()
            nx.obj, nx.best = obj2, best
            nx.p = (lv.p[0] + best * R[0], lv.p[1] + best * R[1], lv.p[2] + best * R[2])
            nx.n = rr.normal_at(scene, obj2, tri2, nx.p, R)
            nx.D, nx.T = list(R), lv.T + best
            c.levels.append(nx)
            lv = nx
    return c


def alone(steps, alive):
    """Per 64-pixel segment (a wave where the width is a multiple of 64) of
    Chain.run's `steps`: at some level one to eight lanes go on while other
    lanes of the wave held a chain that has ended."""
    chains = alive.reshape(-1, 64).sum(1)
    out = np.zeros(chains.shape, bool)
    for _, goes, _, _ in steps:
        g = goes.reshape(-1, 64).sum(1)
        out |= (g >= 1) & (g <= 8) & (chains > g)
    return out


def wave_kinds(steps, alive):
    """(every chain of the wave ends at level 1, every hit lane reaches a
    level >= 2, one to eight lanes go on alone), one bool per segment."""
    hit = alive.reshape(-1, 64)
    reached1, reached2 = steps[1][0].reshape(-1, 64), steps[2][0].reshape(-1, 64)
    return (hit.any(1) & (reached1 == hit).all(1) & ~reached2.any(1),
            hit.any(1) & (reached2 == hit).all(1), alone(steps, alive))


# ---------------------------------------------------------------------------
# What the tests of both files (CPU and GPU) share
# ---------------------------------------------------------------------------
def restated(oracle, key, scene, w, h, rows=None, d=REF_DIR):
    """(hits, chain_ref's geometry), once per key, direction and light set."""
    return lr.restated(chain_ref, oracle, key, scene, w, h, rows, d)


def mixed(scene):
    """One reflectivity per slot: 1, 0.25, 1, 0, 1, 0.25, ..."""
    return np.resize(np.array([1, 0.25, 1, 0], F32), scene.num_cubes + scene.num_spheres)


def chain_facts(c):
    """What the chain scene is there for."""
    refl = CHAIN_REFLECTIVITY
    assert set(refl.tolist()) == {0.0, 0.25, 1.0}
    walks, last, cause = c.stats(refl, 8)
    assert (walks == 1).sum() >= 100 and (walks == 2).sum() >= 100  # 14961, 659
    assert (walks >= 3).sum() >= 100                                # 154
    # ended at a level >= 2 by each cause, at depth 3: 98, 27, 56
    _, last, cause = c.stats(refl, 3)
    for name in ("miss", "matte", "depth"):
        assert (cause[name] & (last >= 2)).sum() >= 20, name
    # the primary object is a candidate again: the hovering sphere, the face, the sphere
    went_on = c.run(refl, 8, False)[1][1]
    back = went_on & (c.levels[2].obj == c.levels[0].obj)
    assert back.sum() >= 20  # 58


def corridor_facts(c):
    """At least 64 pixels reach level RT_MAX_BOUNCES, the ramp long dead."""
    deep = c.bounce(MAX_BOUNCES)["object"] >= 0
    assert deep.sum() >= 64  # 1632
    assert (c.levels[MAX_BOUNCES].T[deep] > 180).all()
    assert (c.levels[2].T[c.levels[2].obj >= 0] > 180).sum() >= 64  # the clamp, early on


def wave_facts(c):
    steps = c.run(WAVE_REFLECTIVITY, 8, False)
    for kind in wave_kinds(steps, c.alive):  # 44, 41, 78
        assert kind.sum() >= 20
