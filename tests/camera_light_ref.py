"""The light pass of a camera view -- TEST INFRASTRUCTURE ONLY.

A numpy restatement of DESIGN.md §3.1i for rt_light_camera / rt_bounce_camera.
Level 0 of every pixel's chain comes from tests/rays_ref.py (`camera`, `cast`)
with tests/reflect_ref.py's `normal_at` at the point o + best * d; from there
it is tests/mirror_ref.py's `Level` / `Chain` machinery as it is: the walks of
`chain_ref`'s loop, `run`, `factor`, `bounce`, `stats`.  Only the frame around
the backward blend is new: a pixel whose ray meets nothing is (0, 0, 0, 255).
"""
import numpy as np

import light_ref as lr
import mirror_ref as mr
import rays_ref as yr
import reflect_ref as rr
from gpu_support import F32

MAX_BOUNCES = mr.MAX_BOUNCES
DEPTHS = (0, 1, 2, 8)
BOUNCES = (0, 1, 2, 8)
LIT_FORMATS = ("i32x4", "rgba8")


class CameraChain(mr.Chain):
    """mirror_ref.Chain whose level 0 is the cast of the camera's rays.
    rays, hits, tri, far: rays_ref.camera's and rays_ref.cast's.  bounce(0) is
    rt_cast_camera's frame."""

    def lit(self, reflectivity, depth, shadows=False):
        """rt_light_camera's int32x4 frame."""
        if reflectivity is None:  # (only where no slot can be read)
            reflectivity, depth = np.zeros(yr.slots(self.scene), F32), 0
        out = np.zeros(self.alive.shape + (4,), np.int32)
        out[..., 3] = 255
        C = [np.zeros(self.alive.shape, F32) for _ in range(3)]
        with np.errstate(all="ignore"):
            for reached, goes, a, r in reversed(self.run(reflectivity, depth, shadows)):
                for ch in range(3):
                    C[ch] = np.where(reached & ~goes, a[ch], C[ch])
                    C[ch] = np.where(goes, rr.mix(a[ch], C[ch], r), C[ch])
            for ch in range(3):
                out[..., ch] = np.where(self.alive, lr.x86_int(C[ch]), 0)
        return out

    def frame(self, reflectivity, depth, shadows, fmt, oracle):
        out = self.lit(reflectivity, depth, shadows)
        return out if fmt == "i32x4" else oracle.pack_rgba8(out)


def camera_chain(scene, cam, width, rows, depth=MAX_BOUNCES):
    """The geometry of levels 0 .. depth of every pixel's chain through `cam`."""
    c = CameraChain()
    c.scene, c._k = scene, {}
    c.rays = yr.camera(cam, width, rows)
    c.hits, c.tri, c.far = yr.cast(scene, c.rays)
    o, d = yr.origins(c.rays), yr.directions(c.rays)
    t, obj = c.hits["t"], c.hits["object"].astype(np.int32)
    c.alive = obj >= 0
    lv = mr.Level()
    lv.obj, lv.best, lv.T = obj, np.array(t), np.array(t)
    with np.errstate(all="ignore"):
        lv.p = (o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2])
        lv.n = rr.normal_at(scene, obj, c.tri, lv.p, d)
        lv.D = [np.array(a) for a in d]
        c.levels = [lv]
        for _ in range(depth):
            R = rr.mirror_dir({"nx": lv.n[0], "ny": lv.n[1], "nz": lv.n[2]}, np.array(lv.D))
            best, obj2, tri2, _ = rr.walk(scene, lv.obj, lv.p, R)
            nx = mr.Level()
            nx.obj, nx.best = obj2, best
            nx.p = (lv.p[0] + best * R[0], lv.p[1] + best * R[1], lv.p[2] + best * R[2])
            nx.n = rr.normal_at(scene, obj2, tri2, nx.p, R)
            nx.D, nx.T = list(R), lv.T + best
            c.levels.append(nx)
            lv = nx
    return c


_CACHE = {}


def restated(key, scene, cam, width, rows):
    """camera_chain, once per key (the caller's name of scene, lights, camera
    and band), read by the CPU and the GPU file."""
    if key not in _CACHE:
        _CACHE[key] = camera_chain(scene, cam, width, rows)
    return _CACHE[key]


def kinds(c, reflectivity, depth=2):
    """What a frame holds, by name -> number of pixels: the level-0 kinds, how
    the chains end at max_bounces `depth`, how deep the geometric chains get,
    and (with lights) pixels a light is hidden from and pixels one reaches."""
    nc = c.scene.num_cubes
    obj = c.levels[0].obj
    _, last, cause = c.stats(reflectivity, depth)
    out = {"miss0": int((obj < 0).sum()), "cube0": int(((obj >= 0) & (obj < nc)).sum()),
           "sphere0": int((obj >= nc).sum()), "far_root0": int((c.far & (obj >= nc)).sum()),
           "ends_matte": int(cause["matte"].sum()), "ends_depth": int(cause["depth"].sum()),
           "ends_miss": int(cause["miss"].sum()),
           "level2": int((c.levels[2].obj >= 0).sum()),
           "level8": int((c.levels[MAX_BOUNCES].obj >= 0).sum())}
    if len(np.asarray(c.scene.lights).reshape(-1, 4)):
        import shadow_reflect_ref as srr
        lv = c.levels[0]
        at = srr.shadow_at(c.scene, lv.obj, lv.n, lv.p)
        out["hidden"] = int(at.occluded.any(0).sum())
        out["reached"] = int((at.cast & ~at.occluded).any(0).sum())
    return out


def host_frames(pkg, cam, scene, width, height, refl, rows=None, accel=None, depths=DEPTHS,
                bounces=BOUNCES):
    """(label, frame) of every output of the two host calls."""
    for b in bounces:
        yield ("bounce", b, False), pkg.bounce_camera(cam, scene, width, height, b, rows=rows,
                                                      accel=accel)
    for depth in depths:
        for shadows in (False, True):
            for fmt in LIT_FORMATS:
                yield (fmt, depth, shadows), pkg.light_camera(cam, scene, width, height, refl,
                                                              depth, shadows, fmt, rows=rows,
                                                              accel=accel)


def want_frame(c, oracle, label, refl):
    what, depth, shadows = label
    return c.bounce(depth) if what == "bounce" else c.frame(refl, depth, shadows, what, oracle)
