"""rt_cast_rays / rt_occlude_rays / rt_camera_rays / rt_cast_camera without a
GPU: the host functions against the numpy restatement (tests/rays_ref.py) of
DESIGN.md §3.1f, against the light pass's own frames, and against the oracle's
triangle test.

Every comparison is on raw 32-bit words (bytes for the occlusion flags); the
only tolerances are the pinhole helper's, which claims no bit-exactness.  Every
case first asserts on the restatement that it contains what it is there for.
No created NaN can reach an output word: `best` is only written from a value
that passed `sf < best` (rays_ref.check_edge asserts it on every edge case).
"""
import ctypes
import inspect
import math
import shutil

import numpy as np
import pytest

import light_contract as lc
import light_ref as lr
import rays_ref as yr
import reflect_ref as rr
import shadow_ref as sr
from hit_ref import K_FAR, REF_DIR
from light_ref import words

F32 = np.float32


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(words(got) if got.dtype.itemsize >= 4 else got,
                       words(want) if want.dtype.itemsize >= 4 else want)


def compare(pkg, scene, rays, label=""):
    """cast_rays (with and without triangles) and occlude_rays of the host
    against the restatement; returns the restatement's (hits, tri, far, occ)."""
    hits, tri, far = yr.cast(scene, rays)
    occ = yr.occlude(scene, rays)[0]
    got, got_tri = pkg.cast_rays(rays, scene, triangles=True)
    assert got.dtype == pkg.HIT_DTYPE and same(got, hits.astype(pkg.HIT_DTYPE)), f"{label} hits"
    assert same(got_tri, tri), f"{label} triangles"
    assert same(pkg.cast_rays(rays, scene), got), f"{label} hits without triangles"
    assert same(pkg.occlude_rays(rays, scene), occ), f"{label} occluded"
    return hits, tri, far, occ


# --- 1. the light pass's own frames, from the caller's side ------------------------------
@pytest.mark.parametrize("name", ["mirror", "inside_a_sphere"])
def test_the_bounce_frame_again(pkg, oracle, name):
    """The hit pixels of the mirror scene as rays (p, R, skip = object):
    rt_cast_rays gives rt_reflect_hits' frame on them, and its triangles.  No
    two objects of the mirror scene intersect, so no bounce of it starts inside
    a sphere: the far roots come from the intersecting spheres of the reflect
    tests, in the same way."""
    if name == "mirror":
        scene = rr.mirror_scene(pkg)
        hits, r = rr.restated(oracle, "mirror", scene, rr.MIRROR_W, rr.MIRROR_H)
    else:
        scene = sr.intersecting_spheres(pkg, [(32, 24, 100, 1)])
        hits, r = rr.restated(oracle, "shadow_edge_p_inside_a_sphere", scene, 64, 48)
    rays, on = yr.bounce_rays(hits, r)
    if name == "mirror":
        assert rays.shape == (128 * 128,)  # the face fills the frame
        for kind, frame in r.kinds.items():
            assert (frame & on).sum() >= 100, kind
    else:
        assert (r.far_root & on & (r.bounce["object"] == 0)).sum() >= 100
    got, tri = pkg.cast_rays(rays, scene, triangles=True)
    assert same(got, pkg.reflect_hits(hits, scene)[on])
    assert same(got, r.bounce[on].astype(pkg.HIT_DTYPE)) and same(tri, r.tri2[on])
    if name == "mirror":
        assert set(np.unique(tri)) >= {-1, 0} and tri.max() <= 11


def test_the_shadow_mask_again(pkg, oracle):
    """The facing hit pixels of the kinds scene as segments (p, L, skip =
    object): rt_occlude_rays gives that light's bit of rt_shadow_hits."""
    scene = sr.kinds_scene(pkg, lights=(sr.KINDS_LIGHT, (-30, 64, 40, 1)))
    hits, r = lr.restated(sr.shadow_ref, oracle, "shadow_kinds", scene, sr.KINDS_W, sr.KINDS_H)
    mask = pkg.shadow_hits(hits, scene)
    nc, obj = scene.num_cubes, hits["object"]
    receivers = {"cube": (obj >= 0) & (obj < nc), "sphere": obj >= nc}
    seen = {(o, rcv, verdict): 0 for o in ("cube", "sphere") for rcv in receivers
            for verdict in (False, True)}
    for light in range(len(scene.lights)):
        rays, where = yr.facing_segments(oracle, scene, hits, light)
        assert np.array_equal(where, r.cast[light]) and where.sum() >= 1000
        got = pkg.occlude_rays(rays, scene)
        assert got.dtype == np.uint8 and set(np.unique(got)) == {0, 1}
        assert np.array_equal(got, ((mask[where] >> light) & 1).astype(np.uint8))
        assert np.array_equal(got, r.occluded[light][where].astype(np.uint8))
        for o, by in (("cube", r.by_cube[light]), ("sphere", r.by_sphere[light])):
            for rcv, at in receivers.items():
                seen[o, rcv, True] += int((where & at & by).sum())
                seen[o, rcv, False] += int((where & at & ~by).sum())
    assert min(seen.values()) >= 10, seen


def test_the_oracles_own_triangle_test(pkg, oracle):
    """(t, triangle) of a one-cube scene is the first minimum over the
    oracle's intersect_tri results with td > 0, taken in a Python loop."""
    scene = lr.one_cube(pkg, [("scale", 15, 12, 10), ("rotate", 0.3, 0.7, 0.1),
                              ("translate", 50, 40, -40)], (1, 1, 1, 255))
    rays = yr.random_rays(scene, 1200, 21, skips=[-1])
    got, tri = pkg.cast_rays(rays, scene, triangles=True)
    verts = scene.cube_vertices[0]
    want_t, want_tri = np.full(len(rays), K_FAR, F32), np.full(len(rays), -1, np.int32)
    for i, ray in enumerate(rays):
        o = [ray["ox"], ray["oy"], ray["oz"]]
        d = [ray["dx"], ray["dy"], ray["dz"]]
        for k in range(12):
            hit, td = oracle.intersect_tri(o, d, verts[3 * k, :3], verts[3 * k + 1, :3],
                                           verts[3 * k + 2, :3])
            if hit == 1 and td > 0.0 and F32(td) < want_t[i]:
                want_t[i], want_tri[i] = F32(td), k
    assert (want_tri >= 0).sum() >= 100 and (want_tri < 0).sum() >= 100
    assert np.array_equal(got["t"].view(np.uint32), want_t.view(np.uint32))
    assert np.array_equal(tri, want_tri)
    assert np.array_equal(got["object"], np.where(want_tri >= 0, 0, -1))


# --- 2. host = restatement ---------------------------------------------------------------
def scenes(pkg):
    base = lr.base(pkg)
    return {
        "base": base,
        "twins": rr.twin_cubes_scene(pkg),
        "sphere_tie": rr.sphere_tie_scene(pkg),
        "spheres_only": pkg.Scene(base.sphere_origins, base.sphere_radius, base.sphere_colours),
        "cubes_only": pkg.Scene(cube_vertices=base.cube_vertices, cube_colours=base.cube_colours),
        "empty": pkg.Scene(),
    }


@pytest.mark.parametrize("name", ["base", "twins", "sphere_tie", "spheres_only", "cubes_only",
                                  "empty"])
def test_random_rays(pkg, oracle, name):
    scene = scenes(pkg)[name]
    small = dict(box=((0, 64), (0, 48), (-70, 20)))  # the 64 x 48 scenes of the reflect tests
    rays = yr.random_rays(scene, 768, 31, **(dict(small, skips=[-1, 2]) if name == "twins" else
                                             small if name == "sphere_tie" else {}))
    if name == "sphere_tie":
        # the mirrored ray of TIE_PIXEL: the quadratic's s0 and a triangle's
        # (float)td are the same float; cubes come first, so the cube wins
        hits, r = rr.restated(oracle, "reflect_sphere_tie", scene, 64, 48)
        y, x = rr.TIE_PIXEL
        tie = yr.make_rays([a[y, x] for a in r.p], [a[y, x] for a in r.R], hits["object"][y, x])
        rays = np.concatenate([tie.reshape(1), rays])
        p, R = yr.origins(rays[:1]), yr.directions(rays[:1])
        tri = [rr.tri_sf(p, R, *scene.cube_vertices[0, 3 * k:3 * k + 3]) for k in range(12)]
        tri = [sf[0] for ok, sf in tri if ok[0]]
        ok, s0, far = rr.sphere_sf(p, R, scene.sphere_origins[0], scene.sphere_radius[0])
        assert ok[0] and not far[0] and min(tri).view(np.uint32) == s0[0].view(np.uint32)
    hits, tri, far, occ = compare(pkg, scene, rays, name)
    obj = hits["object"]
    if name == "empty":
        assert (obj == -1).all() and (hits["t"] == K_FAR).all() and not occ.any()
        # and with NULL arrays
        null, out = type(scene.as_c())(), np.zeros(len(rays), pkg.HIT_DTYPE)
        tri, flags = np.zeros(len(rays), np.int32), np.ones(len(rays), np.uint8)
        assert null.cube_vertices is None and null.sphere_origins is None and null.lights is None
        lib, p = pkg.library(), rays.astype(pkg.RAY_DTYPE)
        assert lib.rt_cast_rays(p.ctypes.data, len(p), ctypes.byref(null), out.ctypes.data,
                                tri.ctypes.data) == 0
        assert lib.rt_occlude_rays(p.ctypes.data, len(p), ctypes.byref(null),
                                   flags.ctypes.data) == 0
        assert same(out, hits.astype(pkg.HIT_DTYPE)) and (tri == -1).all() and not flags.any()
        return
    assert (obj >= 0).sum() >= 50 and (obj == -1).sum() >= 50 and (tri >= 0).sum() != len(rays)
    assert 10 <= occ.sum() <= len(rays) - 10
    if name == "base":
        assert len(np.unique(obj)) >= 20 and far.sum() >= 1
    if name == "twins":  # every candidate of cube 1 ties with cube 0's: the lower slot wins
        assert np.array_equal(scene.cube_vertices[0], scene.cube_vertices[1])
        assert (obj == 0).sum() >= 20 and not (obj == 1).any()
    if name == "sphere_tie":
        assert obj[0] == 0 and hits["t"][0] == s0[0]
    if name == "spheres_only":
        assert scene.num_cubes == 0 and (tri == -1).all()
    if name == "cubes_only":
        assert scene.num_spheres == 0 and ((tri >= 0) == (obj >= 0)).all()


@pytest.mark.parametrize("name", yr.EDGE_NAMES)
def test_edge_rays(pkg, name):
    scene = lr.base(pkg)
    cases = yr.edge_rays(scene)
    assert sorted(cases) == sorted(yr.EDGE_NAMES)
    rays = cases[name]
    hits, tri, far, occ = compare(pkg, scene, rays, name)
    yr.check_edge(name, scene, rays, hits, far, occ.astype(bool))


# --- 3. the camera ----------------------------------------------------------------------
W, H, BAND = 37, 29, (5, 17)


@pytest.mark.parametrize("normalise", [0, 1])
@pytest.mark.parametrize("rows", [None, BAND], ids=["frame", "band"])
def test_camera_rays(pkg, normalise, rows):
    cam = pkg.Camera(**yr.generic_camera(normalise))
    want = yr.camera(cam, W, rows or (0, H))
    got = pkg.camera_rays(cam, W, H, rows)
    assert got.dtype == pkg.RAY_DTYPE and got.shape == want.shape
    assert same(got, want.astype(pkg.RAY_DTYPE))
    assert (got["skip"] == -1).all() and (words(got)[..., 7] == 0).all()
    length = np.sqrt(sum(got[f].astype(np.float64) ** 2 for f in ("dx", "dy", "dz")))
    assert (np.abs(length - 1) < 1e-6).all() if normalise else \
        (np.abs(length - 1) > 1e-3).mean() > 0.9
    if rows:  # a band is a slice of the frame
        assert same(got, pkg.camera_rays(cam, W, H)[rows[0]:rows[1]])


@pytest.mark.parametrize("normalise", [0, 1])
@pytest.mark.parametrize("rows", [None, BAND], ids=["frame", "band"])
def test_cast_camera_is_cast_rays_on_camera_rays(pkg, normalise, rows):
    scene = lr.base(pkg)
    spec = dict(yr.generic_camera(normalise), o0=(30.0, 20.0, 40.0), ou=(1.0, 0.125, -0.5))
    cam = pkg.Camera(**spec)
    rays = pkg.camera_rays(cam, W, H, rows)
    want, want_tri = pkg.cast_rays(rays, scene, triangles=True)
    assert (want["object"] >= 0).sum() >= 100 and (want["object"] == -1).sum() >= 20
    got, tri = pkg.cast_camera(cam, scene, W, H, rows, triangles=True)
    assert same(got, want) and same(tri, want_tri)
    assert same(pkg.cast_camera(cam, scene, W, H, rows), want)
    hits, ref_tri, _ = yr.cast(scene, yr.camera(cam, W, rows or (0, H)))
    assert same(got, hits.astype(pkg.HIT_DTYPE)) and same(tri, ref_tri)


@pytest.mark.parametrize("d", [REF_DIR, (0.3, -0.2, -1.0, -1.0), (0.0, 0.5, -1e-4, 7.0)])
def test_reference_camera(pkg, d):
    cam = pkg.Camera.reference(d)
    assert cam.normalise == 0
    rays = pkg.camera_rays(cam, W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    want = yr.make_rays((xs, ys, 0.0), d[:3], -1)
    assert same(rays, want.astype(pkg.RAY_DTYPE))
    assert np.array_equal(pkg.Camera.reference().d0, pkg.primary_ray_dir()[:3])


def test_pinhole_camera(pkg):
    """The centre pixel of an odd-sized frame looks along the view; a corner
    pixel's centre is where the field of view puts it."""
    eye, target, up = np.array([10.0, -4.0, 25.0]), np.array([-3.0, 8.0, -40.0]), (0.2, 1.0, 0.1)
    w, h, fov = 41, 31, 50.0
    cam = pkg.Camera.pinhole(eye, target, up, fov, w, h)
    assert cam.normalise == 1 and np.array_equal(cam.o0, eye.astype(F32))
    assert not cam.ou.any() and not cam.ov.any()
    rays = pkg.camera_rays(cam, w, h)
    dirs = np.stack([rays[f] for f in ("dx", "dy", "dz")], -1).astype(np.float64)
    view = (target - eye) / np.linalg.norm(target - eye)
    # a dozen float32 roundings of 6e-8 each
    assert dirs[h // 2, w // 2] @ view >= 1 - 1e-6
    th = math.tan(math.radians(fov) / 2)
    sx, sy = (1 - 1 / w) * th * w / h, (1 - 1 / h) * th  # the corner pixel's centre
    half_diagonal = math.atan(math.hypot(sx, sy))
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        assert abs(math.acos(dirs[y, x] @ view) - half_diagonal) <= 1e-5
    # row 0 is towards `up`, x grows along view x up
    right = np.cross(view, up)
    assert dirs[0, w // 2] @ np.array(up) > dirs[h - 1, w // 2] @ np.array(up)
    assert dirs[h // 2, w - 1] @ right > dirs[h // 2, 0] @ right
    for bad in (dict(fov_y=0.0), dict(fov_y=180.0), dict(fov_y=float("nan")), dict(width=0),
                dict(height=0), dict(target=eye), dict(up=(0, 0, 0)), dict(up=target - eye),
                dict(eye=(np.inf, 0, 0)), dict(up=(0, np.nan, 0))):
        kw = dict(dict(eye=eye, target=target, up=up, fov_y=fov, width=w, height=h), **bad)
        lc.refused(pkg, lambda: pkg.Camera.pinhole(**kw))
    c = pkg.Camera().as_c()
    v = np.zeros(3, F32)
    assert pkg.library().rt_camera_pinhole(None, v.ctypes.data, v.ctypes.data, 50.0, 4, 4,
                                           ctypes.byref(c)) == pkg.RT_ERR_INVALID_ARG
    assert pkg.library().rt_camera_reference(None, ctypes.byref(c)) == pkg.RT_ERR_INVALID_ARG
    assert pkg.library().rt_camera_reference(v.ctypes.data, None) == pkg.RT_ERR_INVALID_ARG


def test_a_sphere_in_front_of_a_pinhole_is_a_disc(pkg):
    """A sphere of radius R at distance D on the camera's axis projects to a
    circle of tangent sqrt(R^2 / (D^2 - R^2)): rho pixels.  The unit squares
    about the pixel centres inside a circle cover the disc of radius
    rho - sqrt(1/2) and lie inside the disc of radius rho + sqrt(1/2), so the
    count is within one pixel's rim of the projected area."""
    R, D, w, h, fov = 10.0, 60.0, 101, 81, 40.0
    scene = lr.one_sphere(pkg, (5, 7, -20, 1), R, (1, 1, 1, 255))
    cam = pkg.Camera.pinhole((5, 7, -20 + D), (5, 7, -20), (0, -1, 0), fov, w, h)
    got = pkg.cast_camera(cam, scene, w, h)
    rho = math.sqrt(R * R / (D * D - R * R)) / math.tan(math.radians(fov) / 2) * h / 2
    n = int((got["object"] == 0).sum())
    assert rho > 10
    assert math.pi * (rho - math.sqrt(0.5)) ** 2 <= n <= math.pi * (rho + math.sqrt(0.5)) ** 2
    ys, xs = np.nonzero(got["object"] == 0)
    assert abs(xs.mean() - (w - 1) / 2) < 0.01 and abs(ys.mean() - (h - 1) / 2) < 0.01
    # unit directions: the parameter is the distance, D - R at the centre
    assert abs(got["t"][h // 2, w // 2] - (D - R)) < 1e-3


# --- 4. the argument contract -----------------------------------------------------------
MAX_RAYS = (2**31 - 1) * 256  # one launch's grid


class Args:
    """Valid arguments of the four host entry points on the base scene, and
    the calls (ctx = None: host; else the device entry point behind `ctx`)."""

    def __init__(self, pkg):
        self.pkg, self.lib = pkg, pkg.library()
        self.scene = lr.base(pkg)
        self.sc = self.scene.as_c()
        self.rays = yr.random_rays(self.scene, 8, 3).astype(pkg.RAY_DTYPE)
        self.hits = np.zeros(64, pkg.HIT_DTYPE)
        self.tri = np.zeros(64, np.int32)
        self.occ = np.zeros(64, np.uint8)
        self.out_rays = np.zeros(64, pkg.RAY_DTYPE)
        self.cam = pkg.Camera.reference().as_c()
        for a in (self.rays, self.hits, self.tri, self.out_rays):
            assert a.ctypes.data % 16 == 0
        p = lambda a: a.ctypes.data  # noqa: E731
        self.good = {
            "cast": dict(rays=p(self.rays), n=8, scene=ctypes.byref(self.sc), hits=p(self.hits),
                         tri=p(self.tri)),
            "occlude": dict(rays=p(self.rays), n=8, scene=ctypes.byref(self.sc),
                            occ=p(self.occ)),
            "camera": dict(cam=ctypes.byref(self.cam), width=4, rb=1, re=3,
                           out_rays=p(self.out_rays)),
            "cast_camera": dict(cam=ctypes.byref(self.cam), scene=ctypes.byref(self.sc), width=4,
                                rb=1, re=3, hits=p(self.hits), tri=p(self.tri)),
        }
        self.symbols = {"cast": "rt_cast_rays", "occlude": "rt_occlude_rays",
                        "camera": "rt_camera_rays", "cast_camera": "rt_cast_camera"}

    def call(self, name, ctx=None, **kw):
        a = list(dict(self.good[name], **kw).values())
        if ctx is None:
            return getattr(self.lib, self.symbols[name])(*a)
        return getattr(self.lib, self.symbols[name] + "_device")(ctx, *a, None)


# what each entry point refuses: (argument, value)
def refusals(a, name):
    good = a.good[name]
    bad = [(k, None) for k in good if k in ("rays", "scene", "hits", "occ", "cam", "out_rays")]
    bad += [(k, good[k] + off) for k, off in (("rays", 8), ("rays", 4), ("hits", 4), ("tri", 2),
                                              ("out_rays", 8), ("out_rays", 16 + 4))
            if k in good]
    if "n" in good:
        bad += [("n", -1), ("n", -2**63)]
    if "scene" in good:
        for fields in lc.BAD_SCENES:
            c = a.scene.as_c()
            for field, value in fields.items():
                setattr(c, field, value)
            bad.append(("scene", ctypes.byref(c)))
    if "cam" in good:
        for normalise in (2, -1, 256):
            c = a.pkg.Camera.reference().as_c()
            c.normalise = normalise
            bad.append(("cam", ctypes.byref(c)))
    return bad


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_bad_arguments_are_refused(pkg, device):
    """Every NULL, every misalignment, n < 0, a bad scene, normalise other
    than 0 or 1 and a bad band; the device entry points refuse the same
    before any HIP call (behind a context that is never used), and a NULL
    context."""
    a = Args(pkg)
    ctx = ctypes.c_void_p(a.hits.ctypes.data) if device else None
    bad = pkg.RT_ERR_INVALID_ARG
    for name in a.good:
        if device:
            fn = getattr(a.lib, a.symbols[name] + "_device")
            assert fn(None, *a.good[name].values(), None) == bad, name
        else:
            assert a.call(name) == 0, name
            assert a.call(name, **({"tri": None} if "tri" in a.good[name] else {})) == 0, name
        for key, value in refusals(a, name):
            assert a.call(name, ctx, **{key: value}) == bad, (name, key, value)
        if "width" in a.good[name]:
            for width, rb, re in lc.SHAPES:
                assert a.call(name, ctx, width=width, rb=rb, re=re) == bad, (name, width, rb, re)
            if not device:
                assert a.call(name, rb=1 << 20, re=(1 << 20) + 2) == 0
            # 2^48 pixels: more than one launch
            assert a.call(name, ctx, width=1 << 24, rb=0, re=1 << 24) == pkg.RT_ERR_UNSUPPORTED
        else:
            # (refused before a ray is read)
            assert a.call(name, ctx, n=MAX_RAYS + 1) == pkg.RT_ERR_UNSUPPORTED
            assert a.call(name, ctx, n=2**40) == pkg.RT_ERR_UNSUPPORTED
        # byte outputs have no alignment
        if name == "occlude" and not device:
            assert a.call(name, occ=a.occ.ctypes.data + 1) == 0


def test_no_rays_is_ok_and_writes_nothing(pkg):
    a = Args(pkg)
    a.hits["t"], a.hits["object"], a.tri[:], a.occ[:] = 7.0, 7, 7, 7
    assert a.call("cast", n=0) == 0 and a.call("occlude", n=0) == 0
    assert (a.hits["object"] == 7).all() and (a.tri == 7).all() and (a.occ == 7).all()
    empty = np.zeros((0, 5), pkg.RAY_DTYPE)
    assert pkg.cast_rays(empty, a.scene).shape == (0, 5)
    assert pkg.occlude_rays(empty, a.scene).shape == (0, 5)


def test_skip_out_of_range_is_refused(pkg):
    a = Args(pkg)
    n = yr.slots(a.scene)
    assert n == 50
    for ok in (-1, 0, n - 1):
        rays = a.rays.copy()
        rays["skip"][5] = ok
        assert pkg.cast_rays(rays, a.scene).shape == (8,)
        assert pkg.occlude_rays(rays, a.scene).shape == (8,)
    for bad in (-2, n, yr.I32_MIN, yr.I32_MAX):
        rays = a.rays.copy()
        rays["skip"][5] = bad
        lc.refused(pkg, lambda: pkg.cast_rays(rays, a.scene))
        lc.refused(pkg, lambda: pkg.cast_rays(rays, a.scene, triangles=True))
        lc.refused(pkg, lambda: pkg.occlude_rays(rays, a.scene))
    # on the empty scene every slot is out of range
    rays = a.rays.copy()
    rays["skip"] = 0
    lc.refused(pkg, lambda: pkg.cast_rays(rays, pkg.Scene()))


def test_python_names(pkg):
    lib = pkg.library()
    for symbol in ("rt_cast_rays", "rt_occlude_rays", "rt_camera_rays", "rt_cast_camera",
                   "rt_camera_pinhole", "rt_camera_reference"):
        assert symbol in pkg.EXPORTED_SYMBOLS and hasattr(lib, symbol)
        if symbol.endswith(("rays", "cast_camera")):
            assert symbol + "_device" in pkg.EXPORTED_SYMBOLS and hasattr(lib, symbol + "_device")
    assert pkg.RAY_DTYPE.itemsize == 32 and pkg.RAY_DTYPE == yr.ray_dtype()
    assert ctypes.sizeof(pkg.Camera().as_c()) == 76
    params = {
        (pkg, "cast_rays"): ["rays", "scene", "triangles"],
        (pkg, "occlude_rays"): ["rays", "scene"],
        (pkg, "camera_rays"): ["camera", "width", "height", "rows"],
        (pkg, "cast_camera"): ["camera", "scene", "width", "height", "rows", "triangles"],
        (pkg.Camera, "pinhole"): ["eye", "target", "up", "fov_y", "width", "height"],
        (pkg.Camera, "reference"): ["ray_dir"],
        (pkg.RayTracer, "cast_rays_device"): ["self", "rays_ptr", "n", "device_scene", "hits_ptr",
                                              "triangles_ptr", "stream"],
        (pkg.RayTracer, "occlude_rays_device"): ["self", "rays_ptr", "n", "device_scene",
                                                 "out_ptr", "stream"],
        (pkg.RayTracer, "camera_rays_device"): ["self", "camera", "width", "rows", "out_ptr",
                                                "stream"],
        (pkg.RayTracer, "cast_camera_device"): ["self", "camera", "device_scene", "width", "rows",
                                                "hits_ptr", "triangles_ptr", "stream"],
    }
    for (owner, name), want in params.items():
        if owner is pkg:
            assert name in pkg.__all__
        assert list(inspect.signature(getattr(owner, name)).parameters) == want, name
    assert "RAY_DTYPE" in pkg.__all__ and "Camera" in pkg.__all__
    with pytest.raises(ValueError):
        pkg.cast_rays(np.zeros(4, pkg.HIT_DTYPE), pkg.Scene())
    assert lib.rt_abi_version() == 1


# --- 5. under the sanitizers ------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_rays_arguments_under_sanitizers(tmp_path):
    """tests/rays_args_check.cpp: exactly-sized heap arrays, n = 0, 1 and 257,
    NULL out_triangle, a scene of all NULLs, the refusals."""
    lc.run_args_check(tmp_path, "rays")
