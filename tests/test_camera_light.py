"""rt_light_camera / rt_bounce_camera without a GPU: the
light pass of a camera view.

The host functions against the numpy restatement (tests/camera_light_ref.py:
level 0 from rays_ref's camera and cast, then mirror_ref's chain machinery),
as raw 32-bit words; the identities that tie the new calls to rt_cast_camera,
rt_shade_hits, rt_light_hits_mirrored and rt_bounce_hits; culled = unculled;
what every frame holds, proved on the restatement; the edge cameras; and the
argument contract, host and device (the device entry points refuse before any
HIP call, so without a GPU).
"""
import ctypes
import inspect
import shutil
import subprocess

import numpy as np
import pytest

import camera_light_ref as cr
import light_contract as lc
import light_ref as lr
import mirror_ref as mr
import rays_ref as yr
from gpu_support import H, W
from light_ref import eq

F32 = np.float32
UP = (0, -1, 0)
BAND = (30, 50)  # of an H-row frame; scaled to the case's height


def many(pkg):
    """70 cubes and 70 spheres under three lights (tests/test_light_accel.py's)."""
    return lr.with_lights(pkg.Scene.synthetic(W, H, 70, 70, seed=13, k=0.3), lr.THREE_LIGHTS)


def odd(pkg, scene):
    """`scene` with a NaN coordinate in cube 1 and an infinite one in cube 2:
    their records are always kept."""
    v = scene.cube_vertices.copy().reshape(-1, 36, 4)
    v[1, 7, 1], v[2, 35, 2] = np.nan, -np.inf
    return pkg.Scene(scene.sphere_origins, scene.sphere_radius, scene.sphere_colours,
                     v.reshape(scene.cube_vertices.shape), scene.cube_colours, scene.lights)


# name: (scene, camera, width, height, reflectivity).  The eyes and targets are
# chosen so that the restatement alone holds what KINDS says (test 3).
def cases(pkg):
    big = many(pkg)
    ref = lr.with_lights(pkg.Scene.reference(2), [(300, 200, 300, 1), (0, 0, 50, 1)])
    chain, corridor, wave = mr.chain_scene(pkg), mr.corridor_scene(pkg), mr.wave_scene(pkg)
    pin = pkg.Camera.pinhole
    generic = lambda n: pkg.Camera(**dict(yr.generic_camera(n), o0=(30.0, 20.0, 40.0)))  # noqa: E731
    return {
        "chain_pinhole": (chain, pin((150, 20, 60), (80, 80, -45), UP, 60.0, 96, 96), 96, 96,
                          mr.CHAIN_REFLECTIVITY),
        # the eye inside sphere 5 ((100, 104, -34), r = 10, a mirror): its far
        # root is every pixel's level 0, and the bounce from there leaves it out
        "chain_inside": (chain, pin((101, 103, -33), (121, 125, -3), UP, 140.0, 64, 64), 64, 64,
                         mr.CHAIN_REFLECTIVITY),
        "corridor_pinhole": (corridor, pin((32, 24, 40), (32.5, 24, -100), UP, 30.0, 64, 48), 64,
                             48, mr.CORRIDOR_REFLECTIVITY),
        # (the lower rows look away from the face, z upwards)
        "wave_generic1": (wave, pkg.Camera(**dict(yr.generic_camera(1), o0=(70.0, 30.0, 40.0),
                                                  dv=(-0.0015, 0.02, 0.04))),
                          64, 64, mr.WAVE_REFLECTIVITY),
        "many_pinhole": (big, pin((30, 20, 90), (32, 24, -40), UP, 50.0, W, H), W, H,
                         mr.mixed(big)),
        "many_generic0": (big, generic(0), W, H, mr.mixed(big)),
        "reference_pinhole": (ref, pin((320, 240, 500), (320, 240, -100), UP, 60.0, 80, 60), 80, 60,
                              mr.mixed(ref)),
    }


CASES = ["chain_pinhole", "chain_inside", "corridor_pinhole", "wave_generic1", "many_pinhole",
         "many_generic0", "reference_pinhole"]
# What a case's frame need not hold, and why; every other kind of KINDS it must.
EXEMPT = {
    # two cubes, both perfect mirrors: no sphere, no matte end
    "corridor_pinhole": {"sphere0", "ends_matte"},
    # from inside a sphere every ray meets that sphere
    "chain_inside": {"miss0", "cube0"},
    # two cubes, one a face far wider than the view: most rays keep it
    "wave_generic1": {"culls"},
}
KINDS = ("miss0", "cube0", "sphere0", "hidden", "reached", "ends_matte", "ends_depth", "ends_miss",
         "level2", "culls")


def chain_of(pkg, name, rows=None):
    scene, cam, w, h, refl = cases(pkg)[name]
    return cr.restated((name, rows), scene, cam, w, rows or (0, h))


# --- 1. the restatement = the host ---------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_host(pkg, oracle, name):
    scene, cam, w, h, refl = cases(pkg)[name]
    c = chain_of(pkg, name)
    n = 0
    for label, got in cr.host_frames(pkg, cam, scene, w, h, refl):
        want = cr.want_frame(c, oracle, label, refl)
        assert got.dtype == want.dtype and not eq(got, want), f"{name} {label}: {eq(got, want)}"
        n += 1
    assert n == 4 + 4 * 2 * 2
    rows = (BAND[0] * h // H, BAND[1] * h // H)
    band = chain_of(pkg, name, rows)
    for label, got in cr.host_frames(pkg, cam, scene, w, h, refl, rows=rows, depths=(2,),
                                     bounces=(2,)):
        want = cr.want_frame(band, oracle, label, refl)
        assert not eq(got, want), f"{name} band {label}: {eq(got, want)}"
        # a band is a slice of the frame
        whole = cr.want_frame(c, oracle, label, refl)[rows[0]:rows[1]]
        assert not eq(got, whole), f"{name} band {label} of the frame"


# --- 2. identities ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain_pinhole", "many_generic0"])
def test_level_0_is_the_cast_and_the_shade(pkg, name):
    scene, cam, w, h, refl = cases(pkg)[name]
    cast = pkg.cast_camera(cam, scene, w, h)
    assert not eq(pkg.bounce_camera(cam, scene, w, h, 0), cast)
    dark = lr.with_lights(scene, [])
    for fmt in cr.LIT_FORMATS:
        assert not eq(pkg.light_camera(cam, dark, w, h, refl, 0, False, fmt),
                      pkg.shade_hits(cast, dark, fmt))
        assert not eq(pkg.light_camera(cam, dark, w, h, None, 0, True, fmt),
                      pkg.shade_hits(cast, dark, fmt))


@pytest.mark.parametrize("scene_name", ["chain", "many"])
@pytest.mark.parametrize("d", [(0.0, 0.0, -1.0, -1.0), (0.3, -0.2, -1.0, -1.0)],
                         ids=["reference", "oblique"])
def test_reference_camera_is_the_deferred_pass(pkg, scene_name, d):
    """Camera.reference(d), no -0 component in d: the new calls are
    light_hits_mirrored / bounce_hits on cast_camera's frame, word for word."""
    if scene_name == "chain":
        scene, w, h, refl = mr.chain_scene(pkg), mr.CHAIN_W, mr.CHAIN_H, mr.CHAIN_REFLECTIVITY
    else:
        scene, w, h = many(pkg), W, H
        refl = mr.mixed(scene)
    cam = pkg.Camera.reference(np.array(d, F32))
    assert not np.signbit(np.array(d[:3], F32)[np.array(d[:3], F32) == 0]).any()
    hits = pkg.cast_camera(cam, scene, w, h)
    assert (hits["object"] >= 0).sum() >= 500
    for depth in cr.DEPTHS:
        for shadows in (False, True):
            for fmt in cr.LIT_FORMATS:
                got = pkg.light_camera(cam, scene, w, h, refl, depth, shadows, fmt)
                want = pkg.light_hits_mirrored(hits, scene, refl, depth, fmt, shadows, ray_dir=d)
                assert not eq(got, want), f"depth={depth} shadows={shadows} {fmt}: {eq(got, want)}"
    for b in (1, 2, 8):
        got = pkg.bounce_camera(cam, scene, w, h, b)
        assert not eq(got, pkg.bounce_hits(hits, scene, b, ray_dir=d)), b


@pytest.mark.parametrize("name", CASES)
def test_culled_equals_unculled(pkg, name):
    scene, cam, w, h, refl = cases(pkg)[name]
    accel = pkg.build_accel(scene)
    plain = dict(cr.host_frames(pkg, cam, scene, w, h, refl))
    for label, got in cr.host_frames(pkg, cam, scene, w, h, refl, accel=accel):
        assert not eq(got, plain[label]), f"{name} {label}: {eq(got, plain[label])}"
    rows = (BAND[0] * h // H, BAND[1] * h // H)
    for label, got in cr.host_frames(pkg, cam, scene, w, h, refl, rows=rows, accel=accel,
                                     depths=(2,), bounces=(2,)):
        assert not eq(got, plain[label][rows[0]:rows[1]]), f"{name} band {label}"


def test_always_kept_records_among_culling_ones(pkg):
    good, cam, w, h, refl = cases(pkg)["many_pinhole"]
    scene = odd(pkg, good)
    accel = pkg.build_accel(scene)
    assert (accel["emax2"][1:3] == np.inf).all() and np.isfinite(accel["emax2"][[0, 3]]).all()
    kept = pkg.accel_kept(pkg.camera_rays(cam, w, h), scene, accel)
    assert (kept >= 2).all() and kept.mean() < scene.num_cubes / 2
    plain = dict(cr.host_frames(pkg, cam, scene, w, h, refl, depths=(0, 2), bounces=(0, 2)))
    for label, got in cr.host_frames(pkg, cam, scene, w, h, refl, accel=accel, depths=(0, 2),
                                     bounces=(0, 2)):
        assert not eq(got, plain[label]), f"{label}: {eq(got, plain[label])}"


@pytest.mark.parametrize("name", ["no_cubes", "empty", "no_lights", "33_lights"])
def test_degenerate_scenes(pkg, oracle, name):
    big, cam, w, h, _ = cases(pkg)["many_pinhole"]
    w, h = 48, 40
    cam = pkg.Camera.pinhole((30, 20, 90), (32, 24, -40), UP, 50.0, w, h)
    scene = {"no_cubes": pkg.Scene(big.sphere_origins, big.sphere_radius, big.sphere_colours,
                                   lights=big.lights),
             "empty": lr.with_lights(pkg.Scene(), lr.ONE_LIGHT),
             "no_lights": lr.with_lights(big, []),
             "33_lights": lr.with_lights(big, [(3 * i, 5, 60, 1) for i in range(33)])}[name]
    refl = mr.mixed(scene) if yr.slots(scene) else None
    accel = pkg.build_accel(scene)
    c = cr.camera_chain(scene, cam, w, (0, h), depth=2)
    for a in (None, accel):
        for label, got in cr.host_frames(pkg, cam, scene, w, h, refl, accel=a, depths=(0, 2),
                                         bounces=(0, 2)):
            want = cr.want_frame(c, oracle, label, refl)
            assert not eq(got, want), f"{name} {label}: {eq(got, want)}"
    if name == "empty":
        assert (pkg.light_camera(cam, scene, w, h, None, 8, True) == (0, 0, 0, 255)).all()
        assert (pkg.bounce_camera(cam, scene, w, h, 8)["object"] == -1).all()
    else:
        assert (c.levels[0].obj >= 0).sum() >= 100


# --- 3. not vacuous --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_not_vacuous(pkg, name):
    """Every frame of test 1 holds every kind of pixel the level loop tells
    apart (but what EXEMPT names, with the reason), on the restatement alone."""
    scene, cam, w, h, refl = cases(pkg)[name]
    c = chain_of(pkg, name)
    held = cr.kinds(c, refl)
    if scene.num_cubes:
        kept = pkg.accel_kept(c.rays, scene, pkg.build_accel(scene))
        assert not eq(c.rays.astype(pkg.RAY_DTYPE), pkg.camera_rays(cam, w, h))
        held["culls"] = int(kept.mean() < scene.num_cubes / 2)
    for kind in KINDS:
        if kind not in EXEMPT.get(name, ()):
            assert held.get(kind, 0) >= 1, (name, kind, held)
    if name == "corridor_pinhole":
        assert held["level8"] >= 64 and (c.levels[8].T[c.levels[8].obj >= 0] > 180).all()
    if name == "chain_inside":
        # the eye is inside sphere 5: every pixel's level 0 is its far root
        assert held["far_root0"] == w * h
        assert (c.levels[0].obj == scene.num_cubes + 5).all()


# --- 4. edge cameras -------------------------------------------------------------------------------
def edge_cameras(pkg):
    """name -> (camera, what the restatement's cast must hold).  On the base
    scene under three lights, 37 x 29."""
    g = yr.generic_camera(1)
    inf = np.inf
    return {
        # (d0 + x * du) + y * dv is exactly 0 at pixel (4, 2) (dyadic numbers):
        # normalised, NaN; right of it the rays look down the z axis
        "zero_direction": pkg.Camera(o0=(30, 20, 40), ou=(1, 0, 0), ov=(0, 1, 0),
                                     d0=(-1.0, -0.5, 2.03125), du=(0.25, 0, -0.5),
                                     dv=(0, 0.25, -0.015625), normalise=1),
        # one direction for every pixel, origins on a plane
        "du_dv_zero": pkg.Camera(o0=(0, 0, 40), ou=(1.5, 0, 0), ov=(0, 1.5, 0),
                                 d0=(0.05, -0.05, -1.0), normalise=1),
        # a parameter past 300000 is a miss, so the direction is 10 long: t near 1e5
        "origin_1e6": pkg.Camera(o0=(0, 0, 1e6), ou=(2.5, 0, 0), ov=(0, 2.5, 0),
                                 d0=(0.0001, -0.0001, -10.0), du=(1e-6, 0, 0), dv=(0, 1e-6, 0)),
        # dy: 0 * inf = NaN in column 0, inf elsewhere, which normalises to NaN
        "inf_component": pkg.Camera(**dict(g, o0=(30.0, 20.0, 40.0), du=(0.02, inf, 0.0005))),
    }


EDGE_W, EDGE_H = 37, 29


def edge_scene(pkg):
    return lr.with_lights(lr.base(pkg), lr.THREE_LIGHTS)


def check_edge_camera(name, c):
    """The restatement holds what the case is there for."""
    obj = c.levels[0].obj
    d = np.stack(yr.directions(c.rays))
    if name == "zero_direction":
        assert np.isnan(d[:, 2, 4]).all() and np.isnan(d).any(0).sum() == 1
        assert obj[2, 4] == -1 and (obj >= 0).sum() >= 20
    elif name == "du_dv_zero":
        assert all(len(np.unique(a)) == 1 for a in d) and (obj >= 0).sum() >= 100
    elif name == "origin_1e6":
        assert (np.stack(yr.origins(c.rays))[2] > 9e5).all() and (obj >= 0).sum() >= 20
    elif name == "inf_component":
        assert np.isnan(d[1]).all() and (obj == -1).all()
        assert (c.levels[0].best == 300000.0).all()  # and no NaN in a word
    else:
        raise AssertionError(name)


EDGE_CAMERAS = ["zero_direction", "du_dv_zero", "origin_1e6", "inf_component"]


@pytest.mark.parametrize("name", EDGE_CAMERAS)
def test_edge_cameras(pkg, oracle, name):
    scene, cam = edge_scene(pkg), edge_cameras(pkg)[name]
    refl = mr.mixed(scene)
    c = cr.restated(("edge", name), scene, cam, EDGE_W, (0, EDGE_H))
    check_edge_camera(name, c)
    accel = pkg.build_accel(scene)
    for a in (None, accel):
        for label, got in cr.host_frames(pkg, cam, scene, EDGE_W, EDGE_H, refl, accel=a,
                                         depths=(0, 2, 8), bounces=(0, 1, 8)):
            want = cr.want_frame(c, oracle, label, refl)
            assert not eq(got, want), f"{name} {label}: {eq(got, want)}"


# --- 5. the argument contract ----------------------------------------------------------------------
SYMBOLS = ("rt_light_camera", "rt_bounce_camera")


class Args:
    """Valid C arguments of the two calls on a 5 x 4 frame over the base scene
    under one light; call(symbol, ctx, **replaced)."""

    def __init__(self, pkg, scene=None):
        self.pkg, self.lib = pkg, pkg.library()
        self.scene = lr.with_lights(lr.base(pkg), lr.ONE_LIGHT) if scene is None else scene
        self.sc = self.scene.as_c()
        self.cam = pkg.Camera.pinhole((30, 20, 90), (32, 24, -40), UP, 50.0, 5, 4).as_c()
        self.accel = pkg.build_accel(self.scene)
        self.refl = np.full(max(1, yr.slots(self.scene)), 0.5, F32)
        self.out = np.zeros((4, 5, 4), np.int32)
        p = lambda a: a.ctypes.data  # noqa: E731
        assert p(self.out) % 16 == 0 and (not self.scene.num_cubes or p(self.accel) % 16 == 0)
        self.good = dict(cam=ctypes.byref(self.cam), scene=ctypes.byref(self.sc),
                         accel=p(self.accel) if self.scene.num_cubes else None, width=5, rb=0,
                         re=4, bounce=2, refl=p(self.refl), depth=2, shadows=1, fmt=0,
                         out=p(self.out))

    def call(self, symbol, ctx=None, **kw):
        a = dict(self.good, **kw)
        args = [a[k] for k in ("cam", "scene", "accel", "width", "rb", "re")]
        if "bounce" in symbol:
            args.append(a["bounce"])
        else:
            args += [a["refl"], a["depth"], a["shadows"], a["fmt"]]
        args.append(a["out"])
        if ctx is not None:
            return getattr(self.lib, symbol + "_device")(ctx, *args, None)
        return getattr(self.lib, symbol)(*args)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_bad_arguments_are_refused(pkg, device):
    """Every refusal of the contract; the device entry points behind a context
    that is never used: before any HIP call, so without a GPU."""
    a = Args(pkg)
    bad, p = pkg.RT_ERR_INVALID_ARG, a.good["accel"]
    ctx = ctypes.c_void_p(a.out.ctypes.data) if device else None
    for symbol in SYMBOLS:
        if not device:
            assert a.call(symbol) == 0, symbol
            assert a.call(symbol, accel=None) == 0, symbol  # unculled
        for value in (p + 8, p + 4):
            assert a.call(symbol, ctx, accel=value) == bad, (symbol, value)
        for key in ("cam", "scene", "out"):
            assert a.call(symbol, ctx, **{key: None}) == bad, (symbol, key)
        for width, rb, re in lc.SHAPES:
            assert a.call(symbol, ctx, width=width, rb=rb, re=re) == bad, (symbol, width, rb, re)
        for fields in lc.BAD_SCENES:
            c = a.scene.as_c()
            for field, value in fields.items():
                setattr(c, field, value)
            assert a.call(symbol, ctx, scene=ctypes.byref(c)) == bad, (symbol, fields)
        for normalise in (2, -1):
            cam = pkg.Camera(normalise=0).as_c()
            cam.normalise = normalise
            assert a.call(symbol, ctx, cam=ctypes.byref(cam)) == bad, (symbol, normalise)
    for b in (9, -1):
        assert a.call(SYMBOLS[1], ctx, bounce=b) == bad, b
    assert a.call(SYMBOLS[1], ctx, out=a.good["out"] + 4) == bad  # rt_hit: 8 bytes
    lit = SYMBOLS[0]
    for kw in (dict(depth=9), dict(depth=-1), dict(shadows=2), dict(shadows=-1), dict(fmt=2),
               dict(fmt=3), dict(fmt=-1), dict(refl=None), dict(out=a.good["out"] + 8),
               dict(fmt=1, out=a.good["out"] + 2)):
        assert a.call(lit, ctx, **kw) == bad, kw
    if device:
        assert a.call(lit, ctx, refl=a.good["refl"] + 2) == bad
        for symbol in SYMBOLS:
            assert a.call(symbol, ctypes.c_void_p(None)) == bad, symbol  # a NULL context
    else:
        assert a.call(lit, refl=None, depth=0) == 0
        assert a.call(lit, fmt=1, out=a.good["out"] + 4) == 0
        assert a.call(SYMBOLS[1], bounce=0) == 0 and a.call(SYMBOLS[1], bounce=8) == 0
        for r in (1.5, -0.25, np.nan):
            a.refl[3] = r
            assert a.call(lit) == bad, r
            assert a.call(lit, depth=0) == bad, r  # refused whatever the depth
        a.refl[3] = 0.5
    # 33 lights are served: only masks refuse that many
    a33 = Args(pkg, lr.with_lights(lr.base(pkg), [(i, 5, 60, 1) for i in range(33)]))
    if not device:
        assert a33.call(SYMBOLS[0]) == 0 and a33.call(SYMBOLS[1]) == 0
    # no objects: a NULL reflectivity at any depth; no cubes: nothing to align
    for scene in (lr.with_lights(pkg.Scene(), lr.ONE_LIGHT), pkg.Scene()):
        n = Args(pkg, scene)
        assert n.good["accel"] is None
        if not device:
            assert n.call(lit, refl=None, depth=8) == 0 and n.call(SYMBOLS[1]) == 0


def test_python_names(pkg):
    lib = pkg.library()
    header = (lc.REPO / "include" / "rt_hip.h").read_text()
    for symbol in SYMBOLS:
        for s in (symbol, symbol + "_device"):
            assert s in pkg.EXPORTED_SYMBOLS and hasattr(lib, s) and f"int {s}(" in header
    assert lib.rt_abi_version() == 1
    params = {
        (pkg, "light_camera"): ["camera", "scene", "width", "height", "reflectivity", "max_bounces",
                                "shadows", "fmt", "rows", "accel"],
        (pkg, "bounce_camera"): ["camera", "scene", "width", "height", "bounce", "rows", "accel"],
        (pkg.RayTracer, "light_camera_device"): ["self", "camera", "device_scene", "accel_ptr",
                                                 "width", "rows", "refl_ptr", "max_bounces",
                                                 "out_ptr", "fmt", "shadows", "stream"],
        (pkg.RayTracer, "bounce_camera_device"): ["self", "camera", "device_scene", "accel_ptr",
                                                  "width", "rows", "bounce", "out_ptr", "stream"],
    }
    for (owner, name), want in params.items():
        if owner is pkg:
            assert name in pkg.__all__
        sig = inspect.signature(getattr(owner, name)).parameters
        assert list(sig) == want, name
        if "fmt" in sig:
            assert sig["fmt"].default == "i32x4" and sig["shadows"].default is False
    sig = inspect.signature(pkg.light_camera).parameters
    assert sig["reflectivity"].default is None and sig["max_bounces"].default == 0
    assert sig["accel"].default is None and sig["rows"].default is None
    scene = lr.base(pkg)
    cam = pkg.Camera.reference()
    with pytest.raises(ValueError):  # another scene's records
        pkg.light_camera(cam, scene, 3, 2, accel=pkg.build_accel(scene)[:-1])
    with pytest.raises(ValueError):
        pkg.bounce_camera(cam, scene, 3, 2, 1, accel=pkg.build_accel(scene)[:-1])
    with pytest.raises(ValueError):
        pkg.light_camera(cam, scene, 3, 2, fmt="hit")
    with pytest.raises(ValueError):  # one value per colour slot
        pkg.light_camera(cam, scene, 3, 2, np.zeros(3, F32), 1)
    assert pkg.light_camera(cam, scene, 3, 2).shape == (2, 3, 4)
    assert pkg.light_camera(cam, scene, 3, 2, fmt="rgba8", rows=(1, 2)).shape == (1, 3)
    assert pkg.bounce_camera(cam, scene, 3, 2, 0).dtype == pkg.HIT_DTYPE


# --- 6. under the sanitizers -----------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_camera_light_arguments_under_sanitizers(tmp_path):
    """tests/camera_light_args_check.cpp, a program of its own over the host
    sources, under AddressSanitizer + UndefinedBehaviorSanitizer."""
    csrc = lc.REPO / "opencl-ray-tracer_amd" / "csrc"
    exe = tmp_path / "camera_light_args_check"
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{lc.REPO / 'include'}", "-o", str(exe),
                    str(lc.REPO / "tests" / "camera_light_args_check.cpp"),
                    str(csrc / "rt_camera_light.cpp"), str(csrc / "rt_accel.cpp"),
                    str(csrc / "rt_light.cpp"), str(csrc / "rt_args.cpp"),
                    str(csrc / "rt_scene.cpp"), "-lm"],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "camera light args check ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
