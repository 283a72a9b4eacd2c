"""rt_light_camera_device / rt_bounce_camera_device on the GPU: the kernels
(csrc/rt_camera_light.hip, both walks, all three outputs) against the host
functions (csrc/rt_camera_light.cpp), which tests/test_camera_light.py pins to
the numpy restatement, to the deferred pass and culled to unculled.

Device memory is torch tensors.  Every output sits between guard words
(test_gpu_rays.guarded_words), the scene's arrays and the reflectivity between
padding (light_device.padded_device_scene); the records are built on the
device into guarded words.  Scene, reflectivity and records must come back
unchanged.  Frames are compared as raw 32-bit words.
"""
import numpy as np
import pytest

import camera_light_ref as cr
import light_device as ld
import light_ref as lr
import mirror_ref as mr
import rays_ref as yr
import test_camera_light as tc
import test_gpu_rays as tg
from gpu_support import H, W
from light_ref import eq

gpu = pytest.mark.gpu
F32 = np.float32
RECORD_WORDS = 80  # 320 bytes
WORDS = {"bounce": 2, "i32x4": 4, "rgba8": 1}
# (output, max_bounces or bounce, shadows)
SETTINGS = (("bounce", 0, False), ("bounce", 2, False), ("i32x4", 0, False), ("i32x4", 2, True),
            ("rgba8", 8, False))


def host_frame(pkg, cam, scene, w, rows, refl, label):
    what, depth, shadows = label
    h = rows[1]
    if what == "bounce":
        return pkg.bounce_camera(cam, scene, w, h, depth, rows=rows)
    return pkg.light_camera(cam, scene, w, h, refl, depth, shadows, what, rows=rows)


def read_frame(pkg, torch, buf, w, rows, what):
    body, n = tg.body_words(torch, buf), rows[1] - rows[0]
    if what == "bounce":
        return body.view(pkg.HIT_DTYPE).reshape(n, w)
    return body.view(np.int32).reshape(n, w, 4) if what == "i32x4" else body.reshape(n, w)


def launch(pkg, rt, torch, cam, ds, accel_ptr, w, rows, refl_ptr, label, stream=0):
    """One device call into guarded words; returns the tensor."""
    what, depth, shadows = label
    buf, ptr = tg.guarded_words(torch, (rows[1] - rows[0]) * w * WORDS[what])
    if not stream:
        torch.cuda.synchronize()  # the fill and the caller's uploads are done
    if what == "bounce":
        rt.bounce_camera_device(cam, ds, accel_ptr, w, rows, depth, ptr, stream=stream)
    else:
        rt.light_camera_device(cam, ds, accel_ptr, w, rows, refl_ptr, depth, ptr, fmt=what,
                               shadows=shadows, stream=stream)
    return buf


def compare(pkg, rt, torch, scene, cam, w, rows, refl, settings=SETTINGS, label=""):
    """Every setting through both kernel instances (accel_ptr 0: unculled; the
    device-built records: culled) against the host's unculled frame.  Returns
    the host frames by setting."""
    ds, keep = ld.padded_device_scene(torch, scene)
    refl_dev = (0, None) if refl is None else ld.padded_array(torch, refl)
    records, accel_ptr = tg.guarded_words(torch, RECORD_WORDS * scene.num_cubes)
    torch.cuda.synchronize()
    rt.build_accel_device(ds, accel_ptr if scene.num_cubes else 0)
    want_records = pkg.build_accel(scene).tobytes()
    assert tg.body_words(torch, records).tobytes() == want_records, "records"
    out = {}
    for s in settings:
        want = out[s] = host_frame(pkg, cam, scene, w, rows, refl, s)
        # (without cubes the records' address is still one: the culled instance)
        for name, a in (("unculled", 0), ("culled", accel_ptr)):
            buf = launch(pkg, rt, torch, cam, ds, a, w, rows, refl_dev[0], s)
            got = read_frame(pkg, torch, buf, w, rows, s[0])
            assert got.dtype == want.dtype and not eq(got, want), \
                f"{label} {name} {s}: {eq(got, want)}"
    ld.check_scene_padding(torch, scene, keep)
    if refl is not None:
        ld.check_padding(torch, refl, refl_dev[1], "reflectivity")
    assert tg.body_words(torch, records).tobytes() == want_records, "records after"
    del keep
    return out


def base_view(pkg, w, h):
    """The base scene under three lights through a pinhole that looks at its
    first sphere: the centre pixel hits."""
    scene = lr.with_lights(lr.base(pkg), lr.THREE_LIGHTS)
    target = tuple(float(v) for v in scene.sphere_origins[0][:3])
    return scene, pkg.Camera.pinhole((30, 20, 90), target, tc.UP, 50.0, w, h)


# --- 1. grid edges ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h,rows", [(1, 1, None), (37, 29, None), (37, 29, (5, 17)),
                                      (257, 80, (39, 42)), (83, 31, None)],
                         ids=["1x1", "37x29", "37x29_band", "257x3", "83x31"])
def test_partial_waves_and_workgroups(pkg, rt, w, h, rows):
    """Pixel counts that are no multiple of 64 or 256 (1, 1073, 444, 771,
    2573), and a band offset; 257 x 3 is rows 39..41 of a 257 x 80 view."""
    torch = pytest.importorskip("torch")
    scene, cam = base_view(pkg, w, h)
    rows = rows or (0, h)
    assert ((rows[1] - rows[0]) * w) % 64
    want = compare(pkg, rt, torch, scene, cam, w, rows, mr.mixed(scene), label=f"{w}x{h}")
    hit = want["bounce", 0, False]["object"] >= 0
    if (w, h) == (1, 1):
        assert hit.all()
    else:
        assert hit.sum() >= 20 and (~hit).sum() >= 20
        assert (want["i32x4", 2, True][..., :3] != 0).any(-1).sum() >= 10  # not a black frame


# --- 2. waves by what their lanes do -----------------------------------------------------------
def lanes_camera(pkg):
    """Origin (x, y, 0), direction (0, 0, -1): pixel (x, y) looks down the z axis."""
    return pkg.Camera(ou=(1, 0, 0), ov=(0, 1, 0), d0=(0, 0, -1))


@gpu
@pytest.mark.parametrize("kind", ["all_miss", "one_lane", "one_cube", "levels", "mirrors_8"])
def test_waves_by_what_their_lanes_do(pkg, rt, kind):
    """A 64-wide frame: every row is a wave."""
    torch = pytest.importorskip("torch")
    w = 64
    deep = (("bounce", 1, False), ("bounce", 8, False), ("i32x4", 8, True), ("rgba8", 8, False),
            ("i32x4", 1, False))
    if kind == "all_miss":  # the camera is turned away: no further walk is entered
        scene = lr.with_lights(lr.base(pkg), lr.THREE_LIGHTS)
        cam, h = pkg.Camera.pinhole((30, 20, 90), (30, 20, 300), tc.UP, 50.0, w, 4), 4
        refl = mr.mixed(scene)
    elif kind == "one_lane":  # a sphere of radius 0.4 under pixel (20, 1) alone
        scene = lr.with_lights(lr.one_sphere(pkg, (20, 1, -30, 1), 0.4, (0.9, 0.5, 0.2, 255)),
                               lr.THREE_LIGHTS)
        cam, h, refl = lanes_camera(pkg), 4, np.ones(1, F32)
    elif kind == "one_cube":  # a face far wider than the frame, a perfect mirror
        scene = lr.with_lights(lr.one_cube(pkg, [("scale", 400, 400, 10), ("translate", 32, 2, -60)],
                                           (1.0, 0.7, 0.3, 255)), lr.THREE_LIGHTS)
        cam, h, refl = lanes_camera(pkg), 4, np.ones(1, F32)
    elif kind == "levels":  # chains of one wave that end at levels 0, 1 and >= 2
        scene, cam, _, h, refl = tc.cases(pkg)["wave_generic1"]
        c = tc.chain_of(pkg, "wave_generic1")
        _, last, _ = c.stats(refl, 8)
        per_row = [set(np.minimum(row[row >= 0], 2)) for row in last]
        assert sum(r == {0, 1, 2} for r in per_row) >= 1, per_row
    else:  # depth 8, every object a perfect mirror: the whole 32 KiB LDS stack
        scene, cam, _, h, refl = tc.cases(pkg)["corridor_pinhole"]
        assert (refl == 1).all()
    want = compare(pkg, rt, torch, scene, cam, w, (0, h), refl, settings=deep, label=kind)
    hit = want["bounce", 0, False]["object"] >= 0 if ("bounce", 0, False) in want else \
        pkg.cast_camera(cam, scene, w, h)["object"] >= 0
    if kind == "all_miss":
        assert not hit.any() and (want["i32x4", 8, True] == (0, 0, 0, 255)).all()
    elif kind == "one_lane":
        assert hit.sum() == 1 and hit[1, 20]
    elif kind == "one_cube":
        assert hit.all() and (want["bounce", 1, False]["object"] == -1).all()
    elif kind == "mirrors_8":
        assert (want["bounce", 8, False]["object"] >= 0).sum() >= 64


# --- 3. scene and light counts -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["no_cubes", "empty", "no_lights", "33_lights", "256_primitives"])
def test_scene_and_light_counts(pkg, rt, name):
    torch = pytest.importorskip("torch")
    big = tc.many(pkg)
    w, h = (64, 64) if name == "256_primitives" else (48, 40)
    scene = {"no_cubes": lambda: pkg.Scene(big.sphere_origins, big.sphere_radius,
                                           big.sphere_colours, lights=big.lights),
             "empty": lambda: lr.with_lights(pkg.Scene(), lr.ONE_LIGHT),
             "no_lights": lambda: lr.with_lights(big, []),
             "33_lights": lambda: lr.with_lights(lr.base(pkg), [(3 * i, 5, 60, 1) for i in range(33)]),
             "256_primitives": lambda: lr.with_lights(
                 pkg.Scene.synthetic(W, H, 40, 18, seed=11, k=0.3), lr.THREE_LIGHTS)}[name]()
    if name == "256_primitives":
        assert 12 * scene.num_cubes + scene.num_spheres == 256
    cam = pkg.Camera.pinhole((30, 20, 90), (32, 24, -40), tc.UP, 50.0, w, h)
    refl = mr.mixed(scene) if yr.slots(scene) else None
    settings = (("bounce", 2, False), ("i32x4", 2, True), ("rgba8", 2, False)) \
        if name in ("no_lights", "256_primitives") else SETTINGS
    want = compare(pkg, rt, torch, scene, cam, w, (0, h), refl, settings=settings, label=name)
    if name == "empty":
        assert (want["i32x4", 2, True] == (0, 0, 0, 255)).all()
        assert (want["bounce", 2, False]["object"] == -1).all()
    else:
        assert (pkg.cast_camera(cam, scene, w, h)["object"] >= 0).sum() >= 100


# --- 4. one stream -------------------------------------------------------------------------------
@gpu
def test_build_light_bounce_on_one_stream(pkg, rt):
    """build_accel_device -> light_camera_device -> bounce_camera_device back
    to back on one non-default stream, no synchronisation in between."""
    torch = pytest.importorskip("torch")
    scene, cam, w, h, refl = tc.cases(pkg)["many_pinhole"]
    ds, keep = ld.padded_device_scene(torch, scene)
    refl_ptr, keep_refl = ld.padded_array(torch, refl)
    records, accel_ptr = tg.guarded_words(torch, RECORD_WORDS * scene.num_cubes)
    lit, bounce = ("i32x4", 3, True), ("bounce", 2, False)
    torch.cuda.synchronize()  # uploads and fills are done before the stream starts
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        # (the output tensors are filled on this stream, in front of their launches)
        rt.build_accel_device(ds, accel_ptr, stream=st)
        bufs = [launch(pkg, rt, torch, cam, ds, accel_ptr, w, (0, h), refl_ptr, s, stream=st)
                for s in (lit, bounce)]
    stream.synchronize()
    assert tg.body_words(torch, records).tobytes() == pkg.build_accel(scene).tobytes()
    for s, buf in zip((lit, bounce), bufs):
        got = read_frame(pkg, torch, buf, w, (0, h), s[0])
        want = host_frame(pkg, cam, scene, w, (0, h), refl, s)
        assert not eq(got, want), f"{s}: {eq(got, want)}"
    ld.check_scene_padding(torch, scene, keep)
    ld.check_padding(torch, refl, keep_refl, "reflectivity")
    del keep


# --- 5. edge cameras -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", tc.EDGE_CAMERAS)
def test_edge_cameras(pkg, rt, name):
    torch = pytest.importorskip("torch")
    scene, cam = tc.edge_scene(pkg), tc.edge_cameras(pkg)[name]
    tc.check_edge_camera(name, cr.restated(("edge", name), scene, cam, tc.EDGE_W, (0, tc.EDGE_H)))
    compare(pkg, rt, torch, scene, cam, tc.EDGE_W, (0, tc.EDGE_H), mr.mixed(scene),
            settings=(("bounce", 0, False), ("bounce", 8, False), ("i32x4", 8, True),
                      ("rgba8", 2, False)), label=name)


# --- 6. the headless driver ----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("accel", [False, True], ids=["unculled", "accel"])
def test_headless_lit_camera_ppm(pkg, tmp_path, accel):
    """rt_headless --camera ... --light ... --mirror ... --shadows [--accel]
    --ppm on reference scene 1 at 64 x 48: the PPM bytes are the Python
    pipeline's (pinhole -> light_camera); without the three options --camera is
    the depth ramp as before (tests/test_gpu_rays.py)."""
    import subprocess
    exe = pkg.PKG_DIR / "rt_headless"
    assert exe.exists()
    w, h = 64, 48
    eye, target, fov = (320.0, 240.0, 400.0), (320.0, 240.0, -100.0), 70.0
    lights = [(300.0, 200.0, 300.0), (0.0, 0.0, 50.0)]
    out = tmp_path / "lit.ppm"
    spec = ",".join(str(v) for v in (*eye, *target, fov))
    cmd = [str(exe), "--scene", "1", "--width", str(w), "--height", str(h), "--camera", spec]
    for l in lights:
        cmd += ["--light", ",".join(str(v) for v in l)]
    cmd += ["--mirror", "0.25,2", "--shadows", "--ppm", str(out)] + (["--accel"] if accel else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    scene = lr.with_lights(pkg.Scene.reference(1), [l + (1.0,) for l in lights])
    cam = pkg.Camera.pinhole(eye, target, tc.UP, fov, w, h)
    refl = np.full(yr.slots(scene), 0.25, F32)
    want = pkg.light_camera(cam, scene, w, h, refl, 2, True)
    assert (want[..., :3] != 0).any(-1).sum() >= 100 and (want[..., :3] == 0).all(-1).sum() >= 100
    assert (want != pkg.light_camera(cam, scene, w, h, refl, 0, False)).any(-1).sum() >= 20
    rgb = want[..., :3].astype(np.uint8)  # the Texture's (uint8_t) wrap
    assert out.read_bytes() == f"P6\n{w} {h}\n255\n".encode() + rgb.tobytes()
    assert f"fnv1a64 {pkg.fnv1a64(want):016x}" in r.stdout


# --- 7. a fresh context's renders behind the new code object -------------------------------------
@gpu
def test_fresh_context_renders_after_a_camera_launch(pkg, rt):
    """rt_init does not preload this translation unit: its code object is
    loaded by the first launch.  Behind such a launch a fresh context renders
    int32x4, int32x4, RGBA8 (the sequence of
    test_gpu_hit_format.py::test_automatic_choice_at_size, 1280 x 1024 at
    config 3's density) and gives the session context's frames."""
    torch = pytest.importorskip("torch")
    scene, cam = base_view(pkg, 37, 29)
    ds, keep = ld.padded_device_scene(torch, scene)
    refl_ptr, keep_refl = ld.padded_array(torch, mr.mixed(scene))
    buf = launch(pkg, rt, torch, cam, ds, 0, 37, (0, 29), refl_ptr, ("i32x4", 2, True))
    tg.body_words(torch, buf)  # (synchronises)
    w, h = 1280, 1024
    dense = pkg.Scene.synthetic(w, h, 256, 64, seed=3, k=2.0)
    want = {fmt: rt.render(dense, w, h, fmt=fmt)[0].copy() for fmt in ("i32x4", "rgba8")}
    with pkg.RayTracer(0) as fresh:
        for fmt in ("i32x4", "i32x4", "rgba8"):
            got, _ = fresh.render(dense, w, h, fmt=fmt)
            assert np.array_equal(got, want[fmt]), fmt
    del keep, keep_refl
