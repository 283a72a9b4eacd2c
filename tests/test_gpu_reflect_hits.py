"""rt_reflect_hits_device / rt_light_hits_reflected_device on the GPU: the kernel
(csrc/rt_reflect.hip) against the host functions (csrc/rt_light.cpp), which
tests/test_reflect_hits.py pins to the numpy restatement (tests/reflect_ref.py).

Device memory is torch tensors; every output sits between guard words
(tests/light_device.py), and the guard words and
the hit frame must come back unchanged.  Frames are compared as raw 32-bit
words; no word is masked (a bounce frame holds no created NaN, a lit channel
turns every NaN into INT32_MIN: tests/test_reflect_hits.py).
"""
import numpy as np
import pytest

import light_edges as le
import light_ref as lr
import reflect_ref as rr
import shadow_ref as sr
from gpu_support import H, SCENE_ARRAYS, W, device_scene
from hit_ref import K_FAR, REF_DIR
from light_device import (PASSES, PATTERN, check_scene_padding, compare_all, host_result,
                          padded_device_scene, run_device, unguard, upload_hits)
from light_ref import ONE_LIGHT, THREE_LIGHTS, base, eq

P = "reflect"  # this file's pass of tests/light_device.py
OUTPUTS = PASSES[P].outputs

gpu = pytest.mark.gpu
F32 = np.float32


# --- 1. the four receiver / target kinds ----------------------------------------------
@gpu
@pytest.mark.parametrize("padded", [False, True], ids=["plain", "padded"])
def test_the_four_kinds(pkg, rt, oracle, padded):
    torch = pytest.importorskip("torch")
    scene = rr.mirror_scene(pkg)
    w, h = rr.MIRROR_W, rr.MIRROR_H
    hits = lr.cached_hits(oracle, "mirror", scene, w, h)
    ds, keep = (padded_device_scene if padded else device_scene)(torch, scene)
    got = compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), label="kinds")
    obj, o2, nc = hits["object"], got["bounce"]["object"], scene.num_cubes
    for receiver in (obj < nc, obj >= nc):
        for target in ((o2 >= 0) & (o2 < nc), o2 >= nc):
            assert (receiver & target).sum() >= 100
    assert (o2 == nc + 1).sum() >= 20 and not (obj == nc + 1).any()  # the unseen sphere
    if padded:
        check_scene_padding(torch, scene, keep)
    del keep


# --- 2. wave-level paths ------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", [[], [sr.KINDS_LIGHT]], ids=["no_lights", "one_light"])
def test_wave_level_paths(pkg, rt, oracle, lights):
    """Waves wholly on the face (every lane walks), wholly off it (the wave
    skips the walk) and across its edge (a partial set of lanes walks)."""
    torch = pytest.importorskip("torch")
    scene = rr.wave_scene(pkg, lights)
    w = h = 128
    hits = lr.cached_hits(oracle, "reflect_wave", scene, w, h)
    full, none, mixed = sr.segments(hits["object"] >= 0)  # 70, 114, 72
    assert full >= 30 and none >= 30 and mixed >= 30
    want = pkg.reflect_hits(hits, scene)
    assert (want["object"] == 1).sum() >= 100  # the unseen sphere, in the whole waves ...
    assert sr.segments(want["object"] >= 0)[2] >= 10
    ds, keep = device_scene(torch, scene)
    compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), label="waves")
    del keep


# --- 3. grid edges -------------------------------------------------------------------------
def lone_pixel_scene(pkg):
    """The base scene with sphere 0 moved onto pixel (0, 0), nearer than
    everything else, and sphere 1 straight above it, in front of the ray
    origins: the pixel mirrors it."""
    scene = lr.with_lights(base(pkg), ONE_LIGHT)
    scene.sphere_origins[0] = (0, 0, -5, 1)
    scene.sphere_radius[0] = 3
    scene.sphere_origins[1] = (0, 0, 20, 1)
    scene.sphere_radius[1] = 5
    return scene


@gpu
@pytest.mark.parametrize("w,h", [(1, 1), (257, 3), (83, 31)], ids=["1x1", "257x3", "83x31"])
def test_partial_waves_and_workgroups(pkg, rt, oracle, w, h):
    """Pixel counts that are no multiple of 64 or 256 (1, 771, 2573)."""
    torch = pytest.importorskip("torch")
    assert (w * h) % 64 and (w * h) % 256
    rows = (0, h)
    if (w, h) == (1, 1):
        scene = lone_pixel_scene(pkg)
        hits = lr.cached_hits(oracle, "reflect_lone_pixel", scene, w, h)
        assert hits["object"][0, 0] == scene.num_cubes
        assert pkg.reflect_hits(hits, scene)["object"][0, 0] == scene.num_cubes + 1
    else:
        # (257 x 3: rows 40..42 of a 257 x 80 frame, where the base scene's objects are)
        rows = (40, 43) if h == 3 else (0, h)
        scene = lr.with_lights(base(pkg), ONE_LIGHT)
        hits = lr.cached_hits(oracle, "base", scene, w, H if h == 3 else h, rows)
        assert (pkg.reflect_hits(hits, scene, rows=rows)["object"] >= 0).sum() > 5
    ds, keep = device_scene(torch, scene)
    compare_all(P, pkg, rt, torch, scene, ds, hits, w, rows, label=f"{w}x{h}")
    del keep


# --- 4. trace, then the mirrored light, on one stream ------------------------------------------
@gpu
def test_trace_then_reflected_light_on_one_stream(pkg, rt, oracle):
    """render_device(fmt="hit") and the three reflect calls back to back on a
    non-default stream, no host synchronisation in between: the host pipeline
    (hit_ref, then the host functions) gives the same frames."""
    torch = pytest.importorskip("torch")
    scene = lr.with_lights(base(pkg), THREE_LIGHTS)
    hits_ref = lr.cached_hits(oracle, "base", scene, W, H)
    ds, keep = device_scene(torch, scene)
    hd = torch.full((H, W, 2), PATTERN, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()  # uploads and fills are done before the stream starts
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rt.render_device(ds, W, H, (0, H), hd.data_ptr(), ray_dir=np.array(REF_DIR, F32),
                         fmt="hit", stream=stream.cuda_stream)
        bufs = {what: run_device(P, pkg, rt, torch, ds, hd, W, (0, H), what,
                                 stream=stream.cuda_stream) for what in OUTPUTS}
    stream.synchronize()
    assert np.array_equal(hd.cpu().numpy().view(np.uint32), lr.words(hits_ref))
    for what, buf in bufs.items():
        got = unguard(torch, pkg, buf, W, (0, H), what)
        want = host_result(P, pkg, hits_ref, scene, (0, H), what)
        assert not eq(got, want), f"{what}: {eq(got, want)}"
        if what == "bounce":
            assert (got["object"] >= 0).sum() > 300
    del keep


# --- 5. many candidates through the scalar loops ---------------------------------------------------
@gpu
def test_256_occluders(pkg, rt):
    """18 cubes and 40 spheres: 256 primitives, three lights."""
    torch = pytest.importorskip("torch")
    scene = lr.with_lights(pkg.Scene.synthetic(W, H, 40, 18, seed=11, k=0.3), THREE_LIGHTS)
    assert 12 * scene.num_cubes + scene.num_spheres == 256
    hits, _ = rt.render(scene, W, H, fmt="hit", ray_dir=REF_DIR)
    ds, keep = device_scene(torch, scene)
    got = compare_all(P, pkg, rt, torch, scene, ds, hits, W, (0, H), label="256 primitives")
    o2 = got["bounce"]["object"]
    assert (o2 >= 0).sum() > 50 and len(np.unique(o2)) > 5
    del keep


# --- 6. foreign frames -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["ids", "t"])
def test_foreign_frames(pkg, rt, oracle, kind):
    """Ids just outside [-1, nc + ns) (the host refuses the frame; with those
    ids as -1 it gives what the kernel gives) and foreign t, on padded scenes."""
    torch = pytest.importorskip("torch")
    scene = lr.with_lights(base(pkg), THREE_LIGHTS)
    valid = lr.cached_hits(oracle, "base", scene, W, H)
    given, counts = (le.foreign_ids if kind == "ids" else le.foreign_t)(valid, scene)
    assert len(counts) == (9 if kind == "ids" else 14) and min(counts.values()) >= 4
    obj = given["object"]
    outside = (obj < -1) | (obj >= scene.num_cubes + scene.num_spheres)
    mapped = np.array(given)
    mapped["object"][outside] = -1
    if kind == "ids":
        assert outside.sum() == 36
        for what in OUTPUTS:
            with pytest.raises(pkg.RtError) as e:
                host_result(P, pkg, given, scene, (0, H), what)
            assert e.value.status == pkg.RT_ERR_INVALID_ARG
    else:
        assert not outside.any()
        # t == 300000 beside a real object: the bounce frame walks, the lit frame does not
        far = (given["t"] == K_FAR) & (obj >= 0)
        assert far.sum() >= 8
    ds, keep = padded_device_scene(torch, scene)
    got = compare_all(P, pkg, rt, torch, scene, ds, given, W, (0, H), label=f"foreign {kind}",
                      host_hits=mapped)
    o2 = got["bounce"]["object"]
    assert (o2[outside] == -1).all() and (got["bounce"]["t"][outside] == K_FAR).all()
    assert (o2 >= 0).sum() > 300
    check_scene_padding(torch, scene, keep)
    del keep


# --- 7. numeric edges ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", rr.EDGE_NAMES)
def test_numeric_edges(pkg, rt, oracle, name):
    torch = pytest.importorskip("torch")
    scene, w, h, d, key = rr.edge_cases(pkg)[name]
    hits = lr.cached_hits(oracle, key, scene, w, h, None, d)
    ds, keep = device_scene(torch, scene)
    compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), d=d, label=name)
    del keep


@gpu
@pytest.mark.parametrize("name", ["twins", "sphere_tie", "inside_a_sphere", "ramp"])
def test_ties_far_roots_and_the_ramps_end(pkg, rt, oracle, name):
    """The remaining scenes of the CPU file."""
    torch = pytest.importorskip("torch")
    scene, key = {
        "twins": (rr.twin_cubes_scene(pkg), "reflect_twins"),
        "sphere_tie": (rr.sphere_tie_scene(pkg), "reflect_sphere_tie"),
        "inside_a_sphere": (sr.intersecting_spheres(pkg, [(32, 24, 100, 1)]),
                            "shadow_edge_p_inside_a_sphere"),
        "ramp": (rr.ramp_scene(pkg, ONE_LIGHT), "reflect_ramp"),
    }[name]
    w, h = 64, 48
    hits = lr.cached_hits(oracle, key, scene, w, h)
    ds, keep = device_scene(torch, scene)
    got = compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), label=name)
    if name == "sphere_tie":
        y, x = rr.TIE_PIXEL
        assert got["bounce"]["object"][y, x] == 0
    if name == "twins":
        assert not (got["bounce"]["object"] == 1).any()
    del keep


# --- 8. nothing to mirror ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", [[], ONE_LIGHT], ids=["no_lights", "one_light"])
def test_empty_scene(pkg, rt, lights):
    """NULL scene arrays, with and without lights: (300000, -1), (0, 0, 0, 255)."""
    torch = pytest.importorskip("torch")
    scene = lr.with_lights(pkg.Scene(), lights)
    w, h = 70, 9
    hits = np.empty((h, w), pkg.HIT_DTYPE)
    hits["t"], hits["object"] = K_FAR, -1
    ds, keep = device_scene(torch, scene)
    assert not any(ds.get(k) for k in SCENE_ARRAYS[:5]) and ds["num_lights"] == len(lights)
    got = compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), label="empty")
    assert (got["bounce"]["object"] == -1).all() and (got["bounce"]["t"] == K_FAR).all()
    assert (got["i32x4"] == (0, 0, 0, 255)).all() and (got["rgba8"] == 0xFF000000).all()
    del keep


# --- 9. reflectivity 0 is the light pass ---------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", [[], THREE_LIGHTS], ids=["no_lights", "three_lights"])
def test_reflectivity_zero_is_light_hits_device(pkg, rt, oracle, lights):
    torch = pytest.importorskip("torch")
    scene = rr.mirror_scene(pkg, lights)
    w, h = rr.MIRROR_W, rr.MIRROR_H
    hits = lr.cached_hits(oracle, "mirror", scene, w, h)
    ds, keep = device_scene(torch, scene)
    hd = upload_hits(torch, hits)
    for what in ("i32x4", "rgba8"):
        for refl in (0.0, -0.0):
            got = unguard(torch, pkg, run_device(P, pkg, rt, torch, ds, hd, w, (0, h), what,
                                                 refl=refl), w, (0, h), what)
            want = unguard(torch, pkg, run_device("light", pkg, rt, torch, ds, hd, w, (0, h),
                                                  what), w, (0, h), what)
            assert not eq(got, want), f"{what}: {eq(got, want)}"
            assert not eq(got, pkg.light_hits(hits, scene, what)), what
    del keep
