"""rt_shadow_hits_reflected_device / rt_light_hits_shadowed_reflected_device on
the GPU: the kernel (csrc/rt_shadow_reflect.hip) against the host functions
(csrc/rt_light.cpp), which tests/test_shadow_reflect_hits.py pins to the numpy
restatement (tests/shadow_reflect_ref.py).

Device memory is torch tensors; every output sits between guard words
(tests/light_device.py), and the guard
words and the hit frame must come back unchanged.  Frames are compared as raw
32-bit words; no word is masked (a mask holds no NaN, a lit channel turns
every NaN into INT32_MIN).
"""
import numpy as np
import pytest

import light_edges as le
import light_ref as lr
import reflect_ref as rr
import shadow_ref as sr
import shadow_reflect_ref as srr
from gpu_support import H, SCENE_ARRAYS, W, device_scene
from hit_ref import K_FAR, REF_DIR
from light_device import (PASSES, PATTERN, check_scene_padding, compare_all, host_result,
                          padded_device_scene, run_device, unguard, upload_hits)
from light_ref import ONE_LIGHT, THREE_LIGHTS, base, eq
from test_gpu_reflect_hits import lone_pixel_scene
from test_shadow_reflect_hits import INSIDE_LIGHTS, SPECIAL_NAMES, class_facts, special_scenes

P = "shadow_reflect"  # this file's pass of tests/light_device.py
OUTPUTS = PASSES[P].outputs

gpu = pytest.mark.gpu
F32 = np.float32


# --- 1. the classes of pixels ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("padded", [False, True], ids=["plain", "padded"])
def test_the_classes(pkg, rt, oracle, padded):
    torch = pytest.importorskip("torch")
    scene = srr.class_scene(pkg)
    w, h = srr.CLASS_W, srr.CLASS_H
    hits = lr.cached_hits(oracle, "shadow_reflect_class", scene, w, h)
    class_facts(scene, hits, srr.shadow_reflect_ref(oracle, scene, hits))
    ds, keep = (padded_device_scene if padded else device_scene)(torch, scene)
    got = compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), label="classes")
    assert (got["mask2"] == 1).sum() >= 100 and (got["mask2"] == 2).sum() >= 100
    if padded:
        check_scene_padding(torch, scene, keep)
    del keep


# --- 2. wave-level paths ------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", sorted(srr.WAVE_LIGHTS))
def test_wave_level_paths(pkg, rt, oracle, lights):
    """64-pixel segments of a 128-wide frame are waves.  Hit lanes: all, none,
    some.  Bounces of the hit lanes: all miss (phase 3 is never entered), all
    hit, mixed.  Facing lights at p2: under the light "above" no lane of any
    wave has one; "beside", most waves of phase 3 do."""
    torch = pytest.importorskip("torch")
    scene = srr.wave_scene(pkg, srr.WAVE_LIGHTS[lights])
    w = h = 128
    hits = lr.cached_hits(oracle, "shadow_reflect_wave", scene, w, h)
    c = srr.shadow_reflect_ref(oracle, scene, hits)
    full, none, mixed = sr.segments(hits["object"] >= 0)  # 70, 114, 72
    assert full >= 30 and none >= 30 and mixed >= 30
    hit, hit2 = (hits["object"] >= 0).reshape(-1, 64), c.hit2.reshape(-1, 64)
    with_hits = hit.any(1)
    assert (with_hits & ~hit2.any(1)).sum() >= 20          # every bounce misses: 36
    assert (with_hits & (hit2 == hit).all(1)).sum() >= 20  # every bounce hits: 45
    assert (with_hits & hit2.any(1) & ~(hit2 == hit).all(1)).sum() >= 20  # mixed: 61
    faces2 = c.at_p2.cast.any(0).reshape(-1, 64)
    if lights == "above":
        assert (hit2.any(1) & ~faces2.any(1)).sum() >= 50 and not faces2.any()  # 106
        assert c.at_p.occluded.any(0).sum() >= 1000  # the sphere shadows the face
    else:
        assert (hit2.any(1) & faces2.any(1)).sum() >= 50  # 103
        assert sr.segments(c.at_p2.cast.any(0))[2] >= 50  # a partial pending set
    ds, keep = device_scene(torch, scene)
    compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), label="waves")
    del keep


# --- 3. grid edges -------------------------------------------------------------------------
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
        scene = lr.with_lights(base(pkg), THREE_LIGHTS)
        hits = lr.cached_hits(oracle, "base", scene, w, H if h == 3 else h, rows)
        assert (pkg.reflect_hits(hits, scene, rows=rows)["object"] >= 0).sum() > 5
    ds, keep = device_scene(torch, scene)
    compare_all(P, pkg, rt, torch, scene, ds, hits, w, rows, label=f"{w}x{h}")
    del keep


# --- 4. behind the trace, and behind the bounce, on one stream -----------------------------------
@gpu
def test_trace_then_reflect_then_shadowed_reflected_light_on_one_stream(pkg, rt, oracle):
    """render_device(fmt="hit"), the three calls, rt_reflect_hits_device and
    the three calls again, back to back on a non-default stream with no host
    synchronisation in between: the host pipeline gives the same frames."""
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
        first = {what: run_device(P, pkg, rt, torch, ds, hd, W, (0, H), what,
                                  stream=stream.cuda_stream) for what in OUTPUTS}
        bounce = run_device("reflect", pkg, rt, torch, ds, hd, W, (0, H), "bounce",
                            stream=stream.cuda_stream)
        second = {what: run_device(P, pkg, rt, torch, ds, hd, W, (0, H), what,
                                   stream=stream.cuda_stream) for what in OUTPUTS}
    stream.synchronize()
    assert np.array_equal(hd.cpu().numpy().view(np.uint32), lr.words(hits_ref))
    got = unguard(torch, pkg, bounce, W, (0, H), "bounce")
    assert not eq(got, pkg.reflect_hits(hits_ref, scene)) and (got["object"] >= 0).sum() > 300
    for bufs in (first, second):
        for what, buf in bufs.items():
            got = unguard(torch, pkg, buf, W, (0, H), what)
            want = host_result(P, pkg, hits_ref, scene, (0, H), what)
            assert not eq(got, want), f"{what}: {eq(got, want)}"
            if what == "mask2":
                assert (got != 0).sum() >= 20
    del keep


# --- 5. many occluders and candidates through the scalar loops ---------------------------------------
@gpu
def test_256_occluders(pkg, rt):
    """18 cubes and 40 spheres: 256 primitives, three lights."""
    torch = pytest.importorskip("torch")
    scene = lr.with_lights(pkg.Scene.synthetic(W, H, 40, 18, seed=11, k=0.3), THREE_LIGHTS)
    assert 12 * scene.num_cubes + scene.num_spheres == 256
    hits, _ = rt.render(scene, W, H, fmt="hit", ray_dir=REF_DIR)
    ds, keep = device_scene(torch, scene)
    got = compare_all(P, pkg, rt, torch, scene, ds, hits, W, (0, H), label="256 primitives")
    assert (got["mask2"] != 0).sum() > 20 and len(np.unique(got["mask2"])) >= 3
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
    n_slots = scene.num_cubes + scene.num_spheres
    outside = (obj < -1) | (obj >= n_slots)
    mapped = np.array(given)
    mapped["object"][outside] = -1
    if kind == "ids":
        assert outside.sum() == 36 and set(np.unique(obj[outside])) == {-2, n_slots, n_slots + 1}
        for what in OUTPUTS:
            with pytest.raises(pkg.RtError) as e:
                host_result(P, pkg, given, scene, (0, H), what)
            assert e.value.status == pkg.RT_ERR_INVALID_ARG
    else:
        assert not outside.any()
        # t == 300000 beside a real object: the mask walks, the lit frame does not
        far = (given["t"] == K_FAR) & (obj >= 0)
        assert far.sum() >= 8
    ds, keep = padded_device_scene(torch, scene)
    got = compare_all(P, pkg, rt, torch, scene, ds, given, W, (0, H), label=f"foreign {kind}",
                      host_hits=mapped)
    assert not got["mask2"][outside].any() and (got["mask2"] != 0).sum() >= 20
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
@pytest.mark.parametrize("name", SPECIAL_NAMES + ["inside_a_sphere"])
def test_ties_far_roots_and_the_ramps_end(pkg, rt, oracle, name):
    """The remaining scenes of the CPU file."""
    torch = pytest.importorskip("torch")
    scenes = special_scenes(pkg)
    scenes["inside_a_sphere"] = (sr.intersecting_spheres(pkg, INSIDE_LIGHTS),
                                 "shadow_edge_p_inside_a_sphere")
    scene, key = scenes[name]
    w, h = 64, 48
    hits = lr.cached_hits(oracle, key, scene, w, h)
    ds, keep = device_scene(torch, scene)
    got = compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), label=name)
    if name == "inside_a_sphere":
        assert (got["mask2"] & 2).any() and ((got["mask2"] & 2) == 0).sum() > 100
    del keep


# --- 8. nothing to light ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", [[], ONE_LIGHT], ids=["no_lights", "one_light"])
def test_empty_scene(pkg, rt, lights):
    """NULL scene arrays, with and without lights: mask 0, (0, 0, 0, 255)."""
    torch = pytest.importorskip("torch")
    scene = lr.with_lights(pkg.Scene(), lights)
    w, h = 70, 9
    hits = np.empty((h, w), pkg.HIT_DTYPE)
    hits["t"], hits["object"] = K_FAR, -1
    ds, keep = device_scene(torch, scene)
    assert not any(ds.get(k) for k in SCENE_ARRAYS[:5]) and ds["num_lights"] == len(lights)
    got = compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), label="empty")
    assert not got["mask2"].any()
    assert (got["i32x4"] == (0, 0, 0, 255)).all() and (got["rgba8"] == 0xFF000000).all()
    del keep


# --- 9. the identities with the parent kernels --------------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", [[], srr.CLASS_LIGHTS], ids=["no_lights", "two_lights"])
def test_reflectivity_zero_is_the_shadow_kernels_frame(pkg, rt, oracle, lights):
    torch = pytest.importorskip("torch")
    scene = srr.class_scene(pkg, lights)
    w, h = srr.CLASS_W, srr.CLASS_H
    hits = lr.cached_hits(oracle, "shadow_reflect_class", scene, w, h)
    ds, keep = device_scene(torch, scene)
    hd = upload_hits(torch, hits)
    for what in ("i32x4", "rgba8"):
        want = unguard(torch, pkg, run_device("shadow", pkg, rt, torch, ds, hd, w, (0, h), what),
                       w, (0, h), what)
        assert not eq(want, pkg.light_hits(hits, scene, what, shadows=True)), what
        for refl in (0.0, -0.0):
            got = unguard(torch, pkg, run_device(P, pkg, rt, torch, ds, hd, w, (0, h), what,
                                                 refl=refl), w, (0, h), what)
            assert not eq(got, want), f"{what}: {eq(got, want)}"
    del keep


@gpu
def test_without_lights_it_is_the_reflect_kernels_frame(pkg, rt, oracle):
    """... and shadows=False is the call of before."""
    torch = pytest.importorskip("torch")
    scene = srr.class_scene(pkg, ())
    w, h = srr.CLASS_W, srr.CLASS_H
    hits = lr.cached_hits(oracle, "shadow_reflect_class", scene, w, h)
    ds, keep = device_scene(torch, scene)
    hd = upload_hits(torch, hits)
    for what in ("i32x4", "rgba8"):
        for refl in (0.25, 1.0):
            want = unguard(torch, pkg, run_device("reflect", pkg, rt, torch, ds, hd, w,
                                                  (0, h), what, refl=refl),
                           w, (0, h), what)
            assert not eq(want, pkg.light_hits_reflected(hits, scene, refl, what)), what
            got = unguard(torch, pkg, run_device(P, pkg, rt, torch, ds, hd, w, (0, h), what,
                                                 refl=refl), w, (0, h), what)
            assert not eq(got, want), f"{what} r={refl}: {eq(got, want)}"
    got = unguard(torch, pkg, run_device(P, pkg, rt, torch, ds, hd, w, (0, h), "mask2"),
                  w, (0, h), "mask2")
    assert not got.any()
    del keep
