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

import light_device as ld
import light_ref as lr
import reflect_ref as rr
import shadow_ref as sr
import shadow_reflect_ref as srr
from gpu_support import device_scene
from light_device import (PASSES, check_scene_padding, compare_all, padded_device_scene,
                          run_device, unguard, upload_hits)
from light_ref import ONE_LIGHT, THREE_LIGHTS, eq

P = "shadow_reflect"  # this file's pass of tests/light_device.py
OUTPUTS = PASSES[P].outputs

gpu = pytest.mark.gpu


# --- 1. the classes of pixels ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("padded", [False, True], ids=["plain", "padded"])
def test_the_classes(pkg, rt, oracle, padded):
    torch = pytest.importorskip("torch")
    scene = srr.class_scene(pkg)
    w, h = srr.CLASS_W, srr.CLASS_H
    hits, c = srr.restated(oracle, "shadow_reflect_class", scene, w, h)
    srr.class_facts(scene, hits, c)
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
    hits, c = srr.restated(oracle, "shadow_reflect_wave", scene, w, h)
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

    def facts(scene, hits, rows):
        o2 = pkg.reflect_hits(hits, scene, rows=rows)["object"]
        assert o2[0, 0] == scene.num_cubes + 1 if (w, h) == (1, 1) else (o2 >= 0).sum() > 5
    ld.partial_waves_and_workgroups(P, pkg, rt, torch, oracle, w, h,
                                    (rr.lone_pixel_scene(pkg), "reflect_lone_pixel"),
                                    THREE_LIGHTS, facts)


# --- 4. behind the trace, and behind the bounce, on one stream -----------------------------------
@gpu
def test_trace_then_reflect_then_shadowed_reflected_light_on_one_stream(pkg, rt, oracle):
    """render_device(fmt="hit"), the three calls, rt_reflect_hits_device and
    the three calls again, back to back on a non-default stream with no host
    synchronisation in between: the host pipeline gives the same frames."""
    torch = pytest.importorskip("torch")
    three = [(P, what, ld.Extras()) for what in OUTPUTS]

    def facts(p, what, got):
        assert what != "mask2" or (got != 0).sum() >= 20
        assert what != "bounce" or (got["object"] >= 0).sum() > 300
    ld.trace_then_calls_on_one_stream(pkg, rt, torch, oracle,
                                      three + [("reflect", "bounce", ld.Extras())] + three, facts)


# --- 5. many occluders and candidates through the scalar loops ---------------------------------------
@gpu
def test_256_occluders(pkg, rt):
    """18 cubes and 40 spheres: 256 primitives, three lights."""
    torch = pytest.importorskip("torch")

    def facts(scene, hits, got):
        assert (got["mask2"] != 0).sum() > 20 and len(np.unique(got["mask2"])) >= 3
    ld.many_primitives(P, pkg, rt, torch, facts)


# --- 6. foreign frames -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["ids", "t"])
def test_foreign_frames(pkg, rt, oracle, kind):
    """Ids just outside [-1, nc + ns) (the host refuses the frame; with those
    ids as -1 it gives what the kernel gives) and foreign t, on padded scenes."""
    torch = pytest.importorskip("torch")

    def facts(got, outside):
        assert not got["mask2"][outside].any() and (got["mask2"] != 0).sum() >= 20
    ld.foreign_frames(P, pkg, rt, torch, oracle, kind, facts)


# --- 7. numeric edges ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", rr.EDGE_NAMES)
def test_numeric_edges(pkg, rt, oracle, name):
    torch = pytest.importorskip("torch")
    scene, w, h, d, key = rr.edge_cases(pkg)[name]
    ld.compare_scene(P, pkg, rt, torch, oracle, key, scene, w, h, d, label=name)


@gpu
@pytest.mark.parametrize("name", srr.SPECIAL_NAMES + ["inside_a_sphere"])
def test_ties_far_roots_and_the_ramps_end(pkg, rt, oracle, name):
    """The remaining scenes of the CPU file."""
    torch = pytest.importorskip("torch")
    scenes = srr.special_scenes(pkg)
    scenes["inside_a_sphere"] = (sr.intersecting_spheres(pkg, srr.INSIDE_LIGHTS),
                                 "shadow_edge_p_inside_a_sphere")
    scene, key = scenes[name]
    got = ld.compare_scene(P, pkg, rt, torch, oracle, key, scene, 64, 48, label=name)
    if name == "inside_a_sphere":
        assert (got["mask2"] & 2).any() and ((got["mask2"] & 2) == 0).sum() > 100


# --- 8. nothing to light ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", [[], ONE_LIGHT], ids=["no_lights", "one_light"])
def test_empty_scene(pkg, rt, lights):
    """NULL scene arrays, with and without lights: mask 0, (0, 0, 0, 255)."""
    torch = pytest.importorskip("torch")
    got = ld.empty_scene(P, pkg, rt, torch, lights)
    assert not got["mask2"].any()
    assert (got["i32x4"] == (0, 0, 0, 255)).all() and (got["rgba8"] == 0xFF000000).all()


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
