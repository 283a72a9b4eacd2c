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

import light_device as ld
import light_ref as lr
import reflect_ref as rr
import shadow_ref as sr
from gpu_support import device_scene
from hit_ref import K_FAR
from light_device import (PASSES, check_scene_padding, compare_all, padded_device_scene,
                          run_device, unguard, upload_hits)
from light_ref import ONE_LIGHT, THREE_LIGHTS, eq

P = "reflect"  # this file's pass of tests/light_device.py
OUTPUTS = PASSES[P].outputs

gpu = pytest.mark.gpu


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
@gpu
@pytest.mark.parametrize("w,h", [(1, 1), (257, 3), (83, 31)], ids=["1x1", "257x3", "83x31"])
def test_partial_waves_and_workgroups(pkg, rt, oracle, w, h):
    """Pixel counts that are no multiple of 64 or 256 (1, 771, 2573)."""
    torch = pytest.importorskip("torch")

    def facts(scene, hits, rows):
        o2 = pkg.reflect_hits(hits, scene, rows=rows)["object"]
        assert o2[0, 0] == scene.num_cubes + 1 if (w, h) == (1, 1) else (o2 >= 0).sum() > 5
    ld.partial_waves_and_workgroups(P, pkg, rt, torch, oracle, w, h,
                                    (rr.lone_pixel_scene(pkg), "reflect_lone_pixel"), ONE_LIGHT,
                                    facts)


# --- 4. trace, then the mirrored light, on one stream ------------------------------------------
@gpu
def test_trace_then_reflected_light_on_one_stream(pkg, rt, oracle):
    """render_device(fmt="hit") and the three reflect calls back to back on a
    non-default stream, no host synchronisation in between: the host pipeline
    (hit_ref, then the host functions) gives the same frames."""
    torch = pytest.importorskip("torch")

    def facts(p, what, got):
        assert what != "bounce" or (got["object"] >= 0).sum() > 300
    ld.trace_then_calls_on_one_stream(pkg, rt, torch, oracle,
                                      [(P, what, ld.Extras()) for what in OUTPUTS], facts)


# --- 5. many candidates through the scalar loops ---------------------------------------------------
@gpu
def test_256_occluders(pkg, rt):
    """18 cubes and 40 spheres: 256 primitives, three lights."""
    torch = pytest.importorskip("torch")

    def facts(scene, hits, got):
        o2 = got["bounce"]["object"]
        assert (o2 >= 0).sum() > 50 and len(np.unique(o2)) > 5
    ld.many_primitives(P, pkg, rt, torch, facts)


# --- 6. foreign frames -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["ids", "t"])
def test_foreign_frames(pkg, rt, oracle, kind):
    """Ids just outside [-1, nc + ns) (the host refuses the frame; with those
    ids as -1 it gives what the kernel gives) and foreign t, on padded scenes."""
    torch = pytest.importorskip("torch")

    def facts(got, outside):
        o2 = got["bounce"]["object"]
        assert (o2[outside] == -1).all() and (got["bounce"]["t"][outside] == K_FAR).all()
        assert (o2 >= 0).sum() > 300
    ld.foreign_frames(P, pkg, rt, torch, oracle, kind, facts)


# --- 7. numeric edges ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", rr.EDGE_NAMES)
def test_numeric_edges(pkg, rt, oracle, name):
    torch = pytest.importorskip("torch")
    scene, w, h, d, key = rr.edge_cases(pkg)[name]
    ld.compare_scene(P, pkg, rt, torch, oracle, key, scene, w, h, d, label=name)


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
    got = ld.compare_scene(P, pkg, rt, torch, oracle, key, scene, 64, 48, label=name)
    if name == "sphere_tie":
        y, x = rr.TIE_PIXEL
        assert got["bounce"]["object"][y, x] == 0
    if name == "twins":
        assert not (got["bounce"]["object"] == 1).any()


# --- 8. nothing to mirror ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", [[], ONE_LIGHT], ids=["no_lights", "one_light"])
def test_empty_scene(pkg, rt, lights):
    """NULL scene arrays, with and without lights: (300000, -1), (0, 0, 0, 255)."""
    torch = pytest.importorskip("torch")
    got = ld.empty_scene(P, pkg, rt, torch, lights)
    assert (got["bounce"]["object"] == -1).all() and (got["bounce"]["t"] == K_FAR).all()
    assert (got["i32x4"] == (0, 0, 0, 255)).all() and (got["rgba8"] == 0xFF000000).all()


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
