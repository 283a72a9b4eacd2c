"""rt_shadow_hits_device / rt_light_hits_shadowed_device on the GPU: the kernel
(csrc/rt_shadow.hip) against the host functions (csrc/rt_light.cpp), which
tests/test_shadow_hits.py pins to the numpy restatement (tests/shadow_ref.py).

Device memory is torch tensors; every output sits between guard words
(tests/light_device.py), and the guard words and
the hit frame must come back unchanged.  Frames are compared as raw 32-bit
words.
"""
import numpy as np
import pytest

import light_device as ld
import light_ref as lr
import shadow_ref as sr
from gpu_support import device_scene
from light_device import PASSES, check_scene_padding, compare_all, padded_device_scene
from light_ref import ONE_LIGHT, eq

P = "shadow"  # this file's pass of tests/light_device.py
OUTPUTS = PASSES[P].outputs

gpu = pytest.mark.gpu


# --- 1. the four occluder / receiver kinds ------------------------------------------
@gpu
@pytest.mark.parametrize("padded", [False, True], ids=["plain", "padded"])
def test_the_four_kinds(pkg, rt, oracle, padded):
    torch = pytest.importorskip("torch")
    scene = sr.kinds_scene(pkg)
    w, h = sr.KINDS_W, sr.KINDS_H
    hits = lr.cached_hits(oracle, "shadow_kinds", scene, w, h)
    ds, keep = (padded_device_scene if padded else device_scene)(torch, scene)
    got = compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), label="kinds")
    assert (got["mask"] == 1).sum() > 1000 and set(np.unique(got["mask"]).tolist()) == {0, 1}
    if padded:
        check_scene_padding(torch, scene, keep)
    del keep


# --- 2. wave-level paths ------------------------------------------------------------------
@gpu
def test_wave_level_paths(pkg, rt, oracle):
    """Waves wholly in the shadow (every lane leaves the walk at the sphere:
    the ballot exit), wholly outside it (the full walk) and across its rim (a
    partial pending set)."""
    torch = pytest.importorskip("torch")
    scene = sr.wave_scene(pkg)
    w = h = 128
    hits = lr.cached_hits(oracle, "shadow_wave", scene, w, h)
    assert (hits["object"] == 0).all()
    r = sr.shadow_ref(oracle, scene, hits)
    full, none, mixed = sr.segments(r.mask != 0)  # the restatement: 61, 106, 89
    assert full >= 30 and none >= 30 and mixed >= 10
    ds, keep = device_scene(torch, scene)
    got = compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), label="waves")
    assert np.array_equal(got["mask"], r.mask) and not eq(got["i32x4"], r.lit)
    del keep


# --- 3. grid edges -------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", [(1, 1), (257, 3), (83, 31)], ids=["1x1", "257x3", "83x31"])
def test_partial_waves_and_workgroups(pkg, rt, oracle, w, h):
    """Pixel counts that are no multiple of 64 or 256 (1, 771, 2573)."""
    torch = pytest.importorskip("torch")

    def facts(scene, hits, rows):
        mask = pkg.shadow_hits(hits, scene)
        assert mask[0, 0] == 1 if (w, h) == (1, 1) else (mask != 0).sum() > 5
    ld.partial_waves_and_workgroups(P, pkg, rt, torch, oracle, w, h,
                                    (sr.lone_pixel_scene(pkg), "shadow_lone_pixel"), ONE_LIGHT,
                                    facts, band=False)


# --- 4. trace, then shadowed light, on one stream ---------------------------------------------
@gpu
def test_trace_then_shadowed_light_on_one_stream(pkg, rt, oracle):
    """render_device(fmt="hit") and the three shadow calls back to back on a
    non-default stream, no host synchronisation in between: the host pipeline
    (hit_ref, then the host functions) gives the same frames."""
    torch = pytest.importorskip("torch")

    def facts(p, what, got):
        assert what != "mask" or (got != 0).sum() > 20
    ld.trace_then_calls_on_one_stream(pkg, rt, torch, oracle,
                                      [(P, what, ld.Extras()) for what in OUTPUTS], facts)


# --- 5. many occluders through the scalar loop ---------------------------------------------------
@gpu
def test_256_occluders(pkg, rt):
    """18 cubes and 40 spheres: 256 occluder primitives, three lights."""
    torch = pytest.importorskip("torch")

    def facts(scene, hits, got):
        assert (got["mask"] != 0).sum() > 50 and len(np.unique(got["mask"])) > 2
    ld.many_primitives(P, pkg, rt, torch, facts, label="256 occluders")


# --- 6. foreign frames -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["ids", "t"])
def test_foreign_frames(pkg, rt, oracle, kind):
    """Ids just outside [-1, nc + ns) (the host refuses the frame; with those
    ids as -1 it gives what the kernel gives) and foreign t, on padded scenes."""
    torch = pytest.importorskip("torch")

    def facts(got, outside):
        assert (got["mask"][outside] == 0).all() and (got["mask"] != 0).sum() > 20
    ld.foreign_frames(P, pkg, rt, torch, oracle, kind, facts)


# --- 7. numeric edges ------------------------------------------------------------------------------
EDGE_NAMES = sorted(sr.EDGE_LIGHTS) + ["p_inside_a_sphere", "minus_inf", "nan_colour"]


@gpu
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_numeric_edges(pkg, rt, oracle, name):
    torch = pytest.importorskip("torch")
    _, scene, w, h, d = {c[0]: c for c in sr.edge_cases(pkg)}[name]
    key = "shadow_kinds" if name in sr.EDGE_LIGHTS else "shadow_edge_" + name
    ld.compare_scene(P, pkg, rt, torch, oracle, key, scene, w, h, d, label=name)


# --- 8. nothing to occlude --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", [[], ONE_LIGHT], ids=["no_lights", "one_light"])
def test_empty_scene(pkg, rt, lights):
    """NULL scene arrays, with and without lights: mask 0, (0, 0, 0, 255)."""
    torch = pytest.importorskip("torch")
    got = ld.empty_scene(P, pkg, rt, torch, lights)
    assert not got["mask"].any()
    assert (got["i32x4"] == (0, 0, 0, 255)).all() and (got["rgba8"] == 0xFF000000).all()
