"""rt_bounce_hits_device / rt_light_hits_mirrored_device on the GPU: the kernel
(csrc/rt_mirror.hip) against the host functions (csrc/rt_light.cpp), which
tests/test_mirror_hits.py pins to the numpy restatement (tests/mirror_ref.py).

Device memory is torch tensors; every output sits between guard words
(tests/light_device.py's), and the guard words, the hit frame and, where it is
padded, the reflectivity array must come back unchanged.  Frames are compared
as raw 32-bit words; no word is masked.
"""
import numpy as np
import pytest

import light_device as ld
import light_ref as lr
import mirror_ref as mr
import reflect_ref as rr
import shadow_reflect_ref as srr
from gpu_support import device_scene
from light_device import (check_padding, compare_all, padded_array, padded_device_scene,
                          run_device, unguard, upload_hits, upload_reflectivity)
from light_ref import ONE_LIGHT, eq

P = "mirror"  # this file's pass of tests/light_device.py

gpu = pytest.mark.gpu
F32 = np.float32


# --- 1. the three scenes ---------------------------------------------------------------------
SCENES = {
    "chain": (mr.chain_scene, mr.CHAIN_KEY, mr.CHAIN_W, mr.CHAIN_H, mr.CHAIN_REFLECTIVITY,
              mr.chain_facts),
    "corridor": (mr.corridor_scene, "mirror_corridor", mr.CORRIDOR_W, mr.CORRIDOR_H,
                 mr.CORRIDOR_REFLECTIVITY, mr.corridor_facts),
    "wave": (mr.wave_scene, "mirror_wave", mr.WAVE_W, mr.WAVE_H, mr.WAVE_REFLECTIVITY,
             mr.wave_facts),
}


@gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_scenes(pkg, rt, oracle, name):
    """chain: chains of one, two and more bounces that end by a miss, a matte
    object and the depth.  corridor: level RT_MAX_BOUNCES, past the ramp's end.
    wave (64-pixel segments of a 128-wide frame are waves): waves whose chains
    all end at level 1, waves whose hit lanes all go on, and a few lanes that
    go on alone."""
    torch = pytest.importorskip("torch")
    make, key, w, h, refl, facts = SCENES[name]
    scene = make(pkg)
    facts(mr.restated(oracle, key, scene, w, h)[1])
    got = ld.compare_scene(P, pkg, rt, torch, oracle, key, scene, w, h, label=name, refl=refl)
    if name == "chain":
        assert (got["i32x4", 1, False] != got["i32x4", 2, False]).any(-1).sum() >= 100
    if name == "corridor":
        assert (got["bounce", 8, False]["object"] >= 0).sum() >= 64


# --- 2. grid edges -------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", [(1, 1), (257, 3), (83, 31)], ids=["1x1", "257x3", "83x31"])
def test_partial_waves_and_workgroups(pkg, rt, oracle, w, h):
    """Pixel counts that are no multiple of 64 or 256 (1, 771, 2573)."""
    torch = pytest.importorskip("torch")

    def facts(scene, hits, rows):
        if (w, h) == (1, 1):
            assert pkg.bounce_hits(hits, scene, 1)["object"][0, 0] == scene.num_cubes + 1
        else:
            assert (pkg.bounce_hits(hits, scene, 2, rows=rows)["object"] >= 0).sum() > 5

    def runs(scene):
        return [dict(refl=mr.mixed(scene)),
                dict(refl=np.ones_like(mr.mixed(scene)), label=" mirrors", depths=(8,), bounces=())]
    ld.partial_waves_and_workgroups(P, pkg, rt, torch, oracle, w, h,
                                    (rr.lone_pixel_scene(pkg), "reflect_lone_pixel"),
                                    lr.THREE_LIGHTS, facts, runs=runs)


# --- 3. behind the trace, on one stream ------------------------------------------------------
@gpu
def test_trace_then_bounce_then_mirrored_light_on_one_stream(pkg, rt, oracle):
    """render_device(fmt="hit"), rt_bounce_hits_device and
    rt_light_hits_mirrored_device back to back on a non-default stream with no
    host synchronisation in between: the host pipeline gives the same frames."""
    torch = pytest.importorskip("torch")
    refl = mr.mixed(lr.base(pkg))
    calls = [(P, "bounce", ld.Extras(refl, 2))]
    calls += [(P, what, ld.Extras(refl, 3, shadows)) for what in ld.LIT for shadows in (False, True)]

    def facts(p, what, got):
        assert what != "bounce" or (got["object"] >= 0).sum() > 100
    ld.trace_then_calls_on_one_stream(pkg, rt, torch, oracle, calls, facts, refl=refl)


# --- 4. many occluders and candidates through the scalar loops -----------------------------------
@gpu
def test_256_primitives(pkg, rt):
    """18 cubes and 40 spheres: 256 primitives, three lights, a random
    reflectivity per object, depth 3."""
    torch = pytest.importorskip("torch")
    refl = np.random.default_rng(11).random(58).astype(F32)
    refl[::7] = 0  # some matte

    def facts(scene, hits, got):
        assert (pkg.bounce_hits(hits, scene, 3)["object"] >= 0).sum() > 20
    ld.many_primitives(P, pkg, rt, torch, facts, refl=refl, depths=(3,), bounces=(3,))


# --- 5. foreign frames and arrays -----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["ids", "t"])
def test_foreign_frames(pkg, rt, oracle, kind):
    """Ids just outside [-1, nc + ns) (the host refuses the frame; with those
    ids as -1 it gives what the kernel gives) and foreign t, on padded scenes
    with a padded reflectivity array."""
    torch = pytest.importorskip("torch")

    def facts(got, outside):
        assert (got["bounce", 1, False]["object"][outside] == -1).all()
    ld.foreign_frames(P, pkg, rt, torch, oracle, kind, facts, refl=mr.mixed)


@gpu
def test_reflectivities_outside_0_1_read_as_0(pkg, rt, oracle):
    """1.5, -0.25, NaN and inf at slots the chains meet: the host refuses the
    array; with those slots 0 it gives what the kernel gives."""
    torch = pytest.importorskip("torch")
    scene = mr.chain_scene(pkg)
    w, h = mr.CHAIN_W, mr.CHAIN_H
    hits, c = mr.restated(oracle, mr.CHAIN_KEY, scene, w, h)
    given = np.array(mr.CHAIN_REFLECTIVITY)
    given[[2, 5, 6, 8]] = (1.5, -0.25, np.nan, np.inf)
    cleaned = np.array(given)
    cleaned[[2, 5, 6, 8]] = 0
    walks, _, _ = c.stats(mr.CHAIN_REFLECTIVITY, 8)
    for slot in (2, 5, 6, 8):  # chains go on from each of them with the scene's own array
        assert ((c.levels[0].obj == slot) & (walks >= 1)).sum() >= 100
    with pytest.raises(pkg.RtError) as e:
        pkg.light_hits_mirrored(hits, scene, given, 2)
    assert e.value.status == pkg.RT_ERR_INVALID_ARG
    assert eq(pkg.light_hits_mirrored(hits, scene, cleaned, 2),
              pkg.light_hits_mirrored(hits, scene, mr.CHAIN_REFLECTIVITY, 2))
    ds, keep = padded_device_scene(torch, scene)
    refl_dev = padded_array(torch, given)
    compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), label="outside [0, 1]", refl=given,
                host_refl=cleaned, refl_dev=refl_dev, bounces=())
    check_padding(torch, given, refl_dev[1], "reflectivity")
    del keep, refl_dev


# --- 6. nothing to light ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", [[], ONE_LIGHT], ids=["no_lights", "one_light"])
def test_empty_scene(pkg, rt, lights):
    """NULL scene arrays and a NULL reflectivity array, with and without
    lights: (300000, -1), (0, 0, 0, 255)."""
    torch = pytest.importorskip("torch")
    got = ld.empty_scene(P, pkg, rt, torch, lights, refl=None)
    assert (got["bounce", 8, False]["object"] == -1).all()
    assert (got["i32x4", 8, True] == (0, 0, 0, 255)).all()
    assert (got["rgba8", 8, True] == 0xFF000000).all()


# --- 7. the identities with the one-bounce kernels ------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", [[], srr.CLASS_LIGHTS], ids=["no_lights", "two_lights"])
def test_one_bounce_is_the_one_bounce_kernels_frame(pkg, rt, oracle, lights):
    """Depth 1 with one reflectivity everywhere: reflect_kernel's frame, with
    shadows shadow_reflect_kernel's; bounce 1: reflect_kernel's bounce frame."""
    torch = pytest.importorskip("torch")
    scene = mr.chain_scene(pkg, lights)
    w, h = mr.CHAIN_W, mr.CHAIN_H
    hits = lr.cached_hits(oracle, mr.CHAIN_KEY, scene, w, h)
    ds, keep = device_scene(torch, scene)
    hd = upload_hits(torch, hits)
    slots = scene.num_cubes + scene.num_spheres

    def frame(p, what, **extras):
        return unguard(torch, pkg, run_device(p, pkg, rt, torch, ds, hd, w, (0, h), what, **extras),
                       w, (0, h), what)
    for r in (0.25, 1.0, 0.0, -0.0):
        refl_ptr, keep_refl = upload_reflectivity(torch, np.full(slots, r, F32))
        for what in ("i32x4", "rgba8"):
            for shadows, p in ((False, "reflect"), (True, "shadow_reflect")):
                want = frame(p, what, refl=r)
                got = frame(P, what, refl=refl_ptr, depth=1, shadows=shadows)
                assert not eq(got, want), f"{what} r={r} shadows={shadows}: {eq(got, want)}"
        del keep_refl
    want, got = frame("reflect", "bounce"), frame(P, "bounce", depth=1)
    assert not eq(got, want) and (got["object"] >= 0).sum() > 300
    del keep
