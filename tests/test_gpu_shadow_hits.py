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

import light_edges as le
import light_ref as lr
import shadow_ref as sr
from gpu_support import H, SCENE_ARRAYS, W, device_scene
from hit_ref import K_FAR, REF_DIR
from light_device import (PASSES, PATTERN, check_scene_padding, compare_all, host_result,
                          padded_device_scene, run_device, unguard)
from light_ref import ONE_LIGHT, THREE_LIGHTS, base, eq

P = "shadow"  # this file's pass of tests/light_device.py
OUTPUTS = PASSES[P].outputs

gpu = pytest.mark.gpu
F32 = np.float32


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
def lone_pixel_scene(pkg):
    """The base scene with sphere 0 moved onto pixel (0, 0), nearer than
    everything else, and sphere 1 between its hit point and the light."""
    scene = lr.with_lights(base(pkg), ONE_LIGHT)
    scene.sphere_origins[0] = (0, 0, -5, 1)
    scene.sphere_radius[0] = 3
    scene.sphere_origins[1] = (24, 20, 99, 1)  # half way from (0, 0, -2) to (48, 40, 200)
    scene.sphere_radius[1] = 5
    return scene


@gpu
@pytest.mark.parametrize("w,h", [(1, 1), (257, 3), (83, 31)], ids=["1x1", "257x3", "83x31"])
def test_partial_waves_and_workgroups(pkg, rt, oracle, w, h):
    """Pixel counts that are no multiple of 64 or 256 (1, 771, 2573)."""
    torch = pytest.importorskip("torch")
    assert (w * h) % 64 and (w * h) % 256
    if (w, h) == (1, 1):
        scene = lone_pixel_scene(pkg)
        hits = lr.cached_hits(oracle, "shadow_lone_pixel", scene, w, h)
        assert hits["object"][0, 0] == scene.num_cubes and pkg.shadow_hits(hits, scene)[0, 0] == 1
    else:
        scene = lr.with_lights(base(pkg), ONE_LIGHT)
        hits = lr.cached_hits(oracle, "base", scene, w, h)
        assert (pkg.shadow_hits(hits, scene) != 0).sum() > 5
    ds, keep = device_scene(torch, scene)
    compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), label=f"{w}x{h}")
    del keep


# --- 4. trace, then shadowed light, on one stream ---------------------------------------------
@gpu
def test_trace_then_shadowed_light_on_one_stream(pkg, rt, oracle):
    """render_device(fmt="hit") and the three shadow calls back to back on a
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
        if what == "mask":
            assert (got != 0).sum() > 20
    del keep


# --- 5. many occluders through the scalar loop ---------------------------------------------------
@gpu
def test_256_occluders(pkg, rt):
    """18 cubes and 40 spheres: 256 occluder primitives, three lights."""
    torch = pytest.importorskip("torch")
    scene = lr.with_lights(pkg.Scene.synthetic(W, H, 40, 18, seed=11, k=0.3), THREE_LIGHTS)
    assert 12 * scene.num_cubes + scene.num_spheres == 256
    hits, _ = rt.render(scene, W, H, fmt="hit", ray_dir=REF_DIR)
    ds, keep = device_scene(torch, scene)
    got = compare_all(P, pkg, rt, torch, scene, ds, hits, W, (0, H), label="256 occluders")
    assert (got["mask"] != 0).sum() > 50 and len(np.unique(got["mask"])) > 2
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
    ds, keep = padded_device_scene(torch, scene)
    got = compare_all(P, pkg, rt, torch, scene, ds, given, W, (0, H), label=f"foreign {kind}",
                      host_hits=mapped)
    assert (got["mask"][outside] == 0).all() and (got["mask"] != 0).sum() > 20
    check_scene_padding(torch, scene, keep)
    del keep


# --- 7. numeric edges ------------------------------------------------------------------------------
EDGE_NAMES = sorted(sr.EDGE_LIGHTS) + ["p_inside_a_sphere", "minus_inf", "nan_colour"]


@gpu
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_numeric_edges(pkg, rt, oracle, name):
    torch = pytest.importorskip("torch")
    _, scene, w, h, d = {c[0]: c for c in sr.edge_cases(pkg)}[name]
    key = "shadow_kinds" if name in sr.EDGE_LIGHTS else "shadow_edge_" + name
    hits = lr.cached_hits(oracle, key, scene, w, h, None, d)
    ds, keep = device_scene(torch, scene)
    compare_all(P, pkg, rt, torch, scene, ds, hits, w, (0, h), d=d, label=name)
    del keep


# --- 8. nothing to occlude --------------------------------------------------------------------------
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
    assert not got["mask"].any()
    assert (got["i32x4"] == (0, 0, 0, 255)).all() and (got["rgba8"] == 0xFF000000).all()
    del keep
