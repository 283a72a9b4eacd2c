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

import light_edges as le
import light_ref as lr
import mirror_ref as mr
import shadow_reflect_ref as srr
from gpu_support import H, SCENE_ARRAYS, W, device_scene
from hit_ref import K_FAR, REF_DIR
from light_device import (GUARD, KINDS, PATTERN, SCENE_PAD, SCENE_PAD_VALUE, check_scene_padding,
                          padded_device_scene, run_device, unguard, upload_hits)
from light_ref import ONE_LIGHT, THREE_LIGHTS, base, eq
from test_gpu_reflect_hits import lone_pixel_scene
from test_mirror_hits import chain_facts, corridor_facts, mixed, restated, wave_facts

gpu = pytest.mark.gpu
F32 = np.float32
DEPTHS = (1, 2, 8)


def upload_reflectivity(torch, refl, padded=False):
    """(device address, the tensor that holds it).  `padded`: SCENE_PAD words
    of SCENE_PAD_VALUE on both sides, as light_device.padded_device_scene."""
    a = np.asarray(refl, F32).reshape(-1)
    if padded:
        pad = np.full(SCENE_PAD, SCENE_PAD_VALUE, F32)
        t = torch.from_numpy(np.concatenate([pad, a, pad])).to("cuda:0")
        return t.data_ptr() + 4 * SCENE_PAD, t
    t = torch.from_numpy(np.concatenate([a, np.zeros(1, F32)])).to("cuda:0")  # (never empty)
    return t.data_ptr(), t


def check_reflectivity_padding(torch, refl, tensor):
    torch.cuda.synchronize()
    a = tensor.cpu().numpy()
    assert (a[:SCENE_PAD] == SCENE_PAD_VALUE).all() and (a[-SCENE_PAD:] == SCENE_PAD_VALUE).all()
    want = np.asarray(refl, F32).reshape(-1)
    assert np.array_equal(a[SCENE_PAD:-SCENE_PAD].view(np.uint32), want.view(np.uint32))


def run_mirror(rt, torch, ds, hits_dev, w, rows, what, refl_ptr=0, depth=1, shadows=False,
               d=REF_DIR, stream=None):
    """One device call into a guarded tensor; returns the tensor.  `what`:
    "bounce" (`depth`: the bounce's number), "i32x4" or "rgba8".  Asynchronous
    when `stream` is given."""
    n = (rows[1] - rows[0]) * w
    buf = torch.full((2 * GUARD + n * KINDS[what][0],), PATTERN, dtype=torch.int32,
                     device="cuda:0")
    out_ptr = buf.data_ptr() + 4 * GUARD
    assert out_ptr % 16 == 0 and hits_dev.data_ptr() % 8 == 0
    st = stream or 0  # 0: the context's own stream, which does not wait for torch's
    if not st:
        torch.cuda.synchronize()  # the fill above and the caller's uploads are done
    if what == "bounce":
        rt.bounce_hits_device(hits_dev.data_ptr(), ds, w, rows, out_ptr, depth, ray_dir=d,
                              stream=st)
    else:
        rt.light_hits_mirrored_device(hits_dev.data_ptr(), ds, w, rows, out_ptr, refl_ptr, depth,
                                      ray_dir=d, stream=st, fmt=what, shadows=shadows)
    return buf


def compare_mirror(pkg, rt, torch, scene, ds, hits, w, rows, refl, d=REF_DIR, label="",
                   host_hits=None, host_refl=None, refl_dev=None, depths=DEPTHS,
                   bounces=(1, 2, 8)):
    """The bounce frames and, at every depth, shadows off and on, both lit
    formats of `hits` on the device (scene `ds`; reflectivity `refl`, or what
    `refl_dev` = (address, tensor) holds) against the host functions on
    `host_hits` / `host_refl` (default: the same).  The hit frame must come
    back unchanged.  Returns the device results by (what, depth, shadows)."""
    hd = upload_hits(torch, hits)
    refl_ptr, keep = refl_dev if refl_dev is not None else upload_reflectivity(torch, refl)
    ref_hits = hits if host_hits is None else host_hits
    ref_refl = refl if host_refl is None else host_refl
    out = {}
    for b in bounces:
        got = unguard(torch, pkg, run_mirror(rt, torch, ds, hd, w, rows, "bounce", depth=b, d=d),
                      w, rows, "bounce")
        want = pkg.bounce_hits(ref_hits, scene, b, rows=rows, ray_dir=d)
        assert got.dtype == want.dtype and not eq(got, want), f"{label} bounce {b}: {eq(got, want)}"
        out["bounce", b, False] = got
    for depth in depths:
        for shadows in (False, True):
            for what in ("i32x4", "rgba8"):
                buf = run_mirror(rt, torch, ds, hd, w, rows, what, refl_ptr, depth, shadows, d)
                got = unguard(torch, pkg, buf, w, rows, what)
                want = pkg.light_hits_mirrored(ref_hits, scene, ref_refl, depth, what, shadows,
                                               rows=rows, ray_dir=d)
                assert got.dtype == want.dtype and not eq(got, want), \
                    f"{label} {what} depth={depth} shadows={shadows}: {eq(got, want)}"
                out[what, depth, shadows] = got
    assert np.array_equal(hd.cpu().numpy().view(np.uint32), lr.words(hits)), f"{label}: hit frame"
    del keep
    return out


# --- 1. the three scenes ---------------------------------------------------------------------
SCENES = {
    "chain": (mr.chain_scene, mr.CHAIN_KEY, mr.CHAIN_W, mr.CHAIN_H, mr.CHAIN_REFLECTIVITY,
              chain_facts),
    "corridor": (mr.corridor_scene, "mirror_corridor", mr.CORRIDOR_W, mr.CORRIDOR_H,
                 mr.CORRIDOR_REFLECTIVITY, corridor_facts),
    "wave": (mr.wave_scene, "mirror_wave", mr.WAVE_W, mr.WAVE_H, mr.WAVE_REFLECTIVITY, wave_facts),
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
    hits, c = restated(oracle, key, scene, w, h)
    facts(c)
    ds, keep = device_scene(torch, scene)
    got = compare_mirror(pkg, rt, torch, scene, ds, hits, w, (0, h), refl, label=name)
    if name == "chain":
        assert (got["i32x4", 1, False] != got["i32x4", 2, False]).any(-1).sum() >= 100
    if name == "corridor":
        assert (got["bounce", 8, False]["object"] >= 0).sum() >= 64
    del keep


# --- 2. grid edges -------------------------------------------------------------------------
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
        assert pkg.bounce_hits(hits, scene, 1)["object"][0, 0] == scene.num_cubes + 1
    else:
        # (257 x 3: rows 40..42 of a 257 x 80 frame, where the base scene's objects are)
        rows = (40, 43) if h == 3 else (0, h)
        scene = lr.with_lights(base(pkg), THREE_LIGHTS)
        hits = lr.cached_hits(oracle, "base", scene, w, H if h == 3 else h, rows)
        assert (pkg.bounce_hits(hits, scene, 2, rows=rows)["object"] >= 0).sum() > 5
    ds, keep = device_scene(torch, scene)
    compare_mirror(pkg, rt, torch, scene, ds, hits, w, rows, mixed(scene), label=f"{w}x{h}")
    compare_mirror(pkg, rt, torch, scene, ds, hits, w, rows, np.ones_like(mixed(scene)),
                   label=f"{w}x{h} mirrors", depths=(8,), bounces=())
    del keep


# --- 3. behind the trace, on one stream ------------------------------------------------------
@gpu
def test_trace_then_bounce_then_mirrored_light_on_one_stream(pkg, rt, oracle):
    """render_device(fmt="hit"), rt_bounce_hits_device and
    rt_light_hits_mirrored_device back to back on a non-default stream with no
    host synchronisation in between: the host pipeline gives the same frames."""
    torch = pytest.importorskip("torch")
    scene = lr.with_lights(base(pkg), THREE_LIGHTS)
    hits_ref = lr.cached_hits(oracle, "base", scene, W, H)
    refl = mixed(scene)
    ds, keep = device_scene(torch, scene)
    refl_ptr, keep_refl = upload_reflectivity(torch, refl)
    hd = torch.full((H, W, 2), PATTERN, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()  # uploads and fills are done before the stream starts
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rt.render_device(ds, W, H, (0, H), hd.data_ptr(), ray_dir=np.array(REF_DIR, F32),
                         fmt="hit", stream=stream.cuda_stream)
        bounce = run_mirror(rt, torch, ds, hd, W, (0, H), "bounce", depth=2,
                            stream=stream.cuda_stream)
        lit = {(what, shadows): run_mirror(rt, torch, ds, hd, W, (0, H), what, refl_ptr, 3,
                                           shadows, stream=stream.cuda_stream)
               for what in ("i32x4", "rgba8") for shadows in (False, True)}
    stream.synchronize()
    assert np.array_equal(hd.cpu().numpy().view(np.uint32), lr.words(hits_ref))
    got = unguard(torch, pkg, bounce, W, (0, H), "bounce")
    assert not eq(got, pkg.bounce_hits(hits_ref, scene, 2)) and (got["object"] >= 0).sum() > 100
    for (what, shadows), buf in lit.items():
        got = unguard(torch, pkg, buf, W, (0, H), what)
        want = pkg.light_hits_mirrored(hits_ref, scene, refl, 3, what, shadows)
        assert not eq(got, want), f"{what} shadows={shadows}: {eq(got, want)}"
    del keep, keep_refl


# --- 4. many occluders and candidates through the scalar loops -----------------------------------
@gpu
def test_256_primitives(pkg, rt):
    """18 cubes and 40 spheres: 256 primitives, three lights, a random
    reflectivity per object, depth 3."""
    torch = pytest.importorskip("torch")
    scene = lr.with_lights(pkg.Scene.synthetic(W, H, 40, 18, seed=11, k=0.3), THREE_LIGHTS)
    assert 12 * scene.num_cubes + scene.num_spheres == 256
    refl = np.random.default_rng(11).random(58).astype(F32)
    refl[::7] = 0  # some matte
    hits, _ = rt.render(scene, W, H, fmt="hit", ray_dir=REF_DIR)
    assert (pkg.bounce_hits(hits, scene, 3)["object"] >= 0).sum() > 20
    ds, keep = device_scene(torch, scene)
    compare_mirror(pkg, rt, torch, scene, ds, hits, W, (0, H), refl, label="256 primitives",
                   depths=(3,), bounces=(3,))
    del keep


# --- 5. foreign frames and arrays -----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["ids", "t"])
def test_foreign_frames(pkg, rt, oracle, kind):
    """Ids just outside [-1, nc + ns) (the host refuses the frame; with those
    ids as -1 it gives what the kernel gives) and foreign t, on padded scenes
    with a padded reflectivity array."""
    torch = pytest.importorskip("torch")
    scene = lr.with_lights(base(pkg), THREE_LIGHTS)
    valid = lr.cached_hits(oracle, "base", scene, W, H)
    given, counts = (le.foreign_ids if kind == "ids" else le.foreign_t)(valid, scene)
    assert len(counts) == (9 if kind == "ids" else 14) and min(counts.values()) >= 4
    obj = given["object"]
    n_slots = scene.num_cubes + scene.num_spheres
    refl = mixed(scene)
    outside = (obj < -1) | (obj >= n_slots)
    mapped = np.array(given)
    mapped["object"][outside] = -1
    if kind == "ids":
        assert outside.sum() == 36 and set(np.unique(obj[outside])) == {-2, n_slots, n_slots + 1}
        for call in (lambda: pkg.bounce_hits(given, scene, 2),
                     lambda: pkg.light_hits_mirrored(given, scene, refl, 2)):
            with pytest.raises(pkg.RtError) as e:
                call()
            assert e.value.status == pkg.RT_ERR_INVALID_ARG
    else:
        assert not outside.any()
        # t == 300000 beside a real object: the bounce frame walks, the lit frame does not
        assert ((given["t"] == K_FAR) & (obj >= 0)).sum() >= 8
    ds, keep = padded_device_scene(torch, scene)
    refl_dev = upload_reflectivity(torch, refl, padded=True)
    got = compare_mirror(pkg, rt, torch, scene, ds, given, W, (0, H), refl,
                         label=f"foreign {kind}", host_hits=mapped, refl_dev=refl_dev)
    assert (got["bounce", 1, False]["object"][outside] == -1).all()
    check_scene_padding(torch, scene, keep)
    check_reflectivity_padding(torch, refl, refl_dev[1])
    del keep, refl_dev


@gpu
def test_reflectivities_outside_0_1_read_as_0(pkg, rt, oracle):
    """1.5, -0.25, NaN and inf at slots the chains meet: the host refuses the
    array; with those slots 0 it gives what the kernel gives."""
    torch = pytest.importorskip("torch")
    scene = mr.chain_scene(pkg)
    w, h = mr.CHAIN_W, mr.CHAIN_H
    hits, c = restated(oracle, mr.CHAIN_KEY, scene, w, h)
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
    refl_dev = upload_reflectivity(torch, given, padded=True)
    compare_mirror(pkg, rt, torch, scene, ds, hits, w, (0, h), given, label="outside [0, 1]",
                   host_refl=cleaned, refl_dev=refl_dev, bounces=())
    check_reflectivity_padding(torch, given, refl_dev[1])
    del keep, refl_dev


# --- 6. nothing to light ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", [[], ONE_LIGHT], ids=["no_lights", "one_light"])
def test_empty_scene(pkg, rt, lights):
    """NULL scene arrays and a NULL reflectivity array, with and without
    lights: (300000, -1), (0, 0, 0, 255)."""
    torch = pytest.importorskip("torch")
    scene = lr.with_lights(pkg.Scene(), lights)
    w, h = 70, 9
    hits = np.empty((h, w), pkg.HIT_DTYPE)
    hits["t"], hits["object"] = K_FAR, -1
    ds, keep = device_scene(torch, scene)
    assert not any(ds.get(k) for k in SCENE_ARRAYS[:5]) and ds["num_lights"] == len(lights)
    got = compare_mirror(pkg, rt, torch, scene, ds, hits, w, (0, h), None, label="empty",
                         refl_dev=(0, None))
    assert (got["bounce", 8, False]["object"] == -1).all()
    assert (got["i32x4", 8, True] == (0, 0, 0, 255)).all()
    assert (got["rgba8", 8, True] == 0xFF000000).all()
    del keep


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
    for r in (0.25, 1.0, 0.0, -0.0):
        refl_ptr, keep_refl = upload_reflectivity(torch, np.full(slots, r, F32))
        for what in ("i32x4", "rgba8"):
            for shadows, p in ((False, "reflect"), (True, "shadow_reflect")):
                want = unguard(torch, pkg, run_device(p, pkg, rt, torch, ds, hd, w, (0, h), what,
                                                      refl=r), w, (0, h), what)
                got = unguard(torch, pkg, run_mirror(rt, torch, ds, hd, w, (0, h), what, refl_ptr,
                                                     1, shadows), w, (0, h), what)
                assert not eq(got, want), f"{what} r={r} shadows={shadows}: {eq(got, want)}"
        del keep_refl
    want = unguard(torch, pkg, run_device("reflect", pkg, rt, torch, ds, hd, w, (0, h), "bounce"),
                   w, (0, h), "bounce")
    got = unguard(torch, pkg, run_mirror(rt, torch, ds, hd, w, (0, h), "bounce", depth=1),
                  w, (0, h), "bounce")
    assert not eq(got, want) and (got["object"] >= 0).sum() > 300
    del keep
