"""rt_shadow_hits_accel_device / rt_bounce_hits_accel_device /
rt_light_hits_mirrored_accel_device on the GPU: the kernels
(csrc/rt_light_accel.hip, csrc/rt_shadow_accel.hip) against the host functions, culled
(csrc/rt_light_accel.cpp) and unculled (csrc/rt_light.cpp), which
tests/test_light_accel.py, tests/test_shadow_hits.py and
tests/test_mirror_hits.py pin to each other and to the numpy restatements.

The harness is tests/light_device.py's: for the length of a test its "shadow"
and "mirror" passes are the culled calls (the `culled` fixture), so every
comparison, guard word and padding check of the unculled passes' tests runs on
the culled kernels.  The records are built on the device by
rt_accel_build_device into guarded words; they, the hit frame and the padded
scene must come back unchanged.  Frames are compared as raw 32-bit words with
the host's unculled call; the host's culled call must give the same words.
"""
import numpy as np
import pytest

import light_device as ld
import light_ref as lr
import mirror_ref as mr
import rays_ref as yr
import reflect_ref as rr
import test_gpu_rays as tg
import test_light_accel as ta
from gpu_support import H, W, device_scene
from hit_ref import K_FAR, REF_DIR
from light_device import Extras, Pass, compare_all
from light_ref import eq

gpu = pytest.mark.gpu
F32 = np.float32
RECORD_WORDS = 80  # 320 bytes


def agree(culled, want, what):
    assert culled.dtype == want.dtype and not eq(culled, want), f"host culled {what}"
    return want


def culled_passes(pkg):
    """tests/light_device.py's "shadow" and "mirror" passes over the culled
    calls.  Device: the records' address travels in the scene dict ("accel").
    Host: the unculled call's frame, after the culled call gave the same."""
    def dev(args):
        return args[:2] + (args[1]["accel"],) + args[2:]

    def mask_host(pkg, args, kw, x):
        accel = pkg.build_accel(args[1])
        return agree(pkg.shadow_hits_accel(*args, accel, **kw), pkg.shadow_hits(*args, **kw), "mask")

    def shadowed_host(pkg, args, kw, what, x):
        accel = pkg.build_accel(args[1])
        return agree(pkg.light_hits_mirrored_accel(*args, accel, None, 0, what, True, **kw),
                     pkg.light_hits(*args, what, shadows=True, **kw), what)

    def bounce_host(pkg, args, kw, x):
        accel = pkg.build_accel(args[1])
        return agree(pkg.bounce_hits_accel(*args, accel, x.depth, **kw),
                     pkg.bounce_hits(*args, x.depth, **kw), "bounce")

    def mirrored_host(pkg, args, kw, what, x):
        accel = pkg.build_accel(args[1])
        return agree(pkg.light_hits_mirrored_accel(*args, accel, x.refl, x.depth, what, x.shadows,
                                                   **kw),
                     pkg.light_hits_mirrored(*args, x.refl, x.depth, what, x.shadows, **kw), what)

    return {
        "shadow": Pass(
            "mask", False,
            lambda rt, args, kw, x: rt.shadow_hits_accel_device(*dev(args), **kw),
            lambda rt, args, kw, what, x: rt.light_hits_mirrored_accel_device(
                *dev(args), 0, 0, fmt=what, shadows=True, **kw),
            mask_host, shadowed_host),
        "mirror": Pass(
            "bounce", True,
            lambda rt, args, kw, x: rt.bounce_hits_accel_device(*dev(args), x.depth, **kw),
            lambda rt, args, kw, what, x: rt.light_hits_mirrored_accel_device(
                *dev(args), x.refl, x.depth, fmt=what, shadows=x.shadows, **kw),
            bounce_host, mirrored_host),
    }


@pytest.fixture
def culled(pkg, rt, monkeypatch):
    """The culled passes in place of light_device's, and scene uploads that
    build the records on the device; at the end every record buffer holds the
    host's bytes between intact guards."""
    torch = pytest.importorskip("torch")
    built = []

    def with_records(upload):
        def wrapped(torch_, scene):
            ds, keep = upload(torch_, scene)
            n = scene.num_cubes
            buf, ptr = tg.guarded_words(torch_, RECORD_WORDS * n)
            torch_.cuda.synchronize()
            rt.build_accel_device(ds, ptr if n else 0)
            ds["accel"], ds["accel_owner"] = (ptr if n else 0), buf
            built.append((buf, pkg.build_accel(scene).tobytes()))
            assert tg.body_words(torch_, buf).tobytes() == built[-1][1], "records"
            return ds, keep
        return wrapped

    for name, p in culled_passes(pkg).items():
        monkeypatch.setitem(ld.PASSES, name, p)
    monkeypatch.setattr(ld, "device_scene", with_records(ld.device_scene))
    monkeypatch.setattr(ld, "padded_device_scene", with_records(ld.padded_device_scene))
    yield torch
    for buf, want in built:
        assert tg.body_words(torch, buf).tobytes() == want, "records after"


def both(pkg, rt, torch, scene, ds, hits, w, rows, label="", refl=None, depths=ld.DEPTHS,
         bounces=ld.DEPTHS, **kw):
    """Every output of the three culled calls: {("mask" | lit, 0, True), ...}."""
    got = compare_all("shadow", pkg, rt, torch, scene, ds, hits, w, rows, label=label + " shadow",
                      **kw)
    if refl is None and scene.num_cubes + scene.num_spheres:
        refl = mr.mixed(scene)
    got.update(compare_all("mirror", pkg, rt, torch, scene, ds, hits, w, rows, label=label,
                           refl=refl, depths=depths, bounces=bounces, **kw))
    return got


# --- 1. the scenes ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["chain", "corridor", "wave", "many"])
def test_the_scenes(pkg, rt, oracle, culled, name):
    """The three scenes of the mirror chain (wave: chains of one wave end at
    different levels, at depth 8 too) and 70 cubes + 70 spheres."""
    torch = culled
    scene, key, w, h, refl = ta.scenes(pkg)[name]
    hits = lr.cached_hits(oracle, key, scene, w, h)
    ds, keep = ld.device_scene(torch, scene)
    got = both(pkg, rt, torch, scene, ds, hits, w, (0, h), label=name, refl=refl)
    if name == "many":
        nc = scene.num_cubes
        mask, obj = got["mask"], got["bounce", 1, False]["object"]
        assert (mask != 0).sum() >= 50 and ((obj >= 0) & (obj < nc)).sum() >= 50
        assert (got["i32x4", 2, True] != got["i32x4", 2, False]).any(-1).sum() >= 50
    if name == "corridor":
        assert (got["bounce", 8, False]["object"] >= 0).sum() >= 64
    if name == "wave":
        mr.wave_facts(mr.restated(oracle, key, scene, w, h)[1])
    del keep


# --- 2. grid edges ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", [(1, 1), (257, 3), (83, 31)], ids=["1x1", "257x3", "83x31"])
def test_partial_waves_and_workgroups(pkg, rt, oracle, culled, w, h):
    """Pixel counts that are no multiple of 64 or 256 (1, 771, 2573); 257 x 3
    is a band of a 257 x 80 frame."""
    torch = culled

    def facts(scene, hits, rows):
        if (w, h) != (1, 1):
            assert (pkg.bounce_hits(hits, scene, 2, rows=rows)["object"] >= 0).sum() > 5

    for p, runs in (("shadow", lambda scene: [{}]),
                    ("mirror", lambda scene: [dict(refl=mr.mixed(scene)),
                                              dict(refl=np.ones_like(mr.mixed(scene)),
                                                   label=" mirrors", depths=(8,), bounces=())])):
        ld.partial_waves_and_workgroups(p, pkg, rt, torch, oracle, w, h,
                                        (rr.lone_pixel_scene(pkg), "reflect_lone_pixel"),
                                        lr.THREE_LIGHTS, facts, runs=runs)


@gpu
def test_a_lone_hit_pixel(pkg, rt, oracle, culled):
    """One hit pixel in a frame of misses: one lane of one wave walks."""
    torch = culled
    scene = ta.many(pkg)
    hits = np.array(lr.cached_hits(oracle, ta.MANY_KEY, scene, W, H))
    ys, xs = np.nonzero((hits["object"] >= 0) & (hits["object"] < scene.num_cubes))
    keep_at = (ys[len(ys) // 2], xs[len(ys) // 2])
    lone = np.empty_like(hits)
    lone["t"], lone["object"] = K_FAR, -1
    lone[keep_at] = hits[keep_at]
    ds, keep = ld.device_scene(torch, scene)
    got = both(pkg, rt, torch, scene, ds, lone, W, (0, H), label="lone",
               refl=np.ones(scene.num_cubes + scene.num_spheres, F32), depths=(8,), bounces=(1, 8))
    assert (got["bounce", 1, False]["object"] >= 0).sum() <= 1
    del keep


# --- 3. waves by what their lanes keep ------------------------------------------------------
def kept_per_pixel(pkg, oracle, scene, key, w, h):
    """Per pixel of the host trace: the cubes its level-1 bounce keeps, the
    cubes its shadow segment keeps (the scene's first light), and the former
    with the pixel's own cube not left out (-1 where there is no ray)."""
    hits, r = rr.restated(oracle, key, scene, w, h)
    accel = pkg.build_accel(scene)
    rays, on = yr.bounce_rays(hits, r)
    bounce = np.full(hits.shape, -1, np.int32)
    bounce[on] = pkg.accel_kept(rays, scene, accel, segment=False)
    free = rays.copy()
    free["skip"] = -1
    with_own = np.full(hits.shape, -1, np.int32)
    with_own[on] = pkg.accel_kept(free, scene, accel, segment=False)
    segs, where = yr.facing_segments(oracle, scene, hits, 0)
    segment = np.full(hits.shape, -1, np.int32)
    segment[where] = pkg.accel_kept(segs, scene, accel, segment=True)
    return hits, bounce, segment, with_own


@gpu
def test_waves_by_what_their_lanes_keep(pkg, rt, oracle, culled):
    """A 64-wide frame: every row is a wave.  The frame is the host trace's
    with pixels made misses, so that of four rows' hit lanes: (a) none keeps a
    cube for its bounce or its segment; (b) exactly one lane keeps one; (c)
    every lane keeps one for its bounce; (d) lanes on a cube keep no cube but
    their own.  Every other row is misses.  Then the whole frame over a scene
    with always-kept (NaN, infinite) cubes beside culling ones.  (Chains that
    end at different levels of one wave: the wave scene of test_the_scenes.)"""
    torch = culled
    w, h = 64, H
    scene = lr.with_lights(pkg.Scene.synthetic(w, h, 70, 70, seed=13, k=0.3), lr.ONE_LIGHT)
    nc = scene.num_cubes
    full, kb, ks, own = kept_per_pixel(pkg, oracle, scene, "light_accel_waves", w, h)
    hit = full["object"] >= 0
    none = hit & (kb == 0) & (ks <= 0)
    some = hit & ((kb >= 1) | (ks >= 1))
    alone = hit & (full["object"] < nc) & (kb == 0) & (own == 1) & (ks <= 0)
    row_a = int(none.sum(1).argmax())
    row_c = int((hit & (kb >= 1)).sum(1).argmax())
    rows_b = [y for y in np.argsort(-none.sum(1)) if some[y].any() and y not in (row_a, row_c)]
    rows_d = [y for y in np.argsort(-alone.sum(1)) if y not in (row_a, row_c, rows_b[0])]
    row_b, row_d = int(rows_b[0]), int(rows_d[0])
    assert none[row_a].sum() >= 8 and none[row_b].sum() >= 8
    assert (hit & (kb >= 1))[row_c].sum() >= 32 and alone[row_d].sum() >= 4
    shown = np.zeros(hit.shape, bool)
    shown[row_a] = none[row_a]
    shown[row_b] = none[row_b]
    shown[row_b, int(np.nonzero(some[row_b])[0][0])] = True
    shown[row_c] = hit[row_c] & (kb[row_c] >= 1)
    shown[row_d] = alone[row_d]
    hits = np.array(full)
    hits["t"][~shown], hits["object"][~shown] = K_FAR, -1
    # what the rows hold, from the kept counts of the frame that is launched
    kept = np.maximum(kb, ks)
    assert (kept[row_a][shown[row_a]] == 0).all()
    assert (kept[row_b][shown[row_b]] >= 1).sum() == 1
    assert (kb[row_c][shown[row_c]] >= 1).all()
    assert (own[row_d][shown[row_d]] == 1).all() and (kept[row_d][shown[row_d]] == 0).all()
    mirrors = np.ones(nc + scene.num_spheres, F32)
    ds, keep = ld.device_scene(torch, scene)
    got = both(pkg, rt, torch, scene, ds, hits, w, (0, h), label="waves", refl=mirrors,
               depths=(1, 8), bounces=(1, 8))
    obj = got["bounce", 1, False]["object"]
    assert ((obj[row_a] >= nc) | (obj[row_a] == -1)).all()  # no cube without a kept cube
    assert (obj[row_d][shown[row_d]] != full["object"][row_d][shown[row_d]]).all()
    assert (obj[~shown] == -1).all()
    del keep
    # always-kept cubes beside culling ones, on the whole frame
    odd = ta.odd(pkg, scene)
    accel = pkg.build_accel(odd)
    assert (accel["emax2"][1:3] == np.inf).all()
    rays, on = yr.bounce_rays(full, rr.restated(oracle, "light_accel_waves", scene, w, h)[1])
    k = pkg.accel_kept(rays, odd, accel)
    assert (k >= 1).all() and k.mean() < nc / 2
    ds, keep = ld.device_scene(torch, odd)
    both(pkg, rt, torch, odd, ds, full, w, (0, h), label="always kept", refl=mirrors,
         depths=(2,), bounces=(2,))
    del keep


# --- 4. foreign frames ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["ids", "t"])
def test_foreign_frames(pkg, rt, oracle, culled, kind):
    """Ids just outside [-1, nc + ns) (the host refuses the frame; with those
    ids as -1 it gives what the kernels give) and foreign t, on padded scenes
    with a padded reflectivity array; the padding is checked afterwards."""
    torch = culled

    def mirror_facts(got, outside):
        assert (got["bounce", 1, False]["object"][outside] == -1).all()

    def shadow_facts(got, outside):
        assert not got["mask"][outside].any()
    ld.foreign_frames("mirror", pkg, rt, torch, oracle, kind, mirror_facts, refl=mr.mixed)
    ld.foreign_frames("shadow", pkg, rt, torch, oracle, kind, shadow_facts)


# --- 5. nothing to cull, nothing to light --------------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", [[], lr.ONE_LIGHT], ids=["no_lights", "one_light"])
def test_empty_scene(pkg, rt, culled, lights):
    """NULL scene arrays, a zero accel_ptr and a NULL reflectivity array."""
    torch = culled
    got = ld.empty_scene("mirror", pkg, rt, torch, lights, refl=None)
    assert (got["bounce", 8, False]["object"] == -1).all()
    assert (got["i32x4", 8, True] == (0, 0, 0, 255)).all()
    got = ld.empty_scene("shadow", pkg, rt, torch, lights)
    assert not got["mask"].any()


@gpu
@pytest.mark.parametrize("name", ["no_cubes", "no_lights"])
def test_degenerate_scenes(pkg, rt, oracle, culled, name):
    """Spheres alone with a zero accel_ptr; the 70 + 70 scene without lights."""
    torch = culled
    big = ta.many(pkg)
    hits = lr.cached_hits(oracle, ta.MANY_KEY, big, W, H)
    if name == "no_cubes":
        scene = pkg.Scene(big.sphere_origins, big.sphere_radius, big.sphere_colours,
                          lights=big.lights)
        given = np.array(hits)
        cube = given["object"] < big.num_cubes
        given["object"] = np.where(cube, -1, given["object"] - big.num_cubes)
        given["t"][cube & (hits["object"] >= 0)] = K_FAR
    else:
        scene, given = lr.with_lights(big, []), hits
    ds, keep = ld.device_scene(torch, scene)
    assert (ds["accel"] == 0) == (name == "no_cubes")
    got = both(pkg, rt, torch, scene, ds, given, W, (0, H), label=name, depths=(2,), bounces=(2,))
    assert (got["bounce", 2, False]["object"] >= 0).sum() >= 20
    if name == "no_lights":
        assert not got["mask"].any()
    del keep


@gpu
def test_33_lights_are_refused_by_the_mask_call(pkg, rt, culled):
    torch = culled
    scene = lr.with_lights(lr.base(pkg), [(i, 5, 60, 1) for i in range(33)])
    hits = np.empty((4, 64), pkg.HIT_DTYPE)
    hits["t"], hits["object"] = K_FAR, -1
    ds, keep = ld.device_scene(torch, scene)
    hd = ld.upload_hits(torch, hits)
    with pytest.raises(pkg.RtError) as e:
        ld.run_device("shadow", pkg, rt, torch, ds, hd, 64, (0, 4), "mask")
    assert e.value.status == pkg.RT_ERR_UNSUPPORTED
    buf = ld.run_device("mirror", pkg, rt, torch, ds, hd, 64, (0, 4), "bounce", depth=2)
    assert (ld.unguard(torch, pkg, buf, 64, (0, 4), "bounce")["object"] == -1).all()
    del keep


# --- 6. one stream ---------------------------------------------------------------------------------
@gpu
def test_trace_build_mask_bounce_light_on_one_stream(pkg, rt, oracle):
    """render_device(fmt="hit"), rt_accel_build_device and the three culled
    calls back to back on one non-default stream, one synchronise at the end:
    the host pipeline gives the same frames."""
    torch = pytest.importorskip("torch")
    scene = ta.many(pkg)
    n_slots = scene.num_cubes + scene.num_spheres
    refl = mr.mixed(scene)
    hits_ref = lr.cached_hits(oracle, ta.MANY_KEY, scene, W, H)
    ds, keep = device_scene(torch, scene)
    refl_ptr, keep_refl = ld.upload_reflectivity(torch, refl)
    records, ds["accel"] = tg.guarded_words(torch, RECORD_WORDS * scene.num_cubes)
    hd = torch.full((H, W, 2), ld.PATTERN, dtype=torch.int32, device="cuda:0")
    calls = [("shadow", "mask", Extras()), ("mirror", "bounce", Extras(refl_ptr, 2)),
             ("mirror", "i32x4", Extras(refl_ptr, 3, True)),
             ("mirror", "rgba8", Extras(refl_ptr, 8, False))]
    passes = culled_passes(pkg)
    torch.cuda.synchronize()  # uploads and fills are done before the stream starts
    stream = torch.cuda.Stream()
    bufs = []
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        rt.render_device(ds, W, H, (0, H), hd.data_ptr(), ray_dir=np.array(REF_DIR, F32),
                         fmt="hit", stream=st)
        rt.build_accel_device(ds, ds["accel"], stream=st)
        for p, what, x in calls:
            buf = torch.full((2 * ld.GUARD + W * H * ld.KINDS[what][0],), ld.PATTERN,
                             dtype=torch.int32, device="cuda:0")
            args = (hd.data_ptr(), ds, W, (0, H), buf.data_ptr() + 4 * ld.GUARD)
            kw = dict(ray_dir=REF_DIR, stream=st)
            if what in ld.LIT:
                passes[p].device_lit(rt, args, kw, what, x)
            else:
                passes[p].device(rt, args, kw, x)
            bufs.append(buf)
    stream.synchronize()
    assert np.array_equal(hd.cpu().numpy().view(np.uint32), lr.words(hits_ref))
    accel = pkg.build_accel(scene)
    assert tg.body_words(torch, records).tobytes() == accel.tobytes()
    assert n_slots == 140
    for (p, what, x), buf in zip(calls, bufs):
        got = ld.unguard(torch, pkg, buf, W, (0, H), what)
        x = x._replace(refl=refl)
        args, kw = (hits_ref, scene), dict(rows=(0, H), ray_dir=REF_DIR)
        want = passes[p].host_lit(pkg, args, kw, what, x) if what in ld.LIT else \
            passes[p].host(pkg, args, kw, x)
        assert not eq(got, want), f"{p} {what}: {eq(got, want)}"
    del keep, keep_refl


# --- 7. the pixel index ------------------------------------------------------------------------------
@gpu
def test_256_primitives(pkg, rt, culled):
    """18 cubes and 40 spheres at 96 x 80, the whole frame up to its last
    pixel, three lights, a random reflectivity per object, depth 3."""
    torch = culled
    refl = np.random.default_rng(11).random(58).astype(F32)
    refl[::7] = 0  # some matte

    def facts(scene, hits, got):
        assert (pkg.bounce_hits(hits, scene, 3)["object"] >= 0).sum() > 20
        assert got["i32x4", 3, True].shape == (H, W, 4)
    ld.many_primitives("mirror", pkg, rt, torch, facts, refl=refl, depths=(3,), bounces=(3,))
    ld.many_primitives("shadow", pkg, rt, torch, lambda scene, hits, got: None)
