"""The guarded-tensor harness of the light pass's GPU tests, for all five of
its passes (light, shadow, reflect, shadow_reflect, mirror), and the test
bodies their files share -- TEST INFRASTRUCTURE ONLY.

Device memory is torch tensors.  Every output sits inside a larger tensor
pre-filled with a pattern, and the words around it must come back unchanged.
Importing this module needs no GPU, no torch and no library: `torch` is an
argument wherever it is used.
"""
from collections import namedtuple

import numpy as np
import pytest

import light_ref as lr
from gpu_support import H, SCENE_ARRAYS, W, device_scene
from hit_ref import K_FAR, REF_DIR
from light_ref import eq, words

F32 = np.float32
PATTERN = 0x5A5A5A5A
GUARD = 64  # int32 words in front of and behind every device output (256 B)
# float words on both sides of every array of a padded scene: two cubes' worth
# (2 x 36 float4), which is more than two elements of every other array
SCENE_PAD = 2 * 144
SCENE_PAD_VALUE = F32(-7.25)  # a finite number no scene of the tests holds
REFLECTIVITY = 0.25
# every output kind: (int32 words per pixel, the package's name of its
# structured dtype or None for plain words)
KINDS = {"surface": (4, "SURFACE_DTYPE"), "mask": (1, None), "bounce": (2, "HIT_DTYPE"),
         "mask2": (1, None), "i32x4": (4, None), "rgba8": (1, None)}
LIT = ("i32x4", "rgba8")
DEPTHS = (1, 2, 8)  # of the mirror pass's comparisons, and its bounce numbers

# What a call takes beyond the frame.  refl: the reflect passes' reflectivity;
# for the mirror pass the array (host) or its device address.  depth: the
# mirror pass's max_bounces, or the number of the bounce frame.  shadows: the
# mirror pass's flag.
Extras = namedtuple("Extras", "refl depth shadows", defaults=(REFLECTIVITY, 1, False))


class Pass:
    """One pass of the light pass: its three outputs (its own kind, then the
    two lit formats), whether its lit calls take a reflectivity, and its four
    calls.  `args`: the positional arguments all calls of the kind share;
    `kw`: ray_dir / stream (device) or rows / ray_dir (host); `x`: Extras."""

    def __init__(self, own, refl, device, device_lit, host, host_lit):
        self.outputs, self.refl = (own,) + LIT, refl
        self.device, self.device_lit, self.host, self.host_lit = device, device_lit, host, host_lit


PASSES = {
    "light": Pass(
        "surface", False,
        lambda rt, args, kw, x: rt.hit_surfaces_device(*args, **kw),
        lambda rt, args, kw, what, x: rt.light_hits_device(*args, fmt=what, **kw),
        lambda pkg, args, kw, x: pkg.hit_surfaces(*args, **kw),
        lambda pkg, args, kw, what, x: pkg.light_hits(*args, what, **kw)),
    "shadow": Pass(
        "mask", False,
        lambda rt, args, kw, x: rt.shadow_hits_device(*args, **kw),
        lambda rt, args, kw, what, x: rt.light_hits_device(*args, fmt=what, shadows=True, **kw),
        lambda pkg, args, kw, x: pkg.shadow_hits(*args, **kw),
        lambda pkg, args, kw, what, x: pkg.light_hits(*args, what, shadows=True, **kw)),
    "reflect": Pass(
        "bounce", True,
        lambda rt, args, kw, x: rt.reflect_hits_device(*args, **kw),
        lambda rt, args, kw, what, x: rt.light_hits_reflected_device(*args, x.refl, fmt=what, **kw),
        lambda pkg, args, kw, x: pkg.reflect_hits(*args, **kw),
        lambda pkg, args, kw, what, x: pkg.light_hits_reflected(*args, x.refl, what, **kw)),
    "shadow_reflect": Pass(
        "mask2", True,
        lambda rt, args, kw, x: rt.shadow_hits_reflected_device(*args, **kw),
        lambda rt, args, kw, what, x: rt.light_hits_reflected_device(*args, x.refl, fmt=what,
                                                                     shadows=True, **kw),
        lambda pkg, args, kw, x: pkg.shadow_hits_reflected(*args, **kw),
        lambda pkg, args, kw, what, x: pkg.light_hits_shadowed_reflected(*args, x.refl, what, **kw)),
    "mirror": Pass(
        "bounce", True,
        lambda rt, args, kw, x: rt.bounce_hits_device(*args, x.depth, **kw),
        lambda rt, args, kw, what, x: rt.light_hits_mirrored_device(
            *args, x.refl, x.depth, fmt=what, shadows=x.shadows, **kw),
        lambda pkg, args, kw, x: pkg.bounce_hits(*args, x.depth, **kw),
        lambda pkg, args, kw, what, x: pkg.light_hits_mirrored(*args, x.refl, x.depth, what,
                                                               x.shadows, **kw)),
}
OUTPUTS = PASSES["light"].outputs  # (tests/light_edges.py runs every case on these)


def run_device(p, pkg, rt, torch, ds, hits_dev, w, rows, what, d=REF_DIR, stream=None,
               refl=REFLECTIVITY, depth=1, shadows=False):
    """One device call of pass `p` into a guarded tensor; returns the tensor.
    `rows`: (row_begin, row_end).  `refl`, `depth`, `shadows`: see Extras (the
    mirror pass's `refl` is a device address here).  Asynchronous when
    `stream` is given."""
    n = (rows[1] - rows[0]) * w
    buf = torch.full((2 * GUARD + n * KINDS[what][0],), PATTERN, dtype=torch.int32,
                     device="cuda:0")
    out_ptr = buf.data_ptr() + 4 * GUARD
    assert out_ptr % 16 == 0 and hits_dev.data_ptr() % 8 == 0
    st = stream or 0  # 0: the context's own stream, which does not wait for torch's
    if not st:
        torch.cuda.synchronize()  # the fill above and the caller's uploads are done
    args, kw = (hits_dev.data_ptr(), ds, w, rows, out_ptr), dict(ray_dir=d, stream=st)
    x = Extras(refl, depth, shadows)
    if what in LIT:
        PASSES[p].device_lit(rt, args, kw, what, x)
    else:
        assert what == PASSES[p].outputs[0]
        PASSES[p].device(rt, args, kw, x)
    return buf


def unguard(torch, pkg, buf, w, rows, what):
    """The host copy of a run_device tensor, guards checked and removed."""
    torch.cuda.synchronize()  # every stream, the context's own included
    a = buf.cpu().numpy().view(np.uint32)
    assert (a[:GUARD] == PATTERN).all() and (a[-GUARD:] == PATTERN).all(), "wrote out of bounds"
    body, n = a[GUARD:-GUARD], rows[1] - rows[0]
    if KINDS[what][1]:
        return body.view(getattr(pkg, KINDS[what][1])).reshape(n, w)
    return body.view(np.int32).reshape(n, w, 4) if what == "i32x4" else body.reshape(n, w)


def upload_hits(torch, hits):
    return torch.from_numpy(np.array(hits).view(np.int32).reshape(hits.shape + (2,))).to("cuda:0")


def host_result(p, pkg, hits, scene, rows, what, d=REF_DIR, refl=REFLECTIVITY, depth=1,
                shadows=False):
    args, kw, x = (hits, scene), dict(rows=rows, ray_dir=d), Extras(refl, depth, shadows)
    if what in LIT:
        return PASSES[p].host_lit(pkg, args, kw, what, x)
    assert what == PASSES[p].outputs[0]
    return PASSES[p].host(pkg, args, kw, x)


def settings(p, what, refl, refls, depths, bounces):
    """The Extras at which compare_all takes output `what` of pass `p`."""
    if p == "mirror":
        if what not in LIT:
            return [Extras(refl, b) for b in bounces]
        return [Extras(refl, depth, shadows) for depth in depths for shadows in (False, True)]
    return [Extras(r) for r in (refls if PASSES[p].refl and what in LIT else refls[:1])]


def compare_all(p, pkg, rt, torch, scene, ds, hits, w, rows, d=REF_DIR, label="", host_hits=None,
                outputs=None, refls=(REFLECTIVITY, 1.0), refl=None, host_refl=None, refl_dev=None,
                depths=DEPTHS, bounces=DEPTHS):
    """The three outputs of pass `p` (or `outputs`) of `hits` on the device
    (scene `ds`, as device_scene or padded_device_scene made it; None: uploaded
    here) against the host functions on `host_hits` (default `hits`).  The lit
    ones: at every reflectivity of `refls` where the pass takes one.  The
    mirror pass: the bounce frames `bounces` and the lit ones at every depth of
    `depths`, shadows off and on, with the reflectivity array `refl` (or what
    `refl_dev` = (address, tensor) holds) against the host's on `host_refl`
    (default `refl`).  The hit frame must come back unchanged.  Returns the
    device results by name (the lit ones at refls[0]), the mirror pass's by
    (name, depth or bounce, shadows)."""
    if ds is None:
        ds, keep = device_scene(torch, scene)
    hd = upload_hits(torch, hits)
    ref_hits = hits if host_hits is None else host_hits
    if p == "mirror":
        refl_ptr, keep_refl = refl_dev if refl_dev is not None else upload_reflectivity(torch, refl)
        ref_refl = refl if host_refl is None else host_refl
    out = {}
    for what in (PASSES[p].outputs if outputs is None else outputs):
        for x in settings(p, what, refl, refls, depths, bounces):
            on_dev, on_host = (x._replace(refl=refl_ptr), x._replace(refl=ref_refl)) \
                if p == "mirror" else (x, x)
            buf = run_device(p, pkg, rt, torch, ds, hd, w, rows, what, d, None, *on_dev)
            got = unguard(torch, pkg, buf, w, rows, what)
            want = host_result(p, pkg, ref_hits, scene, rows, what, d, *on_host)
            at = f"depth={x.depth} shadows={x.shadows}" if p == "mirror" else f"r={x.refl}"
            assert got.dtype == want.dtype and not eq(got, want), \
                f"{label} {what} {at}: {eq(got, want)}"
            out.setdefault((what, x.depth, x.shadows) if p == "mirror" else what, got)
    assert np.array_equal(hd.cpu().numpy().view(np.uint32), words(hits)), f"{label}: hit frame"
    return out


def padded_array(torch, a):
    """(device address, tensor) of the float array `a` with SCENE_PAD words of
    SCENE_PAD_VALUE in front of it and behind it, so that an index one or two
    elements outside it still reads memory the test owns."""
    pad = np.full(SCENE_PAD, SCENE_PAD_VALUE, F32)
    t = torch.from_numpy(np.concatenate([pad, np.asarray(a, F32).reshape(-1), pad])).to("cuda:0")
    assert (t.data_ptr() + 4 * SCENE_PAD) % 16 == 0
    return t.data_ptr() + 4 * SCENE_PAD, t


def check_padding(torch, a, tensor, name=""):
    """The padding of a padded_array and the array between it are as
    uploaded: the kernels write nothing there."""
    torch.cuda.synchronize()
    got = tensor.cpu().numpy()
    assert (got[:SCENE_PAD] == SCENE_PAD_VALUE).all(), name
    assert (got[-SCENE_PAD:] == SCENE_PAD_VALUE).all(), name
    want = np.asarray(a, F32).reshape(-1)
    assert np.array_equal(got[SCENE_PAD:-SCENE_PAD].view(np.uint32), want.view(np.uint32)), name


def padded_device_scene(torch, scene):
    """device_scene with every array a padded_array.  Returns (dict for the
    *_device calls, the padded tensors by name)."""
    keep, ds = {}, {}
    for k in SCENE_ARRAYS:
        if np.asarray(getattr(scene, k)).size:
            ds[k], keep[k] = padded_array(torch, getattr(scene, k))
    ds.update(num_spheres=scene.num_spheres, num_cubes=scene.num_cubes,
              num_lights=len(scene.lights))
    return ds, keep


def check_scene_padding(torch, scene, keep):
    for k, t in keep.items():
        check_padding(torch, getattr(scene, k), t, k)


def upload_reflectivity(torch, refl, padded=False):
    """(device address, the tensor that holds it) of the mirror pass's
    reflectivity array; `padded`: a padded_array."""
    if padded:
        return padded_array(torch, refl)
    if refl is None:
        return 0, None
    a = np.asarray(refl, F32).reshape(-1)
    t = torch.from_numpy(np.concatenate([a, np.zeros(1, F32)])).to("cuda:0")  # (never empty)
    return t.data_ptr(), t


# ---------------------------------------------------------------------------
# Test bodies the files of the passes share.  `facts`: the file's own
# assertions on what the frame really holds.
# ---------------------------------------------------------------------------
def compare_scene(p, pkg, rt, torch, oracle, key, scene, w, h, d=REF_DIR, label="", **compare):
    """compare_all on the whole w x h hit frame of `scene` (hit-cache `key`)."""
    hits = lr.cached_hits(oracle, key, scene, w, h, None, d)
    ds, keep = device_scene(torch, scene)
    got = compare_all(p, pkg, rt, torch, scene, ds, hits, w, (0, h), d=d, label=label, **compare)
    del keep
    return got


def partial_waves_and_workgroups(p, pkg, rt, torch, oracle, w, h, lone, lights, facts, band=True,
                                 runs=lambda scene: [{}]):
    """Pixel counts that are no multiple of 64 or 256 (1, 771, 2573).  1 x 1:
    the scene and hit-cache key `lone`; else the base scene under `lights`
    (`band`: 257 x 3 is rows 40..42 of a 257 x 80 frame, where the base
    scene's objects are).  `runs(scene)`: the keywords of each compare_all."""
    assert (w * h) % 64 and (w * h) % 256
    rows = (0, h)
    if (w, h) == (1, 1):
        scene, key = lone
        hits = lr.cached_hits(oracle, key, scene, w, h)
        assert hits["object"][0, 0] == scene.num_cubes
    else:
        rows = (40, 43) if band and h == 3 else (0, h)
        scene = lr.with_lights(lr.base(pkg), lights)
        hits = lr.cached_hits(oracle, "base", scene, w, H if rows[0] else h, rows if band else None)
    facts(scene, hits, rows)
    ds, keep = device_scene(torch, scene)
    for kw in runs(scene):
        kw = dict(kw)
        compare_all(p, pkg, rt, torch, scene, ds, hits, w, rows,
                    label=f"{w}x{h}" + kw.pop("label", ""), **kw)
    del keep


def trace_then_calls_on_one_stream(pkg, rt, torch, oracle, calls, facts, refl=None):
    """render_device(fmt="hit") and `calls` ((pass, output, Extras), in this
    order) back to back on a non-default stream, no host synchronisation in
    between: the host pipeline (hit_ref, then the host functions) gives the
    same frames.  The base scene under three lights; `refl`: the mirror
    pass's reflectivity array.  `facts(pass, output, frame)`."""
    scene = lr.with_lights(lr.base(pkg), lr.THREE_LIGHTS)
    hits_ref = lr.cached_hits(oracle, "base", scene, W, H)
    ds, keep = device_scene(torch, scene)
    refl_ptr, keep_refl = upload_reflectivity(torch, refl)
    hd = torch.full((H, W, 2), PATTERN, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()  # uploads and fills are done before the stream starts
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rt.render_device(ds, W, H, (0, H), hd.data_ptr(), ray_dir=np.array(REF_DIR, F32),
                         fmt="hit", stream=stream.cuda_stream)
        bufs = [run_device(p, pkg, rt, torch, ds, hd, W, (0, H), what, REF_DIR, stream.cuda_stream,
                           *(x._replace(refl=refl_ptr) if p == "mirror" else x))
                for p, what, x in calls]
    stream.synchronize()
    assert np.array_equal(hd.cpu().numpy().view(np.uint32), words(hits_ref))
    for (p, what, x), buf in zip(calls, bufs):
        got = unguard(torch, pkg, buf, W, (0, H), what)
        want = host_result(p, pkg, hits_ref, scene, (0, H), what, REF_DIR,
                           *(x._replace(refl=refl) if p == "mirror" else x))
        assert not eq(got, want), f"{p} {what} {x.depth} {x.shadows}: {eq(got, want)}"
        facts(p, what, got)
    del keep, keep_refl


def many_primitives(p, pkg, rt, torch, facts, label="256 primitives", **compare):
    """18 cubes and 40 spheres: 256 primitives, three lights.
    `facts(scene, hits, frames)`."""
    scene = lr.with_lights(pkg.Scene.synthetic(W, H, 40, 18, seed=11, k=0.3), lr.THREE_LIGHTS)
    assert 12 * scene.num_cubes + scene.num_spheres == 256
    hits, _ = rt.render(scene, W, H, fmt="hit", ray_dir=REF_DIR)
    ds, keep = device_scene(torch, scene)
    got = compare_all(p, pkg, rt, torch, scene, ds, hits, W, (0, H), label=label, **compare)
    facts(scene, hits, got)
    del keep


def foreign_frames(p, pkg, rt, torch, oracle, kind, facts, refl=None):
    """Ids just outside [-1, nc + ns) (the host refuses the frame; with those
    ids as -1 it gives what the kernel gives) and foreign t, on padded scenes
    (the mirror pass: with a padded reflectivity array `refl(scene)`).
    `facts(frames, outside)`."""
    import light_edges as le  # (it takes OUTPUTS from this module)
    scene = lr.with_lights(lr.base(pkg), lr.THREE_LIGHTS)
    valid = lr.cached_hits(oracle, "base", scene, W, H)
    given, counts = (le.foreign_ids if kind == "ids" else le.foreign_t)(valid, scene)
    assert len(counts) == (9 if kind == "ids" else 14) and min(counts.values()) >= 4
    obj = given["object"]
    n_slots = scene.num_cubes + scene.num_spheres
    outside = (obj < -1) | (obj >= n_slots)
    mapped = np.array(given)
    mapped["object"][outside] = -1
    mirror = dict(refl=refl(scene), depth=2) if p == "mirror" else {}
    if kind == "ids":
        assert outside.sum() == 36 and set(np.unique(obj[outside])) == {-2, n_slots, n_slots + 1}
        for what in PASSES[p].outputs:
            with pytest.raises(pkg.RtError) as e:
                host_result(p, pkg, given, scene, (0, H), what, **mirror)
            assert e.value.status == pkg.RT_ERR_INVALID_ARG
    else:
        assert not outside.any()
        # t == 300000 beside a real object: the own output walks, the lit frame does not
        assert ((given["t"] == K_FAR) & (obj >= 0)).sum() >= 8
    ds, keep = padded_device_scene(torch, scene)
    if mirror:
        mirror = dict(refl=mirror["refl"], refl_dev=padded_array(torch, mirror["refl"]))
    got = compare_all(p, pkg, rt, torch, scene, ds, given, W, (0, H), label=f"foreign {kind}",
                      host_hits=mapped, **mirror)
    facts(got, outside)
    check_scene_padding(torch, scene, keep)
    if mirror:
        check_padding(torch, mirror["refl"], mirror["refl_dev"][1], "reflectivity")
    del keep, mirror


def empty_scene(p, pkg, rt, torch, lights, **compare):
    """NULL scene arrays, with and without lights, 70 x 9 misses: the frames."""
    scene = lr.with_lights(pkg.Scene(), lights)
    w, h = 70, 9
    hits = np.empty((h, w), pkg.HIT_DTYPE)
    hits["t"], hits["object"] = K_FAR, -1
    ds, keep = device_scene(torch, scene)
    assert not any(ds.get(k) for k in SCENE_ARRAYS[:5]) and ds["num_lights"] == len(lights)
    got = compare_all(p, pkg, rt, torch, scene, ds, hits, w, (0, h), label="empty", **compare)
    del keep
    return got
