"""The guarded-tensor harness of the light pass's GPU tests, for all four of
its passes (light, shadow, reflect, shadow_reflect) -- TEST INFRASTRUCTURE ONLY.

Device memory is torch tensors.  Every output sits inside a larger tensor
pre-filled with a pattern, and the words around it must come back unchanged.
Importing this module needs no GPU, no torch and no library: `torch` is an
argument wherever it is used.
"""
import numpy as np

from gpu_support import SCENE_ARRAYS, device_scene
from hit_ref import REF_DIR
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


class Pass:
    """One pass of the light pass: its three outputs (its own kind, then the
    two lit formats), whether its lit calls take a reflectivity, and its four
    calls.  `args`: the positional arguments all calls of the kind share;
    `kw`: ray_dir / stream (device) or rows / ray_dir (host)."""

    def __init__(self, own, refl, device, device_lit, host, host_lit):
        self.outputs, self.refl = (own,) + LIT, refl
        self.device, self.device_lit, self.host, self.host_lit = device, device_lit, host, host_lit


PASSES = {
    "light": Pass(
        "surface", False,
        lambda rt, args, kw: rt.hit_surfaces_device(*args, **kw),
        lambda rt, args, kw, what, r: rt.light_hits_device(*args, fmt=what, **kw),
        lambda pkg, args, kw: pkg.hit_surfaces(*args, **kw),
        lambda pkg, args, kw, what, r: pkg.light_hits(*args, what, **kw)),
    "shadow": Pass(
        "mask", False,
        lambda rt, args, kw: rt.shadow_hits_device(*args, **kw),
        lambda rt, args, kw, what, r: rt.light_hits_device(*args, fmt=what, shadows=True, **kw),
        lambda pkg, args, kw: pkg.shadow_hits(*args, **kw),
        lambda pkg, args, kw, what, r: pkg.light_hits(*args, what, shadows=True, **kw)),
    "reflect": Pass(
        "bounce", True,
        lambda rt, args, kw: rt.reflect_hits_device(*args, **kw),
        lambda rt, args, kw, what, r: rt.light_hits_reflected_device(*args, r, fmt=what, **kw),
        lambda pkg, args, kw: pkg.reflect_hits(*args, **kw),
        lambda pkg, args, kw, what, r: pkg.light_hits_reflected(*args, r, what, **kw)),
    "shadow_reflect": Pass(
        "mask2", True,
        lambda rt, args, kw: rt.shadow_hits_reflected_device(*args, **kw),
        lambda rt, args, kw, what, r: rt.light_hits_reflected_device(*args, r, fmt=what,
                                                                     shadows=True, **kw),
        lambda pkg, args, kw: pkg.shadow_hits_reflected(*args, **kw),
        lambda pkg, args, kw, what, r: pkg.light_hits_shadowed_reflected(*args, r, what, **kw)),
}
OUTPUTS = PASSES["light"].outputs  # (tests/light_edges.py runs every case on these)


def run_device(p, pkg, rt, torch, ds, hits_dev, w, rows, what, d=REF_DIR, stream=None,
               refl=REFLECTIVITY):
    """One device call of pass `p` into a guarded tensor; returns the tensor.
    `rows`: (row_begin, row_end).  Asynchronous when `stream` is given."""
    n = (rows[1] - rows[0]) * w
    buf = torch.full((2 * GUARD + n * KINDS[what][0],), PATTERN, dtype=torch.int32,
                     device="cuda:0")
    out_ptr = buf.data_ptr() + 4 * GUARD
    assert out_ptr % 16 == 0 and hits_dev.data_ptr() % 8 == 0
    st = stream or 0  # 0: the context's own stream, which does not wait for torch's
    if not st:
        torch.cuda.synchronize()  # the fill above and the caller's uploads are done
    args, kw = (hits_dev.data_ptr(), ds, w, rows, out_ptr), dict(ray_dir=d, stream=st)
    if what in LIT:
        PASSES[p].device_lit(rt, args, kw, what, refl)
    else:
        assert what == PASSES[p].outputs[0]
        PASSES[p].device(rt, args, kw)
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


def host_result(p, pkg, hits, scene, rows, what, d=REF_DIR, refl=REFLECTIVITY):
    args, kw = (hits, scene), dict(rows=rows, ray_dir=d)
    if what in LIT:
        return PASSES[p].host_lit(pkg, args, kw, what, refl)
    assert what == PASSES[p].outputs[0]
    return PASSES[p].host(pkg, args, kw)


def compare_all(p, pkg, rt, torch, scene, ds, hits, w, rows, d=REF_DIR, label="", host_hits=None,
                outputs=None, refls=(REFLECTIVITY, 1.0)):
    """The three outputs of pass `p` (or `outputs`; the lit ones at every
    reflectivity of `refls` where the pass takes one) of `hits` on the device
    (scene `ds`, as device_scene or padded_device_scene made it; None: uploaded
    here) against the host functions on `host_hits` (default `hits`).  The hit
    frame must come back unchanged.  Returns the device results by name (the
    lit ones at refls[0])."""
    if ds is None:
        ds, keep = device_scene(torch, scene)
    hd = upload_hits(torch, hits)
    ref_hits = hits if host_hits is None else host_hits
    out = {}
    for what in (PASSES[p].outputs if outputs is None else outputs):
        for refl in (refls if PASSES[p].refl and what in LIT else refls[:1]):
            buf = run_device(p, pkg, rt, torch, ds, hd, w, rows, what, d, refl=refl)
            got = unguard(torch, pkg, buf, w, rows, what)
            want = host_result(p, pkg, ref_hits, scene, rows, what, d, refl)
            assert got.dtype == want.dtype and not eq(got, want), \
                f"{label} {what} r={refl}: {eq(got, want)}"
            out.setdefault(what, got)
    assert np.array_equal(hd.cpu().numpy().view(np.uint32), words(hits)), f"{label}: hit frame"
    return out


def padded_device_scene(torch, scene):
    """device_scene with every array a slice of a larger tensor: SCENE_PAD
    words of SCENE_PAD_VALUE in front of it and behind it, so that an index one
    or two elements outside an array still reads memory the test owns.
    Returns (dict for the *_device calls, the padded tensors by name)."""
    keep = {}
    for k in SCENE_ARRAYS:
        a = np.array(getattr(scene, k), F32).reshape(-1)
        if a.size:
            pad = np.full(SCENE_PAD, SCENE_PAD_VALUE, F32)
            keep[k] = torch.from_numpy(np.concatenate([pad, a, pad])).to("cuda:0")
    ds = {k: v.data_ptr() + 4 * SCENE_PAD for k, v in keep.items()}
    assert all(p % 16 == 0 for p in ds.values())
    ds.update(num_spheres=scene.num_spheres, num_cubes=scene.num_cubes,
              num_lights=len(scene.lights))
    return ds, keep


def check_scene_padding(torch, scene, keep):
    """The padding of a padded_device_scene and the arrays between it are as
    uploaded: the kernels write nothing there."""
    torch.cuda.synchronize()
    for k, t in keep.items():
        a = t.cpu().numpy()
        assert (a[:SCENE_PAD] == SCENE_PAD_VALUE).all(), k
        assert (a[-SCENE_PAD:] == SCENE_PAD_VALUE).all(), k
        want = np.array(getattr(scene, k), F32).reshape(-1)
        assert np.array_equal(a[SCENE_PAD:-SCENE_PAD].view(np.uint32), want.view(np.uint32)), k
