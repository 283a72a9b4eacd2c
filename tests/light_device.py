"""The guarded-tensor harness of the light pass's GPU tests -- TEST
INFRASTRUCTURE ONLY.

Device memory is torch tensors.  Every output sits inside a larger tensor
pre-filled with a pattern, and the words around it must come back unchanged.
Importing this module needs no GPU, no torch and no library: `torch` is an
argument wherever it is used.
"""
import numpy as np

from gpu_support import SCENE_ARRAYS, device_scene
from hit_ref import REF_DIR
from light_ref import eq

F32 = np.float32
PATTERN = 0x5A5A5A5A
GUARD = 64  # int32 words in front of and behind every device output (256 B)
WORDS = {"surface": 4, "i32x4": 4, "rgba8": 1}
OUTPUTS = ("surface", "i32x4", "rgba8")
# float words on both sides of every array of a padded scene: two cubes' worth
# (2 x 36 float4), which is more than two elements of every other array
SCENE_PAD = 2 * 144
SCENE_PAD_VALUE = F32(-7.25)  # a finite number no scene of the tests holds


def run_device(pkg, rt, torch, ds, hits_dev, w, rows, what, d=REF_DIR, stream=None):
    """One device call into a guarded tensor; returns the tensor.  `rows`:
    (row_begin, row_end).  Asynchronous when `stream` is given."""
    n = (rows[1] - rows[0]) * w
    buf = torch.full((2 * GUARD + n * WORDS[what],), PATTERN, dtype=torch.int32, device="cuda:0")
    out_ptr = buf.data_ptr() + 4 * GUARD
    assert out_ptr % 16 == 0 and hits_dev.data_ptr() % 8 == 0
    st = stream or 0  # 0: the context's own stream, which does not wait for torch's
    if not st:
        torch.cuda.synchronize()  # the fill above and the caller's uploads are done
    if what == "surface":
        rt.hit_surfaces_device(hits_dev.data_ptr(), ds, w, rows, out_ptr, ray_dir=d, stream=st)
    else:
        rt.light_hits_device(hits_dev.data_ptr(), ds, w, rows, out_ptr, ray_dir=d, stream=st,
                             fmt=what)
    return buf


def unguard(torch, pkg, buf, w, rows, what):
    """The host copy of a run_device tensor, guards checked and removed."""
    torch.cuda.synchronize()  # every stream, the context's own included
    a = buf.cpu().numpy().view(np.uint32)
    assert (a[:GUARD] == PATTERN).all() and (a[-GUARD:] == PATTERN).all(), "wrote out of bounds"
    body, n = a[GUARD:-GUARD], rows[1] - rows[0]
    if what == "surface":
        return body.view(pkg.SURFACE_DTYPE).reshape(n, w)
    return body.view(np.int32).reshape(n, w, 4) if what == "i32x4" else body.reshape(n, w)


def upload_hits(torch, hits):
    return torch.from_numpy(np.array(hits).view(np.int32).reshape(hits.shape + (2,))).to("cuda:0")


def host_result(pkg, hits, scene, rows, what, d=REF_DIR):
    if what == "surface":
        return pkg.hit_surfaces(hits, scene, rows=rows, ray_dir=d)
    return pkg.light_hits(hits, scene, what, rows=rows, ray_dir=d)


def compare_all(pkg, rt, torch, scene, hits, w, rows, d=REF_DIR, label=""):
    """Surfaces and both lit formats of `hits` on the device against the host."""
    ds, keep = device_scene(torch, scene)
    hd = upload_hits(torch, hits)
    out = {}
    for what in OUTPUTS:
        buf = run_device(pkg, rt, torch, ds, hd, w, rows, what, d)
        got = unguard(torch, pkg, buf, w, rows, what)
        want = host_result(pkg, hits, scene, rows, what, d)
        assert not eq(got, want), f"{label} {what}: {eq(got, want)}"
        out[what] = got
    del keep
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
