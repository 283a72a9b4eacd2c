"""The guarded-tensor harness of tests/light_device.py for the three outputs of
the shadowed, mirrored light pass -- TEST INFRASTRUCTURE ONLY.  Importing this
module needs no GPU, no torch and no library.
"""
import numpy as np

from hit_ref import REF_DIR
from light_device import GUARD, PATTERN, upload_hits
from light_ref import eq, words

WORDS = {"mask2": 1, "i32x4": 4, "rgba8": 1}
OUTPUTS = ("mask2", "i32x4", "rgba8")
REFLECTIVITY = 0.25


def run_shadow_reflect_device(pkg, rt, torch, ds, hits_dev, w, rows, what, d=REF_DIR, stream=None,
                              refl=REFLECTIVITY):
    """One device call into a guarded tensor; returns the tensor.  `rows`:
    (row_begin, row_end).  Asynchronous when `stream` is given."""
    n = (rows[1] - rows[0]) * w
    buf = torch.full((2 * GUARD + n * WORDS[what],), PATTERN, dtype=torch.int32, device="cuda:0")
    out_ptr = buf.data_ptr() + 4 * GUARD
    assert out_ptr % 16 == 0 and hits_dev.data_ptr() % 8 == 0
    st = stream or 0  # 0: the context's own stream, which does not wait for torch's
    if not st:
        torch.cuda.synchronize()  # the fill above and the caller's uploads are done
    if what == "mask2":
        rt.shadow_hits_reflected_device(hits_dev.data_ptr(), ds, w, rows, out_ptr, ray_dir=d,
                                        stream=st)
    else:
        rt.light_hits_reflected_device(hits_dev.data_ptr(), ds, w, rows, out_ptr, refl, ray_dir=d,
                                       stream=st, fmt=what, shadows=True)
    return buf


def unguard(torch, buf, w, rows, what):
    """The host copy of a run_shadow_reflect_device tensor, guards checked and removed."""
    torch.cuda.synchronize()  # every stream, the context's own included
    a = buf.cpu().numpy().view(np.uint32)
    assert (a[:GUARD] == PATTERN).all() and (a[-GUARD:] == PATTERN).all(), "wrote out of bounds"
    body, n = a[GUARD:-GUARD], rows[1] - rows[0]
    return body.view(np.int32).reshape(n, w, 4) if what == "i32x4" else body.reshape(n, w)


def host_result(pkg, hits, scene, rows, what, d=REF_DIR, refl=REFLECTIVITY):
    if what == "mask2":
        return pkg.shadow_hits_reflected(hits, scene, rows=rows, ray_dir=d)
    return pkg.light_hits_shadowed_reflected(hits, scene, refl, what, rows=rows, ray_dir=d)


def compare_all(pkg, rt, torch, scene, ds, hits, w, rows, d=REF_DIR, label="", host_hits=None,
                refls=(REFLECTIVITY, 1.0)):
    """The mask at p2 and both lit formats (at every reflectivity of `refls`)
    of `hits` on the device (scene `ds`, as device_scene or padded_device_scene
    made it) against the host functions on `host_hits` (default `hits`).  The
    hit frame must come back unchanged.  Returns the device results by name
    (the lit ones at refls[0])."""
    hd = upload_hits(torch, hits)
    ref_hits = hits if host_hits is None else host_hits
    out = {}
    for what in OUTPUTS:
        for refl in (refls if what != "mask2" else refls[:1]):
            buf = run_shadow_reflect_device(pkg, rt, torch, ds, hd, w, rows, what, d, refl=refl)
            got = unguard(torch, buf, w, rows, what)
            want = host_result(pkg, ref_hits, scene, rows, what, d, refl)
            assert got.dtype == want.dtype and not eq(got, want), \
                f"{label} {what} r={refl}: {eq(got, want)}"
            out.setdefault(what, got)
    assert np.array_equal(hd.cpu().numpy().view(np.uint32), words(hits)), f"{label}: hit frame"
    return out
