"""rt_hit_surfaces_device / rt_light_hits_device over their whole input
domain: every case of tests/light_edges.py on the kernel (csrc/rt_light.hip),
compared with the host functions (csrc/rt_light.cpp) and with the numpy
restatement (tests/light_ref.py) under DESIGN.md §3.1a's rule: lit frames as
raw words, `triangle` exact, a normal component as raw words wherever the
restatement holds a number and NaN where it holds NaN.
tests/test_light_edges.py asserts, without a GPU, that each case contains the
classes it is in the table for; the same check runs here before any parity.

Every output sits between guard words (tests/light_device.py), and every
scene array is a slice of a larger tensor with two cubes' worth of padding on
both sides: the foreign object ids fed here are nc + ns, nc + ns + 1 and -2
only, so that even a kernel without its range check would read inside memory
the test owns.  Guards, padding and the scene arrays must come back unchanged.
"""
import numpy as np
import pytest

import light_edges as le
import light_ref as lr
from light_device import (check_scene_padding, padded_device_scene, run_device, unguard,
                          upload_hits)
from light_edges import CASES, OUTPUTS

gpu = pytest.mark.gpu
F32 = np.float32


def host(pkg, r, hits, what):
    if what == "surface":
        return pkg.hit_surfaces(hits, r.scene, rows=r.rows, ray_dir=r.d)
    return pkg.light_hits(hits, r.scene, what, rows=r.rows, ray_dir=r.d)


def rendered_hits(rt, r):
    """The case's hit frame from the trace itself (generic_kernel: the binned
    kernels take d = (0, 0, D) only), first checked against hit_ref."""
    got, t = rt.render(r.scene, r.w, r.h, rows=r.rows, fmt="hit", ray_dir=np.asarray(r.d, F32))
    assert t.path == "generic" and rt.last_kernel() == "generic_kernel", (r.name, t.path)
    assert np.array_equal(lr.words(got), lr.words(r.given)), f"{r.name}: the trace's hit frame"
    return got


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_host_and_restatement(pkg, rt, oracle, name):
    torch = pytest.importorskip("torch")
    r = le.reference(pkg, oracle, name)
    assert not le.missing_classes(r), le.missing_classes(r)
    hits = rendered_hits(rt, r) if CASES[name]["render"] else r.given
    ds, keep = padded_device_scene(torch, r.scene)
    hd = upload_hits(torch, hits)
    x0, compared = r.x_begin, []
    for what in OUTPUTS:
        buf = run_device("light", pkg, rt, torch, ds, hd, r.w, r.rows, what, r.d)
        got = unguard(torch, pkg, buf, r.w, r.rows, what)
        del buf
        # the host: the same frame, or, where it refuses the frame's ids, the
        # frame with those ids as -1
        if not r.host_ok:
            with pytest.raises(pkg.RtError) as e:
                host(pkg, r, hits, what)
            assert e.value.status == pkg.RT_ERR_INVALID_ARG
        from_host = host(pkg, r, hits if r.host_ok else r.hits, what)
        diff = le.differ(what, got, from_host)
        assert not diff, f"{name} {what} device vs host: {diff}"
        want = {"surface": r.surf, "i32x4": r.lit, "rgba8": r.rgba8}[what]
        diff = le.differ(what, got[:, x0:], want)
        assert not diff, f"{name} {what} device vs restatement: {diff}"
        compared.append(what)
        del got, from_host
    assert tuple(compared) == OUTPUTS
    check_scene_padding(torch, r.scene, keep)
    # the input is read only
    assert np.array_equal(hd.cpu().numpy().view(np.uint32), lr.words(hits))
    del keep, hd
