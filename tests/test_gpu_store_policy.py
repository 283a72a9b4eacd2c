"""The frame stores' cache policy on the GPU (rt_debug_set_store_policy): a
policy changes how the binned trace kernels' stores are cached, never a value.

Every shipped policy, forced, through trace_bin_kernel, trace3_kernel and
trace3_split_kernel (both tile builds) in the three formats, word for word
against the oracle (hit frames: tests/hit_ref.py), on the smallest frames that
take every store form: 40 x 24 (partial tiles at the right and bottom edges:
the bounds-checked stores), a band of a 64 x 48 frame with row_begin > 0, and
1 x 1.  Then the automatic choice from the bytes in flight.  The host side of
it is tests/test_store_policy.py."""
import contextlib

import numpy as np
import pytest

from gpu_support import device_scene, diff_report, knobs, scene_from
from hit_ref import hit_ref, words

gpu = pytest.mark.gpu
POLICIES = ("default", "large")
FORMATS = ("i32x4", "rgba8", "hit")
# (width, height, rows)
FRAMES = [(40, 24, None), (64, 48, (16, 48)), (1, 1, None)]
_COARSE = dict(small_path=False, trace_bin=2)
# name: (knobs, the kernel that must run)
KERNELS = {
    "trace_bin": (dict(small_path=False, trace_bin=1), "trace_bin_kernel"),
    "trace3": (dict(_COARSE, trace_split=1), "trace3_kernel"),
    "trace3_split": (dict(_COARSE, trace_split=2), "trace3_split_kernel"),
    "trace_bin_wide": (dict(small_path=False, trace_bin=1, tile_variant=2), "trace_bin_kernel"),
    "trace3_wide": (dict(_COARSE, trace_split=1, tile_variant=2), "trace3_kernel"),
    "trace3_split_wide": (dict(_COARSE, trace_split=4, tile_variant=2), "trace3_split_kernel"),
}
_REFS = {}


def small_scene(pkg):
    """3 spheres + 1 cube.  On the 40 x 24 frame's 16 x 16 tiles: spheres 0
    and 1 overlap in tile (0, 0) (sphere 0 also covers pixel (0, 0), the
    1 x 1 frame), the cube lies in tile (1, 0), sphere 2 in tile (1, 1), and
    tiles (2, 0), (2, 1) and (0, 1) stay empty."""
    return scene_from(pkg,
                      spheres=[((4, 4, -50, 1), 7, (1, .5, .25, 255)),
                               ((9, 8, -60, 1), 4, (.1, .9, .3, 255)),
                               ((27, 20, -30, 1), 3, (.3, .2, 1, 255))],
                      cubes=[([("scale", 3, 3, 3), ("rotate", .3, .7, .1),
                               ("translate", 23, 6, -40)], (.2, .4, .9, 255))])


def reference(oracle, scene, w, h, rows, fmt):
    """The oracle's frame in `fmt`, computed once per frame and left unchanged."""
    key = (w, h, rows, fmt)
    if key not in _REFS:
        if fmt == "hit":
            r = hit_ref(oracle, scene, w, h, rows=rows)
        else:
            colour = reference(oracle, scene, w, h, rows, "i32x4") if fmt == "rgba8" \
                else oracle.trace(scene, w, h, rows=rows)
            r = oracle.pack_rgba8(colour) if fmt == "rgba8" else colour
        r.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


@contextlib.contextmanager
def store_policy(rt, policy, large_bytes=0):
    try:
        rt.store_policy(policy, large_bytes)
        yield rt
    finally:
        rt.store_policy("auto", 0)


def test_scene_has_an_empty_tile_and_an_overlap(pkg, oracle):
    scene = small_scene(pkg)
    obj = reference(oracle, scene, 40, 24, None, "hit")["object"]
    assert {1, 2} <= set(np.unique(obj[:16, :16]))  # spheres 0 and 1 (slots 1 + index)
    assert 0 in obj[:16, 16:32] and 3 in obj[16:, 16:32]  # the cube, sphere 2
    for tile in (obj[:16, 32:], obj[16:, 32:], obj[16:, :16]):
        assert (tile == -1).all()
    assert reference(oracle, scene, 1, 1, None, "hit")["object"][0, 0] == 1


@gpu
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_frames_are_identical_under_every_policy(pkg, rt, oracle, kernel):
    settings, ran = KERNELS[kernel]
    scene = small_scene(pkg)
    compared = 0
    with knobs(rt, **settings):
        for policy in POLICIES:
            with store_policy(rt, policy):
                for w, h, rows in FRAMES:
                    for fmt in FORMATS:
                        want = reference(oracle, scene, w, h, rows, fmt)
                        got, t = rt.render(scene, w, h, rows=rows, fmt=fmt)
                        where = f"{kernel} {policy} {w}x{h} rows {rows} {fmt}"
                        assert t.path == "binned" and rt.last_kernel() == ran, \
                            f"{where}: ran {rt.last_kernel()}"
                        assert rt.last_store_policy() == policy, where
                        assert got.shape == want.shape and got.dtype == want.dtype, where
                        if fmt == "hit":
                            assert (words(got) == words(want)).all(), where
                        else:
                            assert not diff_report(got, want), f"{where}: {diff_report(got, want)}"
                        compared += 1
    assert compared == len(POLICIES) * len(FRAMES) * len(FORMATS)


def covered_scene(pkg):
    """Three spheres that each cover the whole 64 x 48 frame, and a cube: a
    box overdraw of 3 frames and more, so the frame is not one of the nearly
    empty ones (overdraw below 1) that keep the default policy by themselves."""
    return scene_from(pkg,
                      spheres=[((32, 24, -90 - 10 * i, 1), 60, (1, .5, .1 * i, 255))
                               for i in range(3)],
                      cubes=[([("scale", 5, 5, 5), ("rotate", .3, .7, .1),
                               ("translate", 20, 20, -20)], (.2, .4, .9, 255))])


@gpu
def test_automatic_choice_follows_the_bytes_in_flight(pkg, oracle):
    """Two contexts rendering alternately into two buffers report the
    large-working-set policy once both buffers are among the device's recent
    targets; one context with one buffer reports the default.  The threshold
    is lowered to the two 48 KiB frames' bytes; nothing large is allocated."""
    torch = pytest.importorskip("torch")
    w, h = 64, 48
    scene = covered_scene(pkg)
    want = oracle.trace(scene, w, h)
    ds, keep = device_scene(torch, scene)
    frame_bytes = w * h * 16
    bufs = [torch.zeros((h, w, 4), dtype=torch.int32, device="cuda:0") for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    rts = [pkg.RayTracer(0) for _ in range(2)]
    try:
        for r in rts:
            r.set_small_path(False)
            r.set_trace_bin(1)
            r.store_policy("auto", 2 * frame_bytes)

        def render(i):
            rts[i].render_device(ds, w, h, (0, h), bufs[i].data_ptr(), stream=stream)
            torch.cuda.synchronize()
            assert rts[i].last_kernel() == "trace_bin_kernel"
            return rts[i].last_store_policy()

        # one context, one buffer: after 8 renders nothing else is in the record
        said = [render(0) for _ in range(12)]
        assert said[8:] == ["default"] * 4, said
        assert np.array_equal(bufs[0].cpu().numpy(), want)
        # two buffers alternately: from the second pair on, both contexts
        pairs = [(render(0), render(1)) for _ in range(4)]
        assert pairs[1:] == [("large", "large")] * 3, pairs
        for b in bufs:
            assert np.array_equal(b.cpu().numpy(), want)
        # back to one buffer: the other ages out after 8 renders
        said = [render(0) for _ in range(10)]
        assert said[:7] == ["large"] * 7 and said[7:] == ["default"] * 3, said
        # the default threshold (512 MiB) is far away
        rts[0].store_policy("auto", 0)
        rts[1].store_policy("auto", 0)
        assert [render(0), render(1), render(0)] == ["default"] * 3
    finally:
        for r in rts:
            r.close()
        del keep
