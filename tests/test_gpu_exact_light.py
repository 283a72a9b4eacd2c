"""The kernels of the light pass against exact light and colour
(tests/exact_light.py), directly.

Not a second device-equals-host suite: what each kernel wrote is judged by
`exact_light` itself, with the cases, counts, caps and judges of
tests/test_exact_light.py, so a defect that header, host function and
restatement share still shows.  The hit frames come from the device
(`cast_camera_device` through each case's camera) and are judged first; the
bounce frames that give each level's `t` come from `bounce_hits_device`.
Device memory is torch tensors; every output sits between guard words, the
scene's arrays and the reflectivity array between padding, and guards, padding,
the hit frame, the reflectivities and the cube records must come back unchanged.

1073 pixels are 17 waves with a partial last one, and every frame mixes cube,
sphere and miss lanes in a wave: where the wave-uniform vertex path and the LDS
blend stack could differ from the host.

The file launches kernels of code objects that rt_init does not preload, as
tests/test_gpu_camera_light.py does.
"""
import numpy as np
import pytest

import light_device as ld
import test_exact_light as tl
import test_gpu_rays as tg
from test_gpu_camera_light import RECORD_WORDS

gpu = pytest.mark.gpu
FW, FH, N = tl.FW, tl.FH, tl.N
ROWS = (0, FH)
PASSES = {("light", False): "light", ("light", True): "shadow", ("reflected", False): "reflect",
          ("reflected", True): "shadow_reflect"}


class Device:
    """test_exact_light.Host's calls through the kernels."""

    def __init__(self, pkg, rt, torch):
        self.pkg, self.rt, self.torch = pkg, rt, torch

    def cast(self, c):
        torch = self.torch
        ds, keep = ld.padded_device_scene(torch, c.scene)
        buf, ptr = tg.guarded_words(torch, 2 * N)
        torch.cuda.synchronize()
        self.rt.cast_camera_device(c.cam, ds, FW, ROWS, ptr)
        hits = tg.body_words(torch, buf).view(self.pkg.HIT_DTYPE).reshape(FH, FW).copy()
        ld.check_scene_padding(torch, c.scene, keep)
        del keep
        return hits

    def bounce(self, c, hits, j):
        torch = self.torch
        ds, keep = ld.padded_device_scene(torch, c.scene)
        hd = ld.upload_hits(torch, hits)
        buf = ld.run_device("mirror", self.pkg, self.rt, torch, ds, hd, FW, ROWS, "bounce", d=c.d,
                            depth=j)
        got = ld.unguard(torch, self.pkg, buf, FW, ROWS, "bounce")
        assert np.array_equal(hd.cpu().numpy().view(np.uint32), ld.words(hits)), "hit frame"
        ld.check_scene_padding(torch, c.scene, keep)
        del keep
        return got

    def lit(self, c, hits, call, fmt, refl=None, depth=0, shadows=False):
        pkg, rt, torch = self.pkg, self.rt, self.torch
        ds, keep = ld.padded_device_scene(torch, c.scene)
        hd = ld.upload_hits(torch, hits)
        records = slots = None
        if call in PASSES:
            extra = dict(refl=float(refl)) if call == "reflected" else {}
            buf = ld.run_device(PASSES[call, shadows], pkg, rt, torch, ds, hd, FW, ROWS, fmt, d=c.d,
                                **extra)
            got = ld.unguard(torch, pkg, buf, FW, ROWS, fmt)
        else:
            slots = np.asarray(refl, np.float32)
            refl_ptr, keep_refl = ld.padded_array(torch, slots)
            accel_ptr = 0
            if call.endswith("_accel"):
                records, accel_ptr = tg.guarded_words(torch, RECORD_WORDS * c.scene.num_cubes)
                torch.cuda.synchronize()
                rt.build_accel_device(ds, accel_ptr)
                built = tg.body_words(torch, records).copy()
            if call == "mirrored":
                buf = ld.run_device("mirror", pkg, rt, torch, ds, hd, FW, ROWS, fmt, d=c.d,
                                    refl=refl_ptr, depth=depth, shadows=shadows)
                got = ld.unguard(torch, pkg, buf, FW, ROWS, fmt)
            else:
                buf, ptr = tg.guarded_words(torch, N * ld.KINDS[fmt][0])
                torch.cuda.synchronize()
                if call == "mirrored_accel":
                    rt.light_hits_mirrored_accel_device(hd.data_ptr(), ds, accel_ptr, FW, ROWS, ptr,
                                                        refl_ptr, depth, ray_dir=c.d, fmt=fmt,
                                                        shadows=shadows)
                else:  # "camera", "camera_accel": no hit frame is read
                    rt.light_camera_device(c.cam, ds, accel_ptr, FW, ROWS, refl_ptr, depth, ptr,
                                           fmt=fmt, shadows=shadows)
                got = tg.body_words(torch, buf)
                got = got.view(np.int32).reshape(FH, FW, 4) if fmt == "i32x4" else got
            ld.check_padding(torch, slots, keep_refl, "reflectivity")
            if records is not None:
                assert np.array_equal(tg.body_words(torch, records), built), "cube records"
        assert np.array_equal(hd.cpu().numpy().view(np.uint32), ld.words(hits)), "hit frame"
        ld.check_scene_padding(torch, c.scene, keep)
        del keep
        return got.reshape(N, 4) if fmt == "i32x4" else got.reshape(N)


@pytest.fixture
def device(pkg, rt):
    return Device(pkg, rt, pytest.importorskip("torch"))


@gpu
@pytest.mark.parametrize("name", ["shadow", "slanted"])
def test_lit_and_shadowed_frames_device(pkg, device, name):
    tl.case_lit(pkg, device, name)


@gpu
@pytest.mark.parametrize("r", [0.25, 0.75])
def test_one_bounce_device(pkg, device, r):
    tl.case_bounce(pkg, device, r)


@gpu
@pytest.mark.parametrize("depth, shadows", [(2, False), (2, True), (3, False), (3, True)])
def test_chains_on_flat_mirrors_device(pkg, device, depth, shadows):
    tl.case_corridor(pkg, device, depth, shadows)


@gpu
def test_camera_views_device(pkg, device):
    tl.case_camera(pkg, device)
