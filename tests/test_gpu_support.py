"""tests/gpu_support.py's `knobs`: the table names every diagnostics setter,
the scope resets every one of them however its block ends, and on the GPU a
scope that was left by an exception leaves the session's context rendering
what a fresh one renders."""
import numpy as np
import pytest

from gpu_support import DEFAULTS, H, KNOB_EXCLUSIONS, W, base_scene, knobs


def test_knob_table_is_complete(pkg):
    """A setter added to RayTracer must enter DEFAULTS (and so the reset) or
    KNOB_EXCLUSIONS, with its reason."""
    setters = {name[4:] for name in dir(pkg.RayTracer) if name.startswith("set_")}
    assert setters == set(DEFAULTS) | set(KNOB_EXCLUSIONS)
    assert not set(DEFAULTS) & set(KNOB_EXCLUSIONS)


class _Recorder:
    """Records every set_<name>(value) call, in order."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("set_"):
            raise AttributeError(name)
        return lambda value: self.calls.append((name[4:], value))

    def last(self):
        return dict(self.calls)  # (later calls of a name overwrite earlier ones)


def test_knobs_scope_on_a_recorder():
    stub = _Recorder()
    overlay = dict(DEFAULTS, trace_split=2, tile_variant=2)
    with pytest.raises(ValueError):
        with knobs(stub, trace_split=2, tile_variant=2):
            assert stub.last() == overlay
            raise ValueError("out of the block")
    assert stub.last() == DEFAULTS
    assert len(stub.calls) == 2 * len(DEFAULTS)  # every setter on entry, every one on exit
    stub = _Recorder()
    with pytest.raises(TypeError):
        knobs(stub, no_such_knob=1)
    assert stub.calls == []


@pytest.mark.gpu
def test_knobs_leave_the_defaults_behind(pkg, rt):
    scene = base_scene(pkg)
    with pkg.RayTracer(0) as fresh:
        want, _ = fresh.render(scene, W, H)
        want_kernel = fresh.last_kernel()
    with pytest.raises(ValueError):
        with knobs(rt, small_path=False, trace_bin=2, trace_split=1, tile_variant=2):
            rt.render(scene, W, H)
            assert rt.last_kernel() == "trace3_kernel"
            raise ValueError("out of the block")
    got, _ = rt.render(scene, W, H)
    assert rt.last_kernel() == want_kernel
    assert np.array_equal(got, want)
