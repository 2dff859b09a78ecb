"""The timing loops of tools/benchlib.py on the device: how often each calls its callee and in which order, what it returns,
and the fused-room fixture at its smallest useful size.  The callee adds 1 to 1024 floats: the loops are under test, not a kernel."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

# the smallest room tried that still gives a mesh: 8^3 voxels of 0.18 and the single view of ring(1) fuse to 4 vertices and 2 faces
# (16^3 and one view: 24 and 30; 32^3 and four views: 592 and 980)
TSDF_VOXELS, TSDF_FRAMES = 8, 1


class Counter:
    def __init__(self, log=None, tag=None):
        self.x = torch.zeros(1024, device="cuda")
        self.calls, self.log, self.tag = 0, log, tag

    def __call__(self):
        self.calls += 1
        if self.log is not None:
            self.log.append(self.tag)
        self.x.add_(1.0)
        return "a value the timers must not hand on"


def _samples_ok(ms, n):
    return isinstance(ms, list) and len(ms) == n and all(isinstance(t, float) and math.isfinite(t) and t > 0 for t in ms)


@pytest.mark.parametrize("reps,calls", [(1, 1), (5, 1), (3, 4)])
def test_event_timer(reps, calls):
    import benchlib as B
    fn = Counter()
    ms = B.time_events(fn, reps, calls) if calls > 1 else B.time_events(fn, reps)
    assert fn.calls == 1 + reps * calls and _samples_ok(ms, reps)
    assert float(fn.x[0]) == fn.calls                                         # every call reached the device
    fn = Counter()
    t = B.median_ms(fn, reps, calls)                                          # the same loop, then np.median
    assert fn.calls == 1 + reps * calls and isinstance(t, float) and math.isfinite(t) and t > 0


def test_event_window():
    import benchlib as B
    fn = Counter()
    t = B.event_window(fn, 3)
    assert fn.calls == 3 and isinstance(t, float) and t > 0


@pytest.mark.parametrize("warmup", [True, False])
def test_host_clock_timer(warmup):
    import benchlib as B
    fn = Counter()
    ms = B.time_host(fn, 4, warmup=warmup)
    assert fn.calls == 4 + int(warmup) and _samples_ok(ms, 4)
    fn = Counter()
    assert _samples_ok(B.time_host(fn, 2), 2) and fn.calls == 3               # the warm-up is the default


def test_pair_timer():
    import benchlib as B
    log = []
    a, b = Counter(log, "a"), Counter(log, "b")
    ms = B.time_pair(a, b, 3)
    assert log == ["a", "b"] * 4 and (a.calls, b.calls) == (4, 4)
    assert len(ms) == 2 and _samples_ok(ms[0], 3) and _samples_ok(ms[1], 3)


def test_tsdf_mesh_is_not_empty_and_repeats_bit_for_bit():
    import benchlib as B
    one, two = B.tsdf_mesh(TSDF_VOXELS, TSDF_FRAMES), B.tsdf_mesh(TSDF_VOXELS, TSDF_FRAMES)
    assert one["verts"].shape[0] > 0 and one["faces"].shape[0] > 0
    assert sorted(one) == sorted(two)
    for k in one:
        assert one[k].dtype == two[k].dtype and torch.equal(one[k], two[k]), k
