"""What the tools/bench_*.py programs share: the timing loops, the fixtures that more than one of them measures, the
"positional with a default" command line, and the results epilogue.  Plain functions of their parameters: nothing here reads the
command line, and no tool imports another tool -- what two tools need lives here."""
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the package, and the tests' numpy statements that serve as host baselines.  Every tool now searches ROOT, tests/, tools/ in that
# order (the tools wrote tests/, tools/, ROOT, and only some added tests/); no module name exists in two of the three.
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

ROOM_HALF = (0.62, 0.5, 0.56)          # the half extents of tools/synthetic_sequence.render_analytic_room's room


# ---- timing: every loop returns its samples; the statistic is the caller's next step

def event_window(fn, calls=1):
    """ms per call of one window: ``calls`` back-to-back calls between two device events, then a synchronise (the only place the
    tools make events; a tool that must restore state between windows calls this itself)"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def time_events(fn, reps, calls=1):
    """ms per call of ``reps`` windows of ``calls`` back-to-back calls between two device events, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    return [event_window(fn, calls) for _ in range(reps)]


def time_host(fn, reps, warmup=True):
    """ms by the host clock of ``reps`` calls, each between two device synchronises, after one warm-up call unless told otherwise"""
    if warmup:
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms


def time_pair(a, b, reps):
    """(ms of a, ms of b) by device events over ``reps`` rounds of a, b, after one warm-up of each"""
    a()
    b()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(reps):
        ms[0].append(event_window(a))
        ms[1].append(event_window(b))
    return ms


def median(ms):
    return float(np.median(ms))


def median_min_max(ms):
    return median(ms), float(np.min(ms)), float(np.max(ms))


def median_ms(fn, reps, calls=1):
    """the composition most rows are: median(time_events(fn, reps, calls))"""
    return median(time_events(fn, reps, calls))


# ---- fixtures that more than one tool measures; seeded, functions of their arguments alone

def model():
    """the test network of tests/test_inference_gpu.py::_model"""
    from nicer_slam_amd.model.network import SLAMNetwork
    from nicer_slam_amd.utils.conf import replica_model_conf
    torch.manual_seed(4)
    m = SLAMNetwork(replica_model_conf(use_warp_loss=False)).cuda()
    with torch.no_grad():
        for enc in (m.implicit_network.coarse.encoding, m.implicit_network.fine.encoding, m.rendering_network.encoding):
            enc.embeddings.uniform_(-0.05, 0.05)
    return m.eval()


def model_mesh(res):
    """the surface of model() on [-1, 1]^3 at res^3 samples, without colours"""
    from nicer_slam_amd import inference
    return inference.extract_mesh(model(), res, (-1.0, 1.0), color=False)


def ring(n):
    """n camera-to-world matrices on a ring inside the room, looking outwards, pitched up and down"""
    out = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        a = 2 * np.pi * k / n
        el = 0.6 * np.sin(7.0 * a)
        fwd = np.array([np.cos(a) * np.cos(el), np.sin(el), np.sin(a) * np.cos(el)])
        right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
        right /= np.linalg.norm(right)
        out[k, :3, 0], out[k, :3, 1], out[k, :3, 2] = right, np.cross(fwd, right), fwd
        out[k, :3, 3] = [0.22 * np.cos(a), 0.05 * np.sin(3 * a), 0.22 * np.sin(a)]
    return out.astype(np.float32)


def tsdf_mesh(voxels, frames):
    """the mesh of ``frames`` 480 x 640 views from ring() of the analytic room, fused into voxels^3 cells with colour"""
    import synthetic_sequence as ss
    from nicer_slam_amd.tsdf import TSDFVolume
    H, W, vl = 480, 640, 1.44 / voxels
    poses = ring(frames)
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = 400.0
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    vol = TSDFVolume((-0.72,) * 3, (0.72,) * 3, vl, 4 * vl)
    for lo in range(0, frames, 50):
        c, d, _ = ss.render_analytic_room(torch.from_numpy(poses[lo:lo + 50]), K, H, W, "cuda", ROOM_HALF)
        vol.integrate(d.reshape(-1, H, W), c, poses[lo:lo + 50], K, batch=32)
    return vol.extract_mesh()


def mc_sphere(res, r=0.5, bound=1.0):
    """marching cubes of a sphere of radius r sampled at res^3 points of [-bound, bound]^3"""
    from nicer_slam_amd import inference
    ax = torch.linspace(-bound, bound, res, dtype=torch.float64)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sqrt(X ** 2 + Y ** 2 + Z ** 2) - r).float().cuda()
    step = float(ax[1] - ax[0])
    return inference.marching_cubes(vol, 0.0, (step,) * 3, (-bound,) * 3)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """the camera-to-world matrix at eye whose z axis points at target"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


# ---- command lines and results

def positionals(argv, **spec):
    """argv's leading positionals by name: spec[name] = (convert, default) in their order on the command line.  A missing one takes
    its default; what follows the last named one is ignored, as it always was."""
    return SimpleNamespace(**{name: convert(argv[i]) if i < len(argv) else default
                              for i, (name, (convert, default)) in enumerate(spec.items())})


def mesh_positionals(argv, reps=5, resolution=512, **more):
    """[reps] [resolution] [tsdf voxels=256] [tsdf frames=100] and what a tool adds behind them.  ``reps`` and ``resolution`` are
    the plain int defaults of the two leading positions (both are always int); every further positional in ``more`` is a
    name=(convert, default) pair exactly as positionals() takes it, e.g. mesh_positionals(argv, lattice=(int, 3000))."""
    return positionals(argv, reps=(int, reps), resolution=(int, resolution), voxels=(int, 256), frames=(int, 100), **more)


def write_results(res, name=None, path=None, echo=True):
    """res as json.dumps(indent=1): printed unless echo is False, and written with a trailing newline to ``path``, or to
    profiles/<name> when only a name is given (the directory is made); with neither it is only printed.  Returns the path."""
    text = json.dumps(res, indent=1)
    if echo:
        print(text)
    if path is None and name is not None:
        path = os.path.join(ROOT, "profiles", name)
    if path is not None:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(text + "\n")
    return path
