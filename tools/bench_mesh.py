"""Time mesh extraction for the test model of tests/test_inference_gpu.py::_model on [-1, 1]^3:
sdf_grid, marching cubes (count + emit), the vertex-colour pass, extract_mesh end to end, and the device->host copy of the
volume (the floor of any host marching-cubes route).  Device events, warm-up first; per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.
usage: python tools/bench_mesh.py [resolution=512] [reps=5] [out.ply]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from nicer_slam_amd import inference
from nicer_slam_amd.utils.conf import replica_model_conf
from nicer_slam_amd.model.network import SLAMNetwork

RES = int(sys.argv[1]) if len(sys.argv) > 1 else 512
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
PLY = sys.argv[3] if len(sys.argv) > 3 else None
BOUND = (-1.0, 1.0)
COPY_CEILING = 6.29e12          # bytes/s, measured device copy (MI355X_MICROARCH.md)


def model():
    torch.manual_seed(4)
    m = SLAMNetwork(replica_model_conf(use_warp_loss=False)).cuda()
    with torch.no_grad():
        for enc in (m.implicit_network.coarse.encoding, m.implicit_network.fine.encoding, m.rendering_network.encoding):
            enc.embeddings.uniform_(-0.05, 0.05)
    return m.eval()


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    ms.sort()
    return ms[len(ms) // 2], out


@torch.no_grad()
def main():
    from nicer_slam_amd._native import lib, check
    m = model()
    t_grid, vol = timed(lambda: inference.sdf_grid(m, RES, BOUND))
    ax = torch.linspace(BOUND[0], BOUND[1], RES, dtype=torch.float64)
    step = float(ax[1] - ax[0])
    nx = ny = nz = RES
    ws = torch.empty(max(1, lib.nsa_marching_cubes_workspace(nx, ny, nz)), dtype=torch.uint8, device="cuda")
    totals = torch.empty(2, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def count():
        check(lib.nsa_marching_cubes_count(vol.data_ptr(), nx, ny, nz, 0.0, ws.data_ptr(), totals.data_ptr(), st))
    t_count, _ = timed(count)
    t_mc, mesh = timed(lambda: inference.marching_cubes(vol, 0.0, (step,) * 3, (BOUND[0],) * 3))
    t_col, _ = timed(lambda: inference.vertex_colours(m, mesh["verts"], mesh["normals"]))
    t_all, full = timed(lambda: inference.extract_mesh(m, RES, BOUND))
    host = torch.empty(vol.shape, dtype=vol.dtype, pin_memory=True)
    t_d2h, _ = timed(lambda: host.copy_(vol))
    nbytes = vol.numel() * 4
    res = dict(resolution=RES, V=int(full["verts"].shape[0]), F=int(full["faces"].shape[0]), sdf_grid_ms=round(t_grid, 3),
               count_ms=round(t_count, 3), marching_cubes_ms=round(t_mc, 3), colour_ms=round(t_col, 3),
               extract_mesh_ms=round(t_all, 3), volume_d2h_ms=round(t_d2h, 3),
               count_bytes_per_s=nbytes / (t_count * 1e-3), count_vs_copy_ceiling=nbytes / (t_count * 1e-3) / COPY_CEILING)
    print(json.dumps(res))
    if PLY:
        inference.write_ply(PLY, full)
        print(f"wrote {PLY}: {os.path.getsize(PLY)} bytes")


if __name__ == "__main__":
    main()
