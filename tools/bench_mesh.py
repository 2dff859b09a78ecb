"""Time mesh extraction for the test model of tests/test_inference_gpu.py::_model on [-1, 1]^3:
sdf_grid, marching cubes (count + emit), the vertex-colour pass, extract_mesh end to end, and the device->host copy of the
volume (the floor of any host marching-cubes route).  Device events, warm-up first, np.median of the reps (for an odd count, such
as the default, the middle sample); per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
usage: python tools/bench_mesh.py [resolution=512] [reps=5] [out.ply]"""
import json
import os
import sys

import torch

from benchlib import median_ms, model, positionals
from nicer_slam_amd import inference

BOUND = (-1.0, 1.0)
COPY_CEILING = 6.29e12          # bytes/s, measured device copy (MI355X_MICROARCH.md)


def parse_args(argv):
    return positionals(argv, resolution=(int, 512), reps=(int, 5), ply=(str, None))


@torch.no_grad()
def main(argv=None):
    from nicer_slam_amd._native import lib, check
    a = parse_args(sys.argv[1:] if argv is None else argv)
    RES, timed = a.resolution, lambda fn: median_ms(fn, a.reps)
    m = model()
    grid = lambda: inference.sdf_grid(m, RES, BOUND)
    t_grid, vol = timed(grid), grid()
    ax = torch.linspace(BOUND[0], BOUND[1], RES, dtype=torch.float64)
    step = float(ax[1] - ax[0])
    nx = ny = nz = RES
    ws = torch.empty(max(1, lib.nsa_marching_cubes_workspace(nx, ny, nz)), dtype=torch.uint8, device="cuda")
    totals = torch.empty(2, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def count():
        check(lib.nsa_marching_cubes_count(vol.data_ptr(), nx, ny, nz, 0.0, ws.data_ptr(), totals.data_ptr(), st))
    t_count = timed(count)
    cubes = lambda: inference.marching_cubes(vol, 0.0, (step,) * 3, (BOUND[0],) * 3)
    t_mc, mesh = timed(cubes), cubes()
    t_col = timed(lambda: inference.vertex_colours(m, mesh["verts"], mesh["normals"]))
    extract = lambda: inference.extract_mesh(m, RES, BOUND)
    t_all, full = timed(extract), extract()
    host = torch.empty(vol.shape, dtype=vol.dtype, pin_memory=True)
    t_d2h = timed(lambda: host.copy_(vol))
    nbytes = vol.numel() * 4
    res = dict(resolution=RES, V=int(full["verts"].shape[0]), F=int(full["faces"].shape[0]), sdf_grid_ms=round(t_grid, 3),
               count_ms=round(t_count, 3), marching_cubes_ms=round(t_mc, 3), colour_ms=round(t_col, 3),
               extract_mesh_ms=round(t_all, 3), volume_d2h_ms=round(t_d2h, 3),
               count_bytes_per_s=nbytes / (t_count * 1e-3), count_vs_copy_ceiling=nbytes / (t_count * 1e-3) / COPY_CEILING)
    print(json.dumps(res))
    if a.ply:
        inference.write_ply(a.ply, full)
        print(f"wrote {a.ply}: {os.path.getsize(a.ply)} bytes")


if __name__ == "__main__":
    main()
