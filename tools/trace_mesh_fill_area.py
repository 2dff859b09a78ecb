"""What a kernel trace says about the minimum-area patches: which bound holds the TSDF room (two loops of 684 edges under
method="auto") and the model mesh without every 97th face (thousands of small loops under method="min_area").
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/trace_mesh_fill_area.py
runs each fill three times after a warm-up, on the meshes of tools/bench_mesh_fill.py at their default sizes; then
    python tools/trace_mesh_fill_area.py --summarise DIR
reads the trace and prints, for the last call of each mesh, the launch count, the kernel time beside the span from the first kernel's
start to the last one's end, and the share of the diagonal launches, as one JSON object.  A call is told from the next by its one
k_fa_plan launch; the first half of the calls are the room's, the second half the masked mesh's."""
import csv
import glob
import json
import os
import sys
from types import SimpleNamespace


def summarise(folder):
    files = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {folder}")
    rows = []
    for path in files:
        with open(path) as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows.sort()
    plans = [i for i, r in enumerate(rows) if "k_fa_plan" in r[2]]
    ends = [i for i, r in enumerate(rows) if "k_fa_finish" in r[2] or "k_fa_emit" in r[2]]
    calls = []
    for n, p in enumerate(plans):                                 # a call: from after the previous call's last area kernel to its own
        prev = max([e for e in ends if e < p], default=-1)
        last = max([e for e in ends if e > p and (n + 1 == len(plans) or e < plans[n + 1])], default=p)
        ks = rows[prev + 1:last + 1]
        # (the kernels of the previous call's tail -- concatenations, the topology of the result -- come first: cut at the edge table)
        first = next((i for i, k in enumerate(ks) if "k_edge" in k[2] or "k_te_" in k[2] or "mesh_edges" in k[2]), 0)
        ks = ks[first:]
        area = [k for k in ks if "fill_area" in k[2]]
        diag = [k for k in area if "k_fa_diag" in k[2]]
        wave = [k for k in diag if "k_fa_diag_wave" in k[2]]
        dur = lambda xs: sum(e - s for s, e, _ in xs) / 1e3
        calls.append({"launches": len(ks), "kernel us": dur(ks), "span us": (ks[-1][1] - ks[0][0]) / 1e3,
                      "area launches": len(area), "area kernel us": dur(area), "area span us": (area[-1][1] - area[0][0]) / 1e3,
                      "diagonal launches": len(diag), "diagonal kernel us": dur(diag), "one-wave diagonal launches": len(wave),
                      "one-wave diagonal kernel us": dur(wave), "emit us": dur([k for k in area if "k_fa_emit" in k[2]]),
                      "longest diagonal launch us": max([(e - s) / 1e3 for s, e, _ in diag], default=0.0)})
    half = len(calls) // 2
    out = {"calls in the trace": len(calls), "room, last call": calls[half - 1] if half else None,
           "masked mesh, last call": calls[-1] if calls else None}
    print(json.dumps(out, indent=1))
    return out


def parse_args(argv):
    """--summarise DIR, or the positionals of tools/bench_mesh_fill.py: [reps (unused)] [resolution=512] [tsdf voxels=256] [tsdf frames=100]"""
    if len(argv) > 1 and argv[0] == "--summarise":
        return SimpleNamespace(summarise=argv[1])
    from benchlib import mesh_positionals
    a = mesh_positionals(argv)
    a.summarise = None
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    if a.summarise:
        return summarise(a.summarise)
    import torch
    from benchlib import model_mesh, tsdf_mesh
    from nicer_slam_amd import mesh_fill as M
    room = tsdf_mesh(a.voxels, a.frames)
    full = model_mesh(a.resolution)
    keep = torch.arange(full["faces"].shape[0], device=full["faces"].device) % 97 != 96
    masked = {"verts": full["verts"], "faces": full["faces"][keep]}
    for mesh, method in ((room, "auto"), (masked, "min_area")):
        mesh = {"verts": mesh["verts"].float().contiguous(), "faces": mesh["faces"].to(torch.int32).contiguous()}
        for _ in range(4):                                        # a warm-up and three calls
            _, rep = M.fill_holes(mesh, method=method, return_report=True)
            torch.cuda.synchronize()
        print(method, rep["totals"], rep["area_totals"], flush=True)


if __name__ == "__main__":
    main()
