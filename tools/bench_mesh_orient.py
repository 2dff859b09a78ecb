"""Time the mesh orientation path on the two meshes of tools/bench_mesh_topology.py -- the 512^3 mesh of
tools/bench_mesh.py's model and the mesh fused from tools/bench_tsdf.py's room -- with a seeded 30 % of their faces reversed.  Device
events, warm-up first, medians.  Timed: the kernels of nsa_mesh_orient (the union-find over the double cover) and of
nsa_mesh_orient_volume (the sort by label and the segmented reduction) without the wrappers' read-backs, ``orientation()`` and
``orient()`` end to end including the edge table.  Comparison points: nsa_mesh_face_components on the same edge table (half the nodes,
half the unions per joining edge, but it joins across every edge of count >= 2), and the host route on the same machine -- device ->
host copy of the faces, np.unique of the edge keys, a scipy.sparse.csgraph breadth-first two-colouring over the two-face edges.
Results go to profiles/mesh_orient_bench.json.
usage: python tools/bench_mesh_orient.py [reps=5] [resolution=512] [tsdf voxels=256] [tsdf frames=100]"""
import sys

import numpy as np
import torch

from benchlib import median, median_ms, mesh_positionals, model_mesh, time_host, tsdf_mesh, write_results
from nicer_slam_amd import mesh_topology as M
from nicer_slam_amd._native import lib, check


def parse_args(argv):
    return mesh_positionals(argv)


def host_route(f):
    """the flips of a breadth-first two-colouring the way a host program gets them: every component wound like the face its
    breadth-first tree starts from (scipy picks it; the device's rule is the smallest face).  Returns (flips, components)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import breadth_first_order, connected_components
    g = f.cpu().numpy().astype(np.int64)
    F = len(g)
    a = g.reshape(-1)
    b = g[:, [1, 2, 0]].reshape(-1)
    key = (np.minimum(a, b) << 32) | np.maximum(a, b)
    _, inv, count = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    first = (np.cumsum(count) - count)[count == 2]
    h0, h1 = order[first], order[first + 1]
    f0, f1 = h0 // 3, h1 // 3
    par = (a[h0] == a[h1]).astype(np.int8)                       # 1: the two half-edges run the same way
    n, comp = connected_components(sp.coo_matrix((np.ones(len(f0), np.int8), (f0, f1)), shape=(F, F)), directed=False)
    roots = np.unique(comp, return_index=True)[1]                 # the smallest face of every component
    # one breadth-first forest: a virtual node F joined to every root
    rows, cols = np.concatenate([f0, np.full(len(roots), F)]), np.concatenate([f1, roots])
    graph = sp.coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(F + 1, F + 1)).tocsr()
    _, pred = breadth_first_order(graph + graph.T, F, directed=False)
    # the parity of every tree edge, then the xor along the path to the root by pointer doubling
    ekey = np.minimum(f0, f1) * (F + 1) + np.maximum(f0, f1)
    o = np.argsort(ekey)
    ekey, epar = ekey[o], par[o]
    x, px = np.arange(F), pred[:F].astype(np.int64)
    q = np.minimum(x, px) * (F + 1) + np.maximum(x, px)
    idx = np.minimum(np.searchsorted(ekey, q), len(ekey) - 1) if len(ekey) else np.zeros(F, np.int64)
    acc = np.where(ekey[idx] == q, epar[idx], 0).astype(np.int8) if len(ekey) else np.zeros(F, np.int8)
    anc = np.where(px == F, x, px)
    while not (anc[anc] == anc).all():
        acc, anc = acc ^ acc[anc], anc[anc]
    return acc, n


def case(name, mesh, out, reps):
    timed = lambda fn: median_ms(fn, reps)
    gen = torch.Generator().manual_seed(7)
    f0 = mesh["faces"].contiguous()
    which = (torch.rand(f0.shape[0], generator=gen) < 0.3).to(f0.device)
    f = torch.where(which[:, None], f0[:, [0, 2, 1]], f0).contiguous()
    scrambled = dict(verts=mesh["verts"], faces=f)
    V, F = mesh["verts"].shape[0], f.shape[0]
    r = {"V": V, "F": F, "reversed": int(which.sum())}
    out_mesh, rep = M.orient(scrambled, return_report=True)
    r["report"] = {k: x for k, x in rep.items() if not torch.is_tensor(x)}
    # (a mesh whose faces look into the volume it encloses -- a room seen from inside -- comes back with every face reversed)
    r["restored"] = ("exactly" if torch.equal(out_mesh["faces"], f0) else
                     "every face reversed" if torch.equal(out_mesh["faces"], f0[:, [0, 2, 1]]) else "no")
    r["topology after"] = M.topology(out_mesh)
    dev = f.device
    stream = torch.cuda.current_stream().cuda_stream
    t, _ = M._edge_table(f, V, F, None)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device=dev)
    label, orientable, flip = i32(F), u8(F), u8(F)
    ws = torch.empty(lib.nsa_mesh_orient_workspace(F), dtype=torch.uint8, device=dev)
    tot = torch.empty(4, dtype=torch.int64, device=dev)
    r["orient kernels (cover union-find) ms"] = timed(lambda: check(lib.nsa_mesh_orient(
        f.data_ptr(), F, t["face_edges"].data_ptr(), t["edge_start"].data_ptr(), t["edge_halfedges"].data_ptr(),
        t["_totals"].data_ptr(), ws.data_ptr(), label.data_ptr(), orientable.data_ptr(), flip.data_ptr(), tot.data_ptr(), stream)))
    ws2 = torch.empty(lib.nsa_mesh_face_components_workspace(F), dtype=torch.uint8, device=dev)
    fl, tot2 = i32(F), torch.empty(2, dtype=torch.int64, device=dev)
    r["face components kernels ms"] = timed(lambda: check(lib.nsa_mesh_face_components(
        t["face_edges"].data_ptr(), t["edge_start"].data_ptr(), t["edge_halfedges"].data_ptr(), F, ws2.data_ptr(), fl.data_ptr(),
        tot2.data_ptr(), stream)))
    r["cover / face components"] = r["orient kernels (cover union-find) ms"] / r["face components kernels ms"]
    v = mesh["verts"].float().contiguous()
    origin = M._bbox_centre(v, f, label)
    S, P = torch.zeros(F, dtype=torch.float64, device=dev), torch.zeros(F, dtype=torch.float64, device=dev)
    n, flags, fo = i32(F), u8(F), u8(F)
    ws3 = torch.empty(lib.nsa_mesh_orient_volume_workspace(F), dtype=torch.uint8, device=dev)
    tot3 = torch.empty(5, dtype=torch.int64, device=dev)
    r["volume kernels (sort + segmented reduction) ms"] = timed(lambda: check(lib.nsa_mesh_orient_volume(
        v.data_ptr(), V, f.data_ptr(), F, t["face_edges"].data_ptr(), t["edge_start"].data_ptr(), label.data_ptr(),
        orientable.data_ptr(), flip.data_ptr(), origin.data_ptr(), ws3.data_ptr(), S.data_ptr(), P.data_ptr(), n.data_ptr(),
        flags.data_ptr(), fo.data_ptr(), tot3.data_ptr(), stream)))
    bits = max(1, int(F).bit_length())
    passes = (bits + 7) // 8
    # the unions touch the table once (12 B per edge for its two offsets and half-edges, 8 B of faces) and the labels once; the
    # sort moves (4 + 8 + 8) B per pass and face less one key write and one payload read; the reduction reads a face's three
    # vertices, three edge ids and their offsets
    r["orient MB moved at least"] = (3 * F // 2 * 20 + F * (8 + 12 + 6)) / 1e6
    r["volume MB moved at least"] = ((passes * 20 - 8) * F + F * (12 + 36 + 12 + 24 + 6 + 4)) / 1e6
    r["orientation() ms"] = timed(lambda: M.orientation(scrambled))
    r["orient(outward='volume') ms"] = timed(lambda: M.orient(scrambled))
    r["orient(outward=None) ms"] = timed(lambda: M.orient(scrambled, outward=None))
    r["edge_table() ms"] = timed(lambda: M.edge_table(f, V))
    try:
        r["host components"] = int(host_route(f)[1])
        r["host copy + np.unique + scipy breadth-first two-colouring ms"] = median(time_host(lambda: host_route(f), 3, warmup=False))
    except ImportError:
        r["host copy + np.unique + scipy breadth-first two-colouring ms"] = None
    out[name] = r


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    case(f"model mesh {a.resolution}^3", model_mesh(a.resolution), out, a.reps)
    case(f"tsdf room {a.voxels}^3, {a.frames} frames", tsdf_mesh(a.voxels, a.frames), out, a.reps)
    write_results(out, "mesh_orient_bench.json")


if __name__ == "__main__":
    main()
