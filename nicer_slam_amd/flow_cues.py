"""Optical-flow ground truth from depth and poses, on the device (include/nicer_slam_amd.h Section 13).

The mapping objective's flow term compares the renderer's re-projection flow with ``ground_truth["flow"]`` under
``ground_truth["flow_mask"]`` along ``ground_truth["edges"]``.  The reference makes those offline with GMFlow and a forward-backward
consistency check (preprocess/extract_flows.py) and reads them from a ``*_pair`` directory (code/training/volsdf_train.py:312-361).
With depth frames and poses the flow is geometry: ``induced_flow`` projects every pixel of one frame into another,
``consistency`` applies the reference's occlusion rule, ``FlowStore`` keeps the result on the device and ``FlowStore.select`` is the
per-iteration gather.  Files are the reference's, both ways: a directory written here is read by its trainer, one written by
GMFlow is read here.

    python -m nicer_slam_amd.flow_cues --depth DEPTH_DIR --poses P --intrinsics FX FY CX CY --out SEQ_pair [--interval 10 --rad 2]
"""
import argparse
import lzma
import os

import numpy as np
import torch

from ._native import check, lib
from .mesh_args import ptr, stream
from .tsdf import _as_numpy, _intrinsics4

DEFAULT_NEAR = 1e-3
DEFAULT_ALPHA, DEFAULT_BETA = 0.01, 0.5              # GMFlow's forward_backward_consistency_check


def _on_device(name, *tensors):
    """The kernels read device memory: a host tensor is refused here, before anything is launched."""
    for t in tensors:
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError(f"{name}: device (CUDA) tensors; move host data over with .cuda() first")


def _index_list(x, name):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name}: integer indices")
    return a.astype(np.int64).reshape(-1)


def relative_poses(c2w, src, dst):
    """float64 [E, 3, 4] rows [R_e | t_e] of inv(c2w[dst[e]]) @ c2w[src[e]], composed on the host."""
    P = _as_numpy(c2w, np.float64)
    if P.ndim != 3 or P.shape[1:] != (4, 4):
        raise ValueError("c2w: [n, 4, 4] camera-to-world matrices")
    if not np.isfinite(P).all():
        raise ValueError("c2w: a pose is not finite")
    inv = np.linalg.inv(P)
    return np.ascontiguousarray((inv[dst] @ P[src])[:, :3, :])


# --------------------------------------------------------------------------------------------------------------------- the kernels
@torch.no_grad()
def induced_flow(depth, c2w, intrinsics, src, dst, near=DEFAULT_NEAR, device="cuda"):
    """Flow that depth and poses induce from frame src[e] to frame dst[e]: depth [n, H, W] z-depth (0, negative, NaN, inf = no
    measurement), c2w [n, 4, 4], intrinsics as ``tsdf.TSDFVolume.integrate`` takes them, src / dst [E] frame indices.
    -> (flow [E, H, W, 2] fp32, valid [E, H, W] uint8) on the device.  A pixel is valid when its depth is finite and positive and the
    point lies more than ``near`` in front of the target camera; an invalid pixel has flow (0, 0).  Landing outside the target image
    does not make a pixel invalid."""
    depth = torch.as_tensor(depth)
    if depth.dim() != 3:
        raise ValueError("depth: [n, H, W]")
    n, H, W = depth.shape
    if n == 0 or H == 0 or W == 0 or H * W >= 2 ** 31:
        raise ValueError(f"depth: {n} frames of {H} x {W}")
    src, dst = _index_list(src, "src"), _index_list(dst, "dst")
    if src.shape != dst.shape:
        raise ValueError(f"src and dst: {src.size} and {dst.size} edges")
    if src.size and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= n):
        raise ValueError(f"src / dst: a frame index outside [0, {n})")
    if not (0 <= near < float("inf")):
        raise ValueError("near: finite and >= 0")
    K = _intrinsics4(intrinsics, n)
    P = _as_numpy(c2w, np.float64)
    if P.ndim != 3 or P.shape != (n, 4, 4):
        raise ValueError(f"c2w: [{n}, 4, 4] camera-to-world matrices")
    rel = relative_poses(P, src, dst)
    dev = depth.device if depth.is_cuda else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"induced_flow: device {dev} is not a GPU")
    E = src.size
    flow = torch.empty(E, H, W, 2, dtype=torch.float32, device=dev)
    valid = torch.empty(E, H, W, dtype=torch.uint8, device=dev)
    if E == 0:
        return flow, valid
    d = depth.to(dev, torch.float32).contiguous()
    K_d = torch.from_numpy(np.ascontiguousarray(K)).to(dev)
    rel_d = torch.from_numpy(rel).to(dev)
    src_d = torch.from_numpy(src.astype(np.int32)).to(dev)
    dst_d = torch.from_numpy(dst.astype(np.int32)).to(dev)
    check(lib.nsa_flowcue_induced(d.data_ptr(), n, H, W, K_d.data_ptr(), int(K.shape[0] > 1), rel_d.data_ptr(), src_d.data_ptr(),
                                  dst_d.data_ptr(), E, float(near), flow.data_ptr(), valid.data_ptr(), stream(dev)))
    return flow, valid


@torch.no_grad()
def consistency(fwd, bwd, fwd_valid=None, bwd_valid=None, alpha=DEFAULT_ALPHA, beta=DEFAULT_BETA):
    """The forward-backward consistency rule of extract_flows.py (Section 13): fwd, bwd [P, H, W, 2] (or [H, W, 2]) device flows of
    frame a -> b and b -> a -> (fwd_occ, bwd_occ) [P, H, W] uint8, 1 = occluded.  With validity maps ([P, H, W], both or neither) a
    pixel is also occluded when it or its landing point has no valid flow; without them the result is the reference's rule on any
    flow, GMFlow's included (``torch.from_numpy(read_pair(...)[0]).cuda()``).  Every tensor must be on the device; H, W >= 2."""
    if not isinstance(fwd, torch.Tensor) or not isinstance(bwd, torch.Tensor):
        raise ValueError("fwd and bwd: torch tensors")
    if fwd.dim() == 3:
        fwd, bwd = fwd[None], bwd[None]
        fwd_valid = None if fwd_valid is None else fwd_valid[None]
        bwd_valid = None if bwd_valid is None else bwd_valid[None]
    if fwd.dim() != 4 or fwd.shape[-1] != 2 or bwd.shape != fwd.shape:
        raise ValueError("fwd and bwd: [P, H, W, 2], the same shape")
    if (fwd_valid is None) != (bwd_valid is None):
        raise ValueError("fwd_valid and bwd_valid: both or neither")
    P, H, W, _ = fwd.shape
    if fwd_valid is not None and (tuple(fwd_valid.shape) != (P, H, W) or tuple(bwd_valid.shape) != (P, H, W)):
        raise ValueError(f"validity maps: [{P}, {H}, {W}]")
    if H < 2 or W < 2:
        raise ValueError("consistency: images of at least 2 x 2 pixels")
    _on_device("consistency", fwd, bwd, fwd_valid, bwd_valid)
    dev = fwd.device
    f, b = fwd.to(torch.float32).contiguous(), bwd.to(dev, torch.float32).contiguous()
    fv = None if fwd_valid is None else fwd_valid.to(dev).ne(0).to(torch.uint8).contiguous()
    bv = None if bwd_valid is None else bwd_valid.to(dev).ne(0).to(torch.uint8).contiguous()
    fo = torch.empty(P, H, W, dtype=torch.uint8, device=dev)
    bo = torch.empty(P, H, W, dtype=torch.uint8, device=dev)
    check(lib.nsa_flowcue_consistency(ptr(f), ptr(b), ptr(fv), ptr(bv), P, H, W, float(alpha), float(beta), ptr(fo), ptr(bo),
                                      stream(dev)))
    return fo, bo


# ------------------------------------------------------------------------------------------------------- the reference's pair lists
def pair_list(n_images, interval=10, rad=2):
    """The directed frame pairs extract_flows.py:49-55 computes flow for, in its order: every ``interval``-th frame against the
    rad + 1 such frames before it, both directions."""
    es = []
    for i in range(0, (n_images - 1) // interval + 1):
        for j in range(max(i - rad - 1, 0), i):
            es.append((i * interval, j * interval))
            es.append((j * interval, i * interval))
    return es


def build_graph(keyframe_list, placeholder=0, thresh=30, device="cuda"):
    """volsdf_train.py:312-324: the edges between keyframes whose frame numbers are multiples of 10 and at most ``thresh`` apart.
    -> (idii + placeholder, idjj + placeholder, ii, jj): positions in the keyframe list and frame numbers, int64 on ``device``."""
    ides, es = [], []
    for idx, x in enumerate(keyframe_list):
        for idy, y in enumerate(keyframe_list):
            if x % 10 == 0 and y % 10 == 0 and 0 < abs(x - y) <= thresh:
                ides.append((idx, idy))
                es.append((int(x), int(y)))
    ides = torch.as_tensor(ides, dtype=torch.int64, device=device).reshape(-1, 2)
    es = torch.as_tensor(es, dtype=torch.int64, device=device).reshape(-1, 2)
    return ides[:, 0] + placeholder, ides[:, 1] + placeholder, es[:, 0], es[:, 1]


@torch.no_grad()
def pair_cues(depth, c2w, intrinsics, pairs, near=DEFAULT_NEAR, alpha=DEFAULT_ALPHA, beta=DEFAULT_BETA, device="cuda"):
    """Flow and occlusion for a list of directed pairs (i, j) of frame indices into ``depth``: -> (flow [E, H, W, 2] fp32,
    occ [E, H, W] uint8, 1 = occluded) in the order of ``pairs``.  Every unordered pair is computed once -- its two flows in one
    launch for all pairs, its two occlusion maps in another -- whichever of its directions the list holds, and however often."""
    pairs = [(int(i), int(j)) for i, j in pairs]
    if any(i == j for i, j in pairs):
        raise ValueError("pair_cues: a pair of a frame with itself")
    depth = torch.as_tensor(depth)
    if depth.dim() != 3:
        raise ValueError("depth: [n, H, W]")
    _, H, W = depth.shape
    if H < 2 or W < 2:
        raise ValueError("pair_cues: images of at least 2 x 2 pixels")
    slot = {}
    for i, j in pairs:
        slot.setdefault((min(i, j), max(i, j)), len(slot))
    lo = [k[0] for k in slot]
    hi = [k[1] for k in slot]
    U = len(slot)
    flow, valid = induced_flow(depth, c2w, intrinsics, lo + hi, hi + lo, near, device)      # [0, U): lo -> hi, [U, 2U): hi -> lo
    occ = torch.empty_like(valid)
    if U:
        check(lib.nsa_flowcue_consistency(flow[:U].data_ptr(), flow[U:].data_ptr(), valid[:U].data_ptr(), valid[U:].data_ptr(), U, H, W,
                                          float(alpha), float(beta), occ[:U].data_ptr(), occ[U:].data_ptr(), stream(flow.device)))
    order = [slot[(min(i, j), max(i, j))] + (0 if i < j else U) for i, j in pairs]
    if order == list(range(len(order))) and len(order) == 2 * U:
        return flow, occ
    order = torch.as_tensor(order, dtype=torch.int64, device=flow.device)
    return flow.index_select(0, order), occ.index_select(0, order)


# ----------------------------------------------------------------------------------------------------------------------- the files
def _stem(flow_dir, i, j):
    return os.path.join(flow_dir, f"{int(i):04d}_{int(j):04d}")


def write_pair(flow_dir, i, j, flow, flow_bwd, occ, occ_bwd, compress=True):
    """The four files of extract_flows.py for the pair (i, j): {i:04d}_{j:04d}_flow.npy and _flow_bwd.npy ([H, W, 2] fp32, np.save
    through lzma; ``compress=False`` writes plain .npy, which every reader here and the reference's trainer also take) and _occ.png,
    _occ_bwd.png (single-channel uint8, 255 = occluded)."""
    from PIL import Image
    os.makedirs(flow_dir, exist_ok=True)
    stem = _stem(flow_dir, i, j)
    for tag, f in (("_flow.npy", flow), ("_flow_bwd.npy", flow_bwd)):
        a = _as_numpy(f, np.float32)
        if a.ndim != 3 or a.shape[-1] != 2:
            raise ValueError("write_pair: a flow is [H, W, 2]")
        with (lzma.open(stem + tag, "wb") if compress else open(stem + tag, "wb")) as fh:
            np.save(fh, a)
    for tag, o in (("_occ.png", occ), ("_occ_bwd.png", occ_bwd)):
        a = _as_numpy(o, np.uint8)
        if a.ndim != 2:
            raise ValueError("write_pair: an occlusion map is [H, W]")
        Image.fromarray(np.where(a != 0, np.uint8(255), np.uint8(0))).save(stem + tag)


def _read_flow(path):
    try:
        with lzma.open(path, "rb") as fh:
            return np.load(fh).astype(np.float32)
    except lzma.LZMAError:
        return np.load(path).astype(np.float32)


def _read_occ(path):
    from PIL import Image
    a = np.array(Image.open(path))
    if a.ndim == 3:
        a = a[:, :, 0]                                   # (the trainer reads channel 0 of cv2's three equal channels)
    return (a != 0).astype(np.uint8)


def read_pair(flow_dir, i, j):
    """-> (flow, flow_bwd [H, W, 2] fp32, occ, occ_bwd [H, W] uint8 with 1 = occluded) of the pair (i, j), from lzma-compressed or
    plain .npy as volsdf_train.py:332-341 reads them; a pixel is usable where the trainer's test ``png[:, :, 0] == 0`` holds."""
    stem = _stem(flow_dir, i, j)
    return (_read_flow(stem + "_flow.npy"), _read_flow(stem + "_flow_bwd.npy"), _read_occ(stem + "_occ.png"),
            _read_occ(stem + "_occ_bwd.png"))


# ------------------------------------------------------------------------------------------------------------------- resident store
class FlowStore:
    """The flows [E, H * W, 2] fp32 and usable masks [E, H * W] bool (occlusion == 0) of an edge set, resident on the device:
    the reference's ``get_edges_flow`` tensors, and ``select`` its ``select_flow_uv``."""

    def __init__(self, flows, masks, H, W):
        E = flows.shape[0]
        if tuple(flows.shape) != (E, H * W, 2) or tuple(masks.shape) != (E, H * W):
            raise ValueError(f"FlowStore: flows [E, {H * W}, 2] and masks [E, {H * W}]")
        _on_device("FlowStore", flows)
        self.flows = flows.to(torch.float32).contiguous()
        self.masks = masks.to(self.flows.device, torch.bool).contiguous()
        self.H, self.W = int(H), int(W)

    @classmethod
    def from_dir(cls, flow_dir, edges, device="cuda"):
        """Read {ii:04d}_{jj:04d}_flow.npy and _occ.png of every edge (edges = build_graph's four tensors, or (ii, jj))."""
        ii, jj = _index_list(edges[-2], "ii"), _index_list(edges[-1], "jj")
        flows, masks = [], []
        for i, j in zip(ii, jj):
            stem = _stem(flow_dir, i, j)
            flows.append(_read_flow(stem + "_flow.npy"))
            masks.append(_read_occ(stem + "_occ.png") == 0)
        if not flows:
            raise ValueError("FlowStore.from_dir: no edges")
        H, W = flows[0].shape[:2]
        f = torch.from_numpy(np.stack(flows)).to(device).reshape(len(flows), H * W, 2)
        m = torch.from_numpy(np.stack(masks)).to(device).reshape(len(flows), H * W)
        return cls(f, m, H, W)

    @classmethod
    def from_depth(cls, depth, c2w, intrinsics, edges, placeholder=0, near=DEFAULT_NEAR, alpha=DEFAULT_ALPHA, beta=DEFAULT_BETA,
                   device="cuda"):
        """From depth frames and poses of the keyframes themselves: depth[k], c2w[k] belong to keyframe k of the list build_graph
        was given, so edge e runs from depth[idii[e] - placeholder] to depth[idjj[e] - placeholder]."""
        src = _index_list(edges[0], "idii") - int(placeholder)
        dst = _index_list(edges[1], "idjj") - int(placeholder)
        flow, occ = pair_cues(depth, c2w, intrinsics, list(zip(src.tolist(), dst.tolist())), near, alpha, beta, device)
        E, H, W, _ = flow.shape
        return cls(flow.reshape(E, H * W, 2), (occ == 0).reshape(E, H * W), H, W)

    @torch.no_grad()
    def select(self, sampling_idx, idii):
        """select_flow_uv: sampling_idx [b, n] pixel indices (row * W + column) of the batch's frames, idii [E] the batch row of every
        edge's source frame -> (flow [E, n, 2] fp32, mask [E, n] bool), the ``ground_truth["flow"]`` and ``["flow_mask"]`` of the
        iteration.  One launch; an index outside the image gives flow 0 and mask false."""
        dev = self.flows.device
        E = self.flows.shape[0]
        s = torch.as_tensor(sampling_idx)
        if s.dim() != 2 or s.is_floating_point():
            raise ValueError("sampling_idx: [b, n] integers")
        r = torch.as_tensor(idii)
        if r.dim() != 1 or r.shape[0] != E or r.is_floating_point():
            raise ValueError(f"idii: [{E}] integers")
        s = s.to(dev, torch.int64).contiguous()
        r = r.to(dev, torch.int64).contiguous()
        b, n = s.shape
        out = torch.empty(E, n, 2, dtype=torch.float32, device=dev)
        mask = torch.empty(E, n, dtype=torch.bool, device=dev)
        check(lib.nsa_flowcue_select(ptr(self.flows), ptr(self.masks), E, self.H * self.W, ptr(s), b, n, ptr(r), ptr(out),
                                     ptr(mask), stream(dev)))
        return out, mask


# ------------------------------------------------------------------------------------------------------------------- command line
def write_sequence(depth, c2w, intrinsics, out_dir, interval=10, rad=2, near=DEFAULT_NEAR, chunk=16, compress=True, device="cuda"):
    """A ``*_pair`` directory for a whole sequence: the four files of every pair of ``pair_list(n, interval, rad)``, ``chunk``
    unordered pairs per pass over the device.  Returns the number of pairs written."""
    pairs = pair_list(len(c2w), interval, rad)[0::2]                      # (i, j) with i > j; the list holds (j, i) next to it
    P = _as_numpy(c2w, np.float64)
    K4 = _intrinsics4(intrinsics, len(P))
    K = np.tile(np.eye(4), (K4.shape[0], 1, 1))                           # as matrices: a stack of four rows would read as one matrix
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = K4.T
    for lo in range(0, len(pairs), chunk):
        part = pairs[lo:lo + chunk]
        frames = sorted({f for p in part for f in p})
        at = {f: k for k, f in enumerate(frames)}
        local = [(at[i], at[j]) for i, j in part]
        flow, occ = pair_cues(torch.as_tensor(np.asarray(depth)[frames]), P[frames], K[frames] if K.shape[0] > 1 else K[0],
                              local + [(j, i) for i, j in local], near, device=device)
        flow, occ = flow.cpu().numpy(), occ.cpu().numpy()
        m = len(part)
        for k, (i, j) in enumerate(part):
            write_pair(out_dir, i, j, flow[k], flow[m + k], occ[k], occ[m + k], compress)
            write_pair(out_dir, j, i, flow[m + k], flow[k], occ[m + k], occ[k], compress)
    return 2 * len(pairs)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.flow_cues",
                                 description="Write the flow / occlusion files of a sequence from its depth frames and poses.")
    ap.add_argument("--depth", required=True, help="directory of *.depth.png (uint16 millimetres) or *.npy (metres) frames")
    ap.add_argument("--poses", required=True, help="camera-to-world poses: .npy, text file, or directory of *.pose.txt")
    ap.add_argument("--intrinsics", type=float, nargs=4, required=True, metavar=("FX", "FY", "CX", "CY"))
    ap.add_argument("--out", required=True, help="the *_pair directory to write")
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--rad", type=int, default=2)
    ap.add_argument("--near", type=float, default=DEFAULT_NEAR)
    args = ap.parse_args(argv)
    from .mesh_render import read_depth_dir, read_poses    # (no cycle: only the command line needs the mesh tools)
    c2w = read_poses(args.poses)
    depth = read_depth_dir(args.depth, len(c2w))
    n = write_sequence(depth, c2w, args.intrinsics, args.out, args.interval, args.rad, args.near)
    print(f"{args.out}: {n} pairs of {depth.shape[1]} x {depth.shape[2]}")


if __name__ == "__main__":
    main()
