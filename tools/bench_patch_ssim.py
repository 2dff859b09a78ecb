"""Time the SSIM patch-warp term: nsa_patch_ssim with the gradient at N = 65 536 patches of 5 x 5 and 11 x 11 (what a
mapping iteration of 16 x 16 x 256 patches holds), with the bytes it has to move -- pred and target read, the gradient written, one
mask byte per pixel -- over the time, and the torch restatement (model/warp.py::patch_ssim_term, forward + backward) on the same
device for context.  Device events around CALLS back-to-back launches on preallocated buffers, warm-up first, median of REPS.
usage: python tools/bench_patch_ssim.py [reps=7]"""
import sys

import torch

from benchlib import median_min_max, median_ms, positionals, time_events, write_results
from nicer_slam_amd._native import lib, check
from nicer_slam_amd.fused.warp import patch_ssim
from nicer_slam_amd.model.warp import patch_ssim_term

CALLS = 20
N = 65536


def parse_args(argv):
    return positionals(argv, reps=(int, 7))


def main(argv=None):
    REPS = parse_args(sys.argv[1:] if argv is None else argv).reps
    out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "calls per rep": CALLS, "patches": N}
    g = torch.Generator(device="cuda").manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    for p in (5, 11):
        x = torch.rand(N, p * p, 3, device="cuda", generator=g)
        y = (x + 0.05 * torch.randn(N, p * p, 3, device="cuda", generator=g)).clamp(0, 1)
        m = torch.rand(N, p * p, device="cuda", generator=g) > 0.2
        mb = m.view(torch.uint8)
        grad, loss = torch.empty_like(x), torch.empty(1, device="cuda")
        ws = torch.empty((int(lib.nsa_patch_ssim_workspace(N)) + 1) // 2, device="cuda", dtype=torch.float64)
        call = lambda: check(lib.nsa_patch_ssim(x.data_ptr(), y.data_ptr(), mb.data_ptr(), N, p, loss.data_ptr(), grad.data_ptr(),
                                                ws.data_ptr(), st))
        ms, lo, hi = median_min_max(time_events(call, REPS, CALLS))
        nbytes = 3 * 4 * x.numel() + m.numel()
        key = f"p={p}"
        out[key + " nsa_patch_ssim with gradient ms (median, min, max)"] = [ms, lo, hi]
        out[key + " bytes moved"] = nbytes
        out[key + " TB/s"] = nbytes / ms / 1e9
        out[key + " share of the 6.3 TB/s streaming ceiling"] = nbytes / ms / 1e9 / 6.3
        xr = x.clone().requires_grad_(True)

        def through_autograd():
            xr.grad = None
            patch_ssim(xr, y, m, p).backward()

        def twin():
            xr.grad = None
            patch_ssim_term(xr, y, m, p).backward()
        out[key + " fused.warp.patch_ssim forward + backward ms"] = median_ms(through_autograd, REPS)
        out[key + " torch restatement forward + backward ms"] = median_ms(twin, REPS)
        out[key + " loss"] = float(loss)
        del x, y, m, grad, xr
    write_results(out)


if __name__ == "__main__":
    main()
