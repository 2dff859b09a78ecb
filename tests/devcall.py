"""What every test that calls a kernel through the C ABI needs to hand it arguments (test infrastructure): the current stream, a
pointer or NULL, an fp32 device copy, a NaN-filled output."""
import torch


def st():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(t, dtype=torch.float32):
    return None if t is None else t.detach().to("cuda", dtype).contiguous()


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")
