// render_sdfnet4.hip compiled with plain bf16 GEMM operands (fp32 accumulate): the optional "bf16 MLP" precision mode.
// Everything in namespace nsa becomes nsa_bf16, every entry point nsa_xxx becomes nsa_xxx_bf16.
// Contraction: the resident persistent kernels and the staged ones include the SAME tile statements (sdfnet4_*_body.inc) and are meant to
// agree bit for bit.  Under the compiler's default (fuse a * b + c wherever the optimiser sees one, across statements) each kernel
// function fused on its own terms: the fine backward's two forms differed in the last bits of a few operands, hence by a bf16 rounding
// flip at 17 of 40 971 points (tests/test_gemm_bf16_gpu.py).  "on" fuses only inside one expression -- a property of the source, the
// same in every function that includes it.
#pragma clang fp contract(on)
#define NSA_PIECES 1
#define nsa nsa_bf16
#define NSA_ENTRY(x) x##_bf16
#include "render_sdfnet4.hip"
