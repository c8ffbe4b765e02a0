"""The random-data case of the FP8 rows kernel (skv_linear_rows_fp8) and its two CPU yardsticks; no GPU import.

Gaussian weights go through tensor_op.quantize_fp8_rows, the activations are Gaussian bf16.  The expected output is
bf16(scale[n] * sum_k e4m3(byte[n][k]) * x[m][k]) with the sum and the product in f64.  The two plain f32 evaluations of the same
contract (dense_ref.f32_sequential / f32_pairwise over the decoded bytes, then ONE f32 multiply by the scale) give the share of
outputs an f32 accumulation flips against that reference; tests/test_gpu_rows_gemm_fp8_exact.py holds the kernel to 4 x the
larger one (profiles/fp8_rows_flip_shares.txt)."""
import torch

import dense_ref as dr

RANDOM_ROWS_FP8 = dict(M=17, N=6160, K=1088, seed=17 + 6160 + 1088)


def random_case(M, N, K, seed):
    """(w8 e4m3 [N, K], scale f32 [N], x bf16 [M, K], ref64 [M, N] = scale * (x . decode(w8)) in f64, not rounded)"""
    from shadowkv_amd import tensor_op
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    x = torch.randn(M, K, generator=g).bfloat16()
    w8, scale = tensor_op.quantize_fp8_rows(w)
    return w8, scale, x, (x.double() @ w8.double().t()) * scale.double()


def flipped(sum32, scale, ref64):
    """Outputs whose bf16(f32(scale * sum32)) differs from bf16(ref64): (count, total)"""
    got = dr.round_bf16((sum32 * scale).double())                 # one f32 multiply, one rounding
    return int((got != dr.round_bf16(ref64)).sum()), got.numel()


def cpu_flips(case=None):
    """((sequential count, total), (pairwise count, total)) on the case"""
    w8, scale, x, ref64 = random_case(**(case or RANDOM_ROWS_FP8))
    wf = w8.float()
    return flipped(dr.f32_sequential(wf, x), scale, ref64), flipped(dr.f32_pairwise(wf, x), scale, ref64)
