"""Host restatement of the summation ORDER of the decode GEMV (skv_gemv.hip, skv_gemv_frame.h), bit for bit.

The integer banks of tests/dense_ref.py give the same sum in every order of accumulation, so they cannot see a loop that
multiplies its k-steps in another order.  This module states the order itself, for Gaussian data:

  * a k-step is 512 elements; lane l of the wave holds elements 512 s + 8 l .. 8 l + 7 of step s, one f32 accumulator per
    element slot (4 packed pairs), and runs ONE fused multiply-add chain per slot over the steps ascending; a partial last
    step (K % 512 elements) extends the chains of the lanes below (K % 512) / 8 only, last;
  * skv_gemv_row_total: ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)) per lane, then the wave tree - pairs of
    neighbouring lanes, six levels (wave_tree_sum: xor 1, 2, the two mirrors, xor 16, 32; IEEE addition commutes, so the
    mirrors add the same two numbers);
  * the total is rounded to bf16 (and, with a bias: bf16(bf16(total) + bias)).

The fused multiply-add is evaluated in f64: the product of two bf16 values has 16 significant bits and is exact there, and
the sum product + accumulator is checked to be exact in f64 with the TwoSum error term, so rounding it to f32 is the one
rounding the hardware instruction makes.  A step where the f64 sum is NOT exact would round twice: `row_totals` counts those
steps and `restate` asserts there are none - a condition on the inputs (met by choosing the seed on the CPU), not a
tolerance.  tests/test_gemv_order_ref_cpu.py checks this module against exact rational arithmetic."""
import numpy as np
import torch

import dense_ref as dr

STEP = 512
# (N, K, seed) of the plain launches of tests/test_gpu_gemv_order.py: eight k-steps (all requested before the first FMA at two rows
# per wave), 28 k-steps (steady state and drain of the pipeline), one k-step + an 8-element tail.  Seeds chosen on the CPU
# (test_gemv_order_ref_cpu.py keeps them honest): no inexact f64 step.
PLAIN_CASES = [(64, 4096, 1), (24, 14336, 1), (16, 520, 1)]
NORM_CASE = (64, 4096, 2)             # the NORM plain launch (x from dense_ref.norm_inputs: the norm itself is exact)
Q_CASE = dict(Hq=4, Hkv=1, K=4096, seed=3)     # skv_q_gemv_rope, one KV group


def f64(t):
    """bf16 / f32 torch tensor -> numpy f64 (exact)"""
    return t.float().double().numpy()


def gaussian(N, K, seed, w_std=0.05):
    """(w bf16 [N, K], x bf16 [K], bias bf16 [N]): Gaussian values of realistic magnitudes, CPU generator, arranged so that the
    ORDER of the f32 sums shows in the bf16 outputs.  On plain Gaussian rows it hardly does: another order moves an f32 total
    by an ulp or two, 2^-15 of a bf16 ulp.  So with h = the whole k-steps / 2: x repeats its first h steps in its second h, and
    every odd row of w carries the negated first h steps in its second h.  An odd row's exact sum (tail aside) is 0 and what
    the kernel returns is the rounding residue of its f32 chains - a number that every change of order replaces by another.
    Even rows stay ordinary dot products."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * w_std).bfloat16()
    x = torch.randn(K, generator=g).bfloat16()
    bias = (torch.randn(N, generator=g) * 0.1).bfloat16()
    h = (K // STEP) // 2 * STEP
    x[h:2 * h] = x[:h]
    w[1::2, h:2 * h] = -w[1::2, :h]
    return w, x, bias


def symmetric_norm_inputs(K, seed):
    """Inputs of the fused residual add + RMSNorm for which the norm is exact and its output Gaussian: h = x + residual = +-2
    element-wise as in dense_ref.norm_inputs, so mean(h^2) = 4 and h * rstd = +-1 (eps = 0) or +-0.99999875 (eps = 1e-5) and
    xn = bf16(h * rstd * w_norm) = +-w_norm for ANY bf16 w_norm (the factor is 2^-19 from 1, a bf16 ulp is 2^-8) - w_norm is
    Gaussian here, 8 significant bits, so the products of the GEMV have 16 like those of real data.  The second half of every
    vector repeats the first, so that the odd rows of `gaussian` cancel on xn.  bf16 tensors: x, residual, w_norm, h, xn."""
    n = dr.norm_inputs(K, seed, residual=True)
    g = torch.Generator().manual_seed(seed + 7)
    wn = (1.0 + 0.3 * torch.randn(K, generator=g)).bfloat16()
    out = dict(x=dr.to_bf16(n["x"]), residual=dr.to_bf16(n["residual"]), w_norm=wn, h=dr.to_bf16(n["h"]))
    out["xn"] = ((n["h"] // 2).float() * wn.float()).bfloat16()          # exact: +-w_norm
    for k in out:
        out[k][K // 2:] = out[k][:K // 2].clone()
    return out


def fma32(a, b, acc):
    """f32 fma(a, b, acc) for bf16-valued a, b and f32 acc (all numpy f64 arrays holding those values).  Returns (result as
    f64 holding an f32 value, number of elements whose f64 sum was inexact)."""
    p = a * b                                  # exact: 8 x 8 significant bits
    s = p + acc
    bb = s - p
    err = (p - (s - bb)) + (acc - bb)          # TwoSum: s + err == p + acc exactly
    return s.astype(np.float32).astype(np.float64), int(np.count_nonzero(err))


def lane_chains(w, x, order=None):
    """The 64 x 8 accumulators of every row after all k-steps: (acc f64 [N, 64, 8] holding f32 values, inexact steps).
    order: a permutation of the whole k-steps (default ascending) - the CPU test swaps two to show the bits move."""
    w, x = f64(w), f64(x)
    N, K = w.shape
    steps, tail = K // STEP, K % STEP
    acc = np.zeros((N, 64, 8))
    bad = 0
    for s in (range(steps) if order is None else order):
        ws = w[:, s * STEP:(s + 1) * STEP].reshape(N, 64, 8)
        xs = x[s * STEP:(s + 1) * STEP].reshape(1, 64, 8)
        acc, b = fma32(ws, xs, acc)
        bad += b
    if tail:
        lanes = tail // 8
        ws = w[:, steps * STEP:].reshape(N, lanes, 8)
        xs = x[steps * STEP:].reshape(1, lanes, 8)
        acc[:, :lanes], b = fma32(ws, xs, acc[:, :lanes])
        bad += b
    return acc, bad


def row_totals(w, x, order=None):
    """(f32 totals [N] as torch f32, inexact steps): the chains, skv_gemv_row_total's pair tree, the wave tree."""
    acc, bad = lane_chains(w, x, order)
    a = torch.from_numpy(acc).float()                       # exact: the values are f32
    lane = ((a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])) + ((a[..., 4] + a[..., 5]) + (a[..., 6] + a[..., 7]))
    v = lane                                                # [N, 64]
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0], bad


def finish(tot, bias=None):
    """f32 totals -> the launch's bf16 outputs"""
    y = tot.bfloat16()
    return y if bias is None else (y.float() + bias.float()).bfloat16()


def restate(w, x, bias=None):
    """Expected bf16 outputs [N] of y = W . x (+ bias); asserts the inputs leave no doubly rounded step."""
    tot, bad = row_totals(w, x)
    assert bad == 0, f"{bad} fused multiply-adds are not exact in f64 on these inputs: choose another seed"
    return finish(tot, bias)


def norm_case():
    """The NORM plain launch: the weights of `gaussian`; x, residual, w_norm from symmetric_norm_inputs, whose residual add and
    RMSNorm are exact, so the order of the GEMV's f32 sums is all that decides the bits."""
    N, K, seed = NORM_CASE
    w, _, bias = gaussian(N, K, seed)
    n = symmetric_norm_inputs(K, seed)
    return dict(N=N, K=K, w=w, bias=bias, n=n, xn=n["xn"])


def q_case(glm):
    """skv_q_gemv_rope with one KV group: fused [q; k; v] Gaussian weights (the launch streams the q rows), exact norm inputs, a
    cos / sin table, q_override values."""
    Hq, Hkv, K, seed = Q_CASE["Hq"], Q_CASE["Hkv"], Q_CASE["K"], Q_CASE["seed"] + int(glm)
    w, _, bias = gaussian((Hq + 2 * Hkv) * 128, K, seed)
    n = symmetric_norm_inputs(K, seed)
    g = torch.Generator().manual_seed(seed + 100)
    cs = (torch.rand(40, 64 if glm else 128, generator=g) * 2 - 1).bfloat16()
    ov = torch.randn(1, Hq, 128, generator=g).bfloat16()
    return dict(Hq=Hq, Hkv=Hkv, K=K, glm=glm, w=w, bias=bias, n=n, xn=n["xn"], cs=cs, ov=ov)
