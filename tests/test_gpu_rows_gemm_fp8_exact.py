"""GPU: the FP8 rows kernel (skv_rows_gemm_fp8.hip, 2..32 token rows against e4m3 weights) against tests/dense_ref.py, bit for bit.

The banks' weights {+-1, +-2, +-3} are e4m3 numbers and the per-row scales are powers of two from 2^-2 .. 2^2: the expected output
is scale * (an integer computed in int64), at most 8 significant bits, so every order of f32 accumulation gives it and bf16 holds
it - raw bits are compared.  The SiLU pair form carries dense_ref.SILU_RTOL; the Gaussian case one bf16 ulp and a flip share
measured from two CPU f32 evaluations (tests/fp8_rows_ref.py).  Every output buffer carries sentinels past its end."""
import pytest
import torch

import dense_ref as dr
import fp8_rows_ref as rr
import util
from dense_ref import expected_branch
from test_gpu_gemv_fp8_exact import (DEV, PAD, SENT, _L, assert_bits, assert_silu, dev16, fp8_weights, pair_scales, pow2_scales,
                                     scaled, sentinel_buf)

pytestmark = pytest.mark.gpu

ROWS_M = (2, 8, 9, 16, 17, 32)
ROWS_K = (64, 192, 576, 2112, 8256)           # K / 64 = 1, 3, 9, 33, 129
ROWS_N = (48, 2 * 1003, 6160, 16400)          # 2 * 1003: the SiLU pair form


def test_rows_fp8_shapes_reach_every_branch():
    reached = {expected_branch(M, N, K) for M in ROWS_M for N in ROWS_N for K in ROWS_K}
    assert reached == {"g1 paired", "g2 1/2x8", "g1", "g2 2/4x4", "g2 2/2x8", "g2 2/1x8", "g1 two tiles"}
    assert len(reached) == 7                                               # the seven return statements of skv_rows_pick
    assert expected_branch(17, 48, 8256) == "g2 2/1x8" and expected_branch(17, 48, 2112) == "g1 two tiles"
    assert expected_branch(16, 6160, 64) == "g2 1/2x8" and expected_branch(32, 16400, 64) == "g2 2/4x4"
    # the SiLU pair form (N = 2006) and the plain form both reach the two first-generation tile counts and the 1x8 shape
    assert {expected_branch(M, 2006, K) for M in ROWS_M for K in ROWS_K} == {"g1 paired", "g1", "g1 two tiles", "g2 2/1x8"}


def run_rows(bank, w8, scale_d, x, bias, silu, M):
    """One launch per matrix of the bank: y [launches, M, No]; the row past M and PAD more values keep the sentinel."""
    _lib, L, st = _L()
    p = _lib.ptr
    N, K = bank.rows, bank.K
    No = N // 2 if silu else N
    y = sentinel_buf(bank.launches, (M + 1) * No + PAD)
    for l in range(bank.launches):
        rc = L.skv_linear_rows_fp8(p(w8[l * N:(l + 1) * N]), p(scale_d[l * N:(l + 1) * N]), p(x), p(bias), p(y[l]), M, N, K, int(silu), st)
        assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((y[:, M * No:] == SENT).all()), "written past the last token row"
    return y[:, :M * No].view(bank.launches, M, No)


@pytest.mark.parametrize("K", ROWS_K)
@pytest.mark.parametrize("N", ROWS_N)
def test_rows_fp8_exact(N, K):
    """skv_linear_rows_fp8 at every M of ROWS_M: K / 64 = 1, 3, 9 (fewer k-steps than the 8 split-K waves, or barely more), 33
    (single steps only in the first generation), 129 (unrolled batches + a tail); ragged N (48, 6160 = 385 tiles, 1003 pairs)."""
    silu = N == 2 * 1003
    I = N // 2
    xi, colsign = dr.structured_x(max(ROWS_M), K, seed=N + K)
    bank = dr.pair_bank(I, K, seed=N + K, colsign=colsign) if silu else dr.plain_bank(N, K, seed=N + K)
    w8 = fp8_weights(bank)
    x_d = dev16(xi)
    sums = bank.sums(xi)                                           # [M, launches, N]
    if silu:
        # one scale set for every token row: the gate rows' cap (|scale * g| <= 48) is taken over the largest |g| of the rows
        scale = pair_scales(sums.abs().amax(0), I, seed=N + K + 1)
    else:
        scale = pow2_scales(bank.launches * N, seed=N + K + 1)
    scale_d, sv = scale.to(DEV), scale.view(bank.launches, N)
    for M in ROWS_M:
        what = f"rows fp8 M {M} N {N} K {K} [{expected_branch(M, N, K)}]"
        xm = x_d[:M].contiguous()
        t = scaled(sums[:M], sv)                                   # bf16 [M, launches, N], exact
        if silu:
            g, u = t[..., :I], t[..., I:]
            assert bool((g != 0).all()) and bool((u != 0).all())
            y = run_rows(bank, w8, scale_d, xm, None, True, M)
            assert_silu(y.permute(1, 0, 2), dr.silu_mul_ref(g, u), what)
        else:
            for bias in (None, dr.integer_bias(N, seed=N + M)):
                bias_d = None if bias is None else dev16(bias)
                y = run_rows(bank, w8, scale_d, xm, bias_d, False, M)
                # bias: bf16(bf16r(t) + bias) - t is a bf16 number, t + bias is exact in f32 and rounded once
                want = t if bias is None else (t.float() + bias.float()).bfloat16()
                assert_bits(y.permute(1, 0, 2), want, what + f" bias {bias is not None}")


@pytest.mark.parametrize("M", [9, 2, 17])
def test_rows_fp8_byte_decoding_and_operand_pairing(M):
    """254 rows, one per non-NaN byte: row n holds its byte once, at column 17 n mod 128, zeros elsewhere - all 16 byte positions
    of a lane's load and both MFMA halves occur.  x[m][k] = 2^(m % 3), scale 1: y[m][n] = 2^(m % 3) * e4m3(byte n), exactly.  The
    expectation is torch's float8_e4m3fn cast on the CPU: OCP e4m3fn against fnuz differ by a factor 2 on every normal value and
    on the meaning of 0x80.  (M = 9 is the first generation's plain form; 2 the paired token operand, 17 the two token tiles.)"""
    _lib, L, st = _L()
    p = _lib.ptr
    K = 128
    b = torch.tensor([v for v in range(256) if v not in (0x7F, 0xFF)], dtype=torch.uint8)
    N = b.numel()
    assert N == 254
    cols = (17 * torch.arange(N)) % K
    assert set((cols % 16).tolist()) == set(range(16)) and set((cols // 64).tolist()) == {0, 1}
    w = torch.zeros(N, K, dtype=torch.uint8)
    w[torch.arange(N), cols] = b
    val = b.view(torch.float8_e4m3fn).float()
    assert float(val[0x08]) == 2.0 ** -6 and float(val[0x01]) == 2.0 ** -9 and float(val[0x7E]) == 448.0
    assert int(b[0x7F]) == 0x80 and float(val[0x7F]) == 0.0                     # (index 0x7F: byte 0x80, minus zero)
    xm = torch.exp2((torch.arange(M) % 3).float()).view(M, 1).expand(M, K).contiguous()
    want = xm[:, :1] * val.view(1, N)                   # <= 4 significant bits: exact in bf16 (subnormal e4m3 values included)
    assert torch.equal(want.bfloat16().float(), want)
    y = sentinel_buf((M + 1) * N + PAD)
    wd, sd, xd = w.to(DEV), torch.ones(N, device=DEV), xm.bfloat16().to(DEV)
    rc = L.skv_linear_rows_fp8(p(wd), p(sd), p(xd), 0, p(y), M, N, K, 0, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = y[:M * N].view(M, N).cpu().float()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong; first (token, byte index) {bad[0].tolist()}: byte {hex(int(b[bad[0][1]]))} gave " \
                             f"{float(got[tuple(bad[0])])}, e4m3fn says {float(want[tuple(bad[0])])}"
    assert bool((y[M * N:] == SENT).all())


# Outputs of the random case whose bf16 result differs from bf16(f64), for the two plain CPU f32 evaluations of the same contract
# (tests/fp8_rows_ref.py; profiles/fp8_rows_flip_shares.txt; tests/test_fp8_rows_cpu.py recomputes them).  The kernel's order -
# MFMA trees, two accumulators, split-K partials - is neither of the two, hence the project's factor 4 on the larger share.
ROWS_FP8_CPU_FLIPS = (10, 6)                      # (sequential, pairwise) of 104,720 outputs at (M, N, K) = (17, 6160, 1088)
ROWS_FP8_OUTPUTS = 104720
ROWS_FP8_SHARE_BOUND = 4 * max(ROWS_FP8_CPU_FLIPS) / ROWS_FP8_OUTPUTS


def test_rows_fp8_random_data_within_one_ulp():
    _lib, L, st = _L()
    c = rr.RANDOM_ROWS_FP8
    M, N, K = c["M"], c["N"], c["K"]
    assert M * N == ROWS_FP8_OUTPUTS
    w8, scale, x, ref64 = rr.random_case(**c)
    y = sentinel_buf(M + 1, N)
    wd, sd, xd = w8.to(DEV), scale.to(DEV), x.to(DEV)
    rc = L.skv_linear_rows_fp8(_lib.ptr(wd), _lib.ptr(sd), _lib.ptr(xd), 0, _lib.ptr(y), M, N, K, 0, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((y[M] == SENT).all())
    want = dr.round_bf16(ref64).bfloat16()
    d = util.ulp_diff_bf16(y[:M].cpu(), want)
    share = float((d > 0).double().mean())
    print(f"rows fp8 random data: values {d.numel()}  differing {int((d > 0).sum())} (share {share:.3e}, bound "
          f"{ROWS_FP8_SHARE_BOUND:.3e})  max ulp {int(d.max())}")
    assert int(d.max()) <= 1, f"an output is {int(d.max())} bf16 ulps from bf16(f64)"
    assert share <= ROWS_FP8_SHARE_BOUND, f"share of outputs that differ from bf16(f64) {share:.3e} > {ROWS_FP8_SHARE_BOUND:.3e}"
