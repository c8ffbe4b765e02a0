"""GPU: the MXFP4 rows kernel (skv_rows_gemm_mxfp4.hip, 2..32 token rows against e2m1 nibbles + e8m0 block scales) against
tests/mxfp4_rows_ref.py, bit for bit.

The banks' weights {+-1, +-2, +-3} are e2m1 numbers, the block scales powers of two from 2^-2 .. 2^2 that alternate between the
blocks of a row, x and the bias small integers: every partial sum in every order is exact in f32 and the result is a bf16 number
(RowsBank.expected asserts both) - raw bits are compared.  The SiLU pair form carries dense_ref.SILU_RTOL; the decode of nibbles
and scale bytes is pinned element by element; the Gaussian case carries one bf16 ulp and a flip share measured from two CPU f32
evaluations.  Every output buffer carries sentinels past its end."""
import pytest
import torch

import dense_ref as dr
import mxfp4_rows_ref as rr
import util
from dense_ref import expected_branch          # RowsMxfp4 goes through skv_rows_pick unchanged
from mxfp4_rows_ref import ROWS_K, ROWS_M, ROWS_N
from test_gpu_gemv_mxfp4_exact import DEV, PAD, SENT, _L, assert_bits, assert_silu, dev16, sentinel_buf

pytestmark = pytest.mark.gpu


def test_rows_mxfp4_shapes_reach_every_branch():
    reached = {expected_branch(M, N, K) for M in ROWS_M for N in ROWS_N for K in ROWS_K}
    assert reached == {"g1 paired", "g2 1/2x8", "g1", "g2 2/4x4", "g2 2/2x8", "g2 2/1x8", "g1 two tiles"}
    assert len(reached) == 7                                               # the seven return statements of skv_rows_pick
    assert expected_branch(17, 48, 16512) == "g2 2/1x8" and expected_branch(17, 48, 4224) == "g1 two tiles"
    assert expected_branch(16, 6160, 128) == "g2 1/2x8" and expected_branch(32, 16400, 128) == "g2 2/4x4"
    # the SiLU pair form (N = 2006) and the plain form both reach the two first-generation tile counts and the 1x8 shape
    assert {expected_branch(M, 2006, K) for M in ROWS_M for K in ROWS_K} == {"g1 paired", "g1", "g1 two tiles", "g2 2/1x8"}


def run_rows(mx, w4, sc, x, bias, silu, M):
    """One launch per matrix of the bank: y [launches, M, No]; the row past M and PAD more values keep the sentinel."""
    _lib, L, st = _L()
    p = _lib.ptr
    N, K = mx.rows, mx.K
    No = N // 2 if silu else N
    y = sentinel_buf(mx.launches, (M + 1) * No + PAD)
    for l in range(mx.launches):
        rc = L.skv_linear_rows_mxfp4(p(w4[l * N:(l + 1) * N]), p(sc[l * N:(l + 1) * N]), p(x), p(bias), p(y[l]), M, N, K, int(silu), st)
        assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((y[:, M * No:] == SENT).all()), "written past the last token row"
    return y[:, :M * No].view(mx.launches, M, No)


@pytest.mark.parametrize("K", ROWS_K)
@pytest.mark.parametrize("N", ROWS_N)
def test_rows_mxfp4_exact(N, K):
    """skv_linear_rows_mxfp4 at every M of ROWS_M: K / 128 = 1, 3, 9 (fewer k-steps than the 8 split-K waves, or barely more), 33
    (single steps and one batch), 129 (unrolled batches + a tail); ragged N (48, 6160 = 385 tiles, 1003 pairs)."""
    rb, xi, silu = rr.exact_case(N, K)
    I = N // 2
    mx = rb.pack()
    w4, sc = mx.w4.to(DEV), mx.w_scale.to(DEV)
    x_d = dev16(xi)
    t_all = rb.expected(xi)                                        # f64 [32, launches, N], exact; the decode cross-check runs once
    for M in ROWS_M:
        what = f"rows mxfp4 M {M} N {N} K {K} [{expected_branch(M, N, K)}]"
        xm = x_d[:M].contiguous()
        t = t_all[:M].bfloat16()
        if silu:
            g, u = t[..., :I], t[..., I:]
            assert bool((g != 0).all()) and bool((u != 0).all())
            y = run_rows(mx, w4, sc, xm, None, True, M)
            assert_silu(y.permute(1, 0, 2), dr.silu_mul_ref(g, u), what)
        else:
            for bias in (None, dr.integer_bias(N, seed=N + M)):
                bias_d = None if bias is None else dev16(bias)
                y = run_rows(mx, w4, sc, xm, bias_d, False, M)
                # bias: bf16(bf16r(t) + bias) - t is a bf16 number, t + bias is exact in f32 and rounded once
                want = t if bias is None else (t.float() + bias.float()).bfloat16()
                assert_bits(y.permute(1, 0, 2), want, what + f" bias {bias is not None}")


@pytest.mark.parametrize("M", rr.PROBE_M)
def test_rows_mxfp4_nibble_byte_and_scale_decoding(M):
    """Rows with ONE non-zero nibble (mxfp4_rows_ref.decode_probe_rows), K = 256: all 16 codes x both nibbles x all 16 byte
    positions of a lane's load x lane groups g = 0..3 x two k-steps, the element's block at scale byte 128 and the row's other
    blocks at 125; every code at scale bytes {27, 126, 127, 128, 227}; code 6 at every byte 27 .. 227.  x[m][k] = 2^(m % 3):
    y[m][n] = 2^(m % 3) * value(n) exactly.  This pins the nibble order under byte_sel, the dword <-> MFMA assignment, the sign, the
    scale-byte <-> lane-group mapping and the bf16 conversion over the whole scale range.  (M = 2: the paired token operand,
    9: one token tile, 17: two.)"""
    _lib, L, st = _L()
    p = _lib.ptr
    K = rr.PROBE_K
    w4, sc, col, val = rr.decode_probe_rows(K)
    N = w4.shape[0]
    xm = rr.probe_x(M, K)
    want = xm[:, :1].double() * val.view(1, N)          # 2 significant bits times a power of two: a bf16 number
    assert torch.equal(want.bfloat16().double(), want)
    y = sentinel_buf((M + 1) * N + PAD)
    w4_d, sc_d, xd = w4.to(DEV), sc.to(DEV), xm.bfloat16().to(DEV)
    rc = L.skv_linear_rows_mxfp4(p(w4_d), p(sc_d), p(xd), 0, p(y), M, N, K, 0, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = y[:M * N].view(M, N).cpu().double()
    bad = (got != want).nonzero()
    assert torch.equal(got, want), f"{bad.shape[0]} wrong; first (token, row) {bad[0].tolist()}: column {int(col[bad[0][1]])} gave " \
                                   f"{float(got[tuple(bad[0])])}, the format says {float(want[tuple(bad[0])])}"
    assert bool((y[M * N:] == SENT).all())


# Outputs of the random case whose bf16 result differs from bf16(f64), for the two plain CPU f32 evaluations of the same contract
# (tests/mxfp4_rows_ref.py; profiles/mxfp4_rows_flip_shares.txt; tests/test_mxfp4_rows_cpu.py recomputes them).  The kernel's
# order - MFMA trees, its accumulators, split-K partials - is neither of the two, hence the project's factor 4 on the larger share.
ROWS_MXFP4_CPU_FLIPS = (2, 2)                     # (sequential, pairwise) of 104,720 outputs at (M, N, K) = (17, 6160, 1152)
ROWS_MXFP4_OUTPUTS = 104720
ROWS_MXFP4_SHARE_BOUND = 4 * max(ROWS_MXFP4_CPU_FLIPS) / ROWS_MXFP4_OUTPUTS


def test_rows_mxfp4_random_data_within_one_ulp():
    _lib, L, st = _L()
    c = rr.RANDOM_ROWS_MXFP4
    M, N, K = c["M"], c["N"], c["K"]
    assert M * N == ROWS_MXFP4_OUTPUTS
    w4, sc, x, ref64 = rr.random_case(**c)
    y = sentinel_buf(M + 1, N)
    wd, sd, xd = w4.to(DEV), sc.to(DEV), x.to(DEV)
    rc = L.skv_linear_rows_mxfp4(_lib.ptr(wd), _lib.ptr(sd), _lib.ptr(xd), 0, _lib.ptr(y), M, N, K, 0, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((y[M] == SENT).all())
    want = dr.round_bf16(ref64).bfloat16()
    d = util.ulp_diff_bf16(y[:M].cpu(), want)
    share = float((d > 0).double().mean())
    print(f"rows mxfp4 random data: values {d.numel()}  differing {int((d > 0).sum())} (share {share:.3e}, bound "
          f"{ROWS_MXFP4_SHARE_BOUND:.3e})  max ulp {int(d.max())}")
    assert int(d.max()) <= 1, f"an output is {int(d.max())} bf16 ulps from bf16(f64)"
    assert share <= ROWS_MXFP4_SHARE_BOUND, f"share of outputs that differ from bf16(f64) {share:.3e} > {ROWS_MXFP4_SHARE_BOUND:.3e}"
