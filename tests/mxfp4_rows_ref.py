"""CPU references for the MXFP4 rows kernel (skv_linear_rows_mxfp4); no GPU import.  Not collected.

Built on tests/mxfp4_ref.py (the format, MxBank, the f64 decode) and tests/dense_ref.py (the structured inputs, the SiLU reference,
the branch skv_rows_pick takes - RowsMxfp4 uses that tree unchanged, so dense_ref.expected_branch holds for it):

  - RowsBank: an MxBank's exact outputs for M token rows of dense_ref.structured_x at once.  Weights {+-1, +-2, +-3} (e2m1
    numbers), the scale of row r and block b 2^(e_r + ((r + b) & 1)) with e_r in {-2 .. 1}, x in {+-1 .. +-4}: a row's terms are
    integers times 2^e_r whose magnitudes sum to at most 8 * 3 * 4 * 2 = 192 units - every partial sum in every order is exact in
    f32 and the total is a bf16 number.  expected() asserts both, and that the f64 decode of the packed bytes gives the same.
  - decode_probe_rows: single-element rows for the kernel's 128-element k-step.
  - the Gaussian case with its f64 reference and two plain CPU f32 evaluations (sequential, pairwise) of the same contract: the
    share of outputs an f32 accumulation flips against bf16(f64) (profiles/mxfp4_rows_flip_shares.txt)."""
import numpy as np
import torch

import dense_ref as dr
import mxfp4_ref as mr
import util

ROWS_M = (2, 8, 9, 16, 17, 32)
ROWS_K = (128, 384, 1152, 4224, 16512)         # K / 128 = 1, 3, 9, 33, 129
ROWS_N = (48, 2 * 1003, 6160, 16400)           # 2 * 1003: the SiLU pair form
DECODE_CHECK_ROWS = 1024                       # rows of a large bank whose packed bytes are decoded in f64 (evenly spread)


class RowsBank:
    """A dense_ref Bank with per-row exponents e_r, as MXFP4, for many token rows.  pack() makes the bytes (mxfp4_ref.MxBank)."""

    def __init__(self, bank, row_exp):
        self.bank, self.K, self.rows, self.launches = bank, bank.K, bank.rows, bank.launches
        self.R = bank.cols.shape[0]
        self.row_exp = row_exp.view(self.R).to(torch.int64)
        r = torch.arange(self.R).view(self.R, 1)
        self.factor = 1 + ((r + bank.cols // mr.BLOCK) & 1)            # the alternation between the blocks of a row
        self._mx = None

    def units(self, x):
        """x int64 [M, K] -> (units int64 [M, launches, rows], sum of |terms| int64 [M, R]): t = units * 2^e_r"""
        terms = x[:, self.bank.cols] * (self.bank.vals * self.factor)
        return terms.sum(-1).view(x.shape[0], self.launches, self.rows), terms.abs().sum(-1)

    def pack(self):
        if self._mx is None:
            self._mx = mr.MxBank(self.bank, self.row_exp)
        return self._mx

    def expected(self, x, decode=True):
        """The exact outputs as f64 [M, launches, rows] (bf16 numbers), with the assertions the construction rests on: the
        magnitudes of a row's terms sum below 2^24 units (every partial sum in every order is exact in f32), the total is a bf16
        number, and (decode) the f64 decode of the packed bytes times x gives the same numbers - for every row of a bank of up to
        DECODE_CHECK_ROWS rows, for that many evenly spread rows of a larger one."""
        u, mags = self.units(x)
        assert int(mags.max()) < 2 ** 24 and int(u.abs().max()) <= 256
        t = u.double() * torch.ldexp(torch.ones(self.R, dtype=torch.float64), self.row_exp).view(1, self.launches, self.rows)
        assert torch.equal(t.bfloat16().double(), t)
        if decode:
            mx = self.pack()
            pick = torch.arange(self.R) if self.R <= DECODE_CHECK_ROWS else torch.linspace(0, self.R - 1, DECODE_CHECK_ROWS).long()
            w = mr.decode(mx.w4[pick], mx.w_scale[pick])               # f64 [rows picked, K]
            ref = x.double().numpy() @ w.T
            assert np.array_equal(ref, t.view(x.shape[0], self.R)[:, pick].numpy())
        return t


def plain_rows_bank(N, K, seed):
    bank = dr.plain_bank(N, K, seed, P=mr.MX_P)
    assert bank.covers_every_column()
    return RowsBank(bank, mr.row_exponents(bank.cols.shape[0], seed + 1))


def pair_rows_bank(I, K, seed, colsign, x):
    """[gate; up] rows whose products share a sign for every token row (dense_ref.pair_bank).  One exponent set serves all token
    rows: a gate row keeps the largest e_r <= its draw with |g| <= 48 for the LARGEST |g| over the rows of x - the cap
    pair_scales (tests/test_gpu_gemv_fp8_exact.py) puts on FP8 row scales.  |units| <= 96, so the cap is >= -1 and every e_r stays
    in {-2 .. 1}; |units| >= 4, so 1 <= |g| <= 48 and g, u are never 0."""
    bank = dr.pair_bank(I, K, seed, colsign, P=mr.MX_PAIR_P)
    R = bank.cols.shape[0]
    e = mr.row_exponents(R, seed + 1)
    u = RowsBank(bank, e).units(x)[0].abs().view(x.shape[0], R)
    assert int(u.min()) >= 4 and int(u.max()) <= 96
    hi = torch.floor(torch.log2(48.0 / u.amax(0).double())).to(torch.int64)
    gate = (torch.arange(R) % (2 * I)) < I
    e = torch.where(gate, torch.minimum(e, hi), e)
    assert int(e.min()) >= -2 and int(e.max()) <= 1
    rb = RowsBank(bank, e)
    g = (rb.units(x)[0].double() * torch.ldexp(torch.ones(R, dtype=torch.float64), e).view(1, rb.launches, 2 * I))[..., :I].abs()
    assert bool((g >= 1).all()) and bool((g <= 48).all())
    return rb


def exact_case(N, K):
    """(rows bank, x int64 [max M, K], silu) of one (N, K) of the GPU grid, seeds as tests/test_gpu_rows_gemm_fp8_exact.py"""
    silu = N == 2 * 1003
    xi, colsign = dr.structured_x(max(ROWS_M), K, seed=N + K)
    rb = pair_rows_bank(N // 2, K, N + K, colsign, xi) if silu else plain_rows_bank(N, K, N + K)
    return rb, xi, silu


# ------------------------------------------------------------------------------------------------------- decode probe
PROBE_K = 256                                   # two k-steps of 128 elements
PROBE_M = (2, 9, 17)                            # the paired token operand, one token tile, two token tiles


def decode_probe_rows(K=PROBE_K):
    """Single-element rows for the rows kernel: (w4 [R, K / 2], w_scale [R, K / 32], col int64 [R], value f64 [R]).
    Part 1: all 16 nibble codes x both nibbles x all 16 byte positions of a lane's 16-byte load x lane groups g = 0..3 x the two
    k-steps - element 128 s + 32 g + 2 byte + nibble - the element's block at scale byte 128 (2.0) and every other block of the
    row at 125 (a scale byte taken from another lane group or k-step shows).  Part 2: every code at scale bytes
    {27, 126, 127, 128, 227}.  Part 3: code 6 (4.0) at every scale byte 27 .. 227."""
    rows = [(128 * s + 32 * g + 2 * byte + nib, code, 128)
            for code in range(16) for nib in range(2) for byte in range(16) for g in range(4) for s in range(K // 128)]
    rows += [(32 * 1 + 7, code, sb) for code in range(16) for sb in (27, 126, 127, 128, 227)]
    rows += [(128 + 32 * 2 + 18, 6, sb) for sb in range(27, 228)]
    R = len(rows)
    w4 = torch.zeros(R, K // 2, dtype=torch.uint8)
    sc = torch.full((R, K // mr.BLOCK), 125, dtype=torch.uint8)
    col = torch.tensor([r[0] for r in rows])
    val = np.zeros(R)
    for i, (k, code, sb) in enumerate(rows):
        w4[i, k // 2] = code << (4 * (k & 1))
        sc[i, k // mr.BLOCK] = sb
        val[i] = (-1.0 if code & 8 else 1.0) * mr.E2M1[code & 7] * 2.0 ** (sb - 127)
    assert np.array_equal(mr.decode(w4, sc)[np.arange(R), col.numpy()], val)
    assert int((mr.decode(w4, sc) != 0).sum(axis=1).max()) == 1
    return w4, sc, col, torch.from_numpy(val)


def probe_x(M, K=PROBE_K):
    """x[m][k] = 2^(m % 3), f32 [M, K]"""
    return torch.exp2((torch.arange(M) % 3).float()).view(M, 1).expand(M, K).contiguous()


# ------------------------------------------------------------------------------------ random-data companion (flip shares)
# The seed is the first from M + N + K on at which BOTH CPU f32 evaluations below stay within one bf16 ulp of bf16(f64) on every
# output: at M + N + K itself one output cancels to 3.2e-6 among terms of 4e-2 and the sequential f32 sum is 8 ulps off - the
# one-ulp criterion of the GPU test asks of the kernel what a plain f32 accumulation of the same contract can meet.
RANDOM_ROWS_MXFP4 = dict(M=17, N=6160, K=1152, seed=17 + 6160 + 1152 + 1)


def random_case(M, N, K, seed):
    """(w4 [N, K / 2], w_scale [N, K / 32], x bf16 [M, K], ref64 [M, N] = x . decode(w4, w_scale) in f64, not rounded)"""
    from shadowkv_amd import tensor_op
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    x = torch.randn(M, K, generator=g).bfloat16()
    w4, sc = tensor_op.quantize_mxfp4_rows(w)
    return w4, sc, x, x.double() @ torch.from_numpy(mr.decode(w4, sc)).t()


def flipped(sum32, ref64):
    """Outputs whose bf16(sum32) differs from bf16(ref64) (no multiply after the sum: the scales are in the weights):
    (count, total, largest distance in bf16 ulps)"""
    got, want = dr.round_bf16(sum32.double()), dr.round_bf16(ref64)
    return int((got != want).sum()), got.numel(), int(util.ulp_diff_bf16(got.bfloat16(), want.bfloat16()).max())


def cpu_flips(case=None):
    """((sequential count, total, max ulp), (pairwise count, total, max ulp)) on the case"""
    w4, sc, x, ref64 = random_case(**(case or RANDOM_ROWS_MXFP4))
    wf = torch.from_numpy(mr.decode(w4, sc)).float()                   # exact: 2 significant bits
    return flipped(dr.f32_sequential(wf, x), ref64), flipped(dr.f32_pairwise(wf, x), ref64)
