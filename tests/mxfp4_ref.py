"""CPU restatement of the weight-only MXFP4 format in numpy / f64, independent of shadowkv_amd.tensor_op:
decode of a (w4, w_scale) pair, the block quantiser, the decode GEMV, and the builders of the EXACT test cases of
tests/test_gpu_gemv_mxfp4_exact.py.  Not collected (no test_ prefix).

Format: w4 uint8 [N, K / 2], element 2i of a row in the low nibble of byte i and element 2i + 1 in the high nibble; a nibble is
sign (bit 3) + e2m1 code (bits 0..2) with the values E2M1; w_scale uint8 [N, K / 32] e8m0: 2^(byte - 127) for 32 consecutive
elements.  W[n][k] = 2^(w_scale[n][k / 32] - 127) * e2m1(nibble[n][k]).

The exact construction (after tests/dense_ref.py): a dense_ref Bank with P = 8 nonzeros {+-1, +-2, +-3} per row - all e2m1
numbers - and for row r and block b the scale 2^(e_r + ((r + b) & 1)) with e_r from {-2 .. 1}: the blocks of one row alternate
between two scales and 2^-2 .. 2^2 all occur.  With x in {+-1 .. +-4} a row's terms are integers times 2^e_r whose magnitudes
sum to at most 8 * 3 * 4 * 2 = 192: every partial sum in every order is exact in f32 and the total has at most 8 significant
bits - a bf16 number.  Both are asserted here."""
import numpy as np
import torch

import dense_ref as dr

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
BLOCK = 32
S_MIN, S_MAX = -100, 100
MX_P = 8              # nonzeros of a plain row: |units| <= 8 * 3 * 4 * 2 = 192, + bias 32 in quarter units still one rounding
MX_PAIR_P = 4         # as dense_ref.PAIR_P


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def nibbles(w4):
    """uint8 [N, K / 2] -> int64 [N, K]: element order = low nibble, then high nibble, of each byte"""
    b = _np(w4).astype(np.int64)
    return np.stack((b & 0xF, b >> 4), axis=-1).reshape(b.shape[0], -1)


def decode(w4, w_scale):
    """f64 [N, K]"""
    nib = nibbles(w4)
    val = np.where(nib & 8, -E2M1[nib & 7], E2M1[nib & 7])
    e = _np(w_scale).astype(np.int64) - 127
    return val * np.repeat(np.ldexp(1.0, e), BLOCK, axis=1)


def block_exponent(amax):
    """The smallest integer s with amax / 2^s <= 6, by search from a log2 estimate (f64 [...] -> int64); clamped to
    [S_MIN, S_MAX]; 0 for amax == 0."""
    amax = np.asarray(amax, dtype=np.float64)
    safe = np.where(amax > 0, amax, 1.0)
    s = np.floor(np.log2(safe)).astype(np.int64) - 2
    for _ in range(3):
        s = np.where(safe > 6.0 * np.ldexp(1.0, s), s + 1, s)
    for _ in range(3):
        s = np.where(safe <= 6.0 * np.ldexp(1.0, s - 1), s - 1, s)
    assert np.all(safe <= 6.0 * np.ldexp(1.0, s)) and np.all(safe > 6.0 * np.ldexp(1.0, s - 1))
    return np.where(amax > 0, np.clip(s, S_MIN, S_MAX), 0)


def round_e2m1(a):
    """|value| in units of the block scale (f64, >= 0) -> e2m1 code 0..7: the nearest value, a tie to the code with mantissa bit
    0 (the even code); values above 6 (a clamped scale) take 6."""
    a = np.minimum(np.asarray(a, dtype=np.float64), 6.0)
    d = np.abs(a[..., None] - E2M1)
    best = d.min(axis=-1, keepdims=True)
    tie = d == best
    even = tie & (np.arange(8) % 2 == 0)
    pick = np.where(even.any(axis=-1, keepdims=True), even, tie)
    return pick.argmax(axis=-1)


def quantize(w):
    """f64 / f32 / bf16 [N, K] -> (w4 uint8 [N, K / 2], w_scale uint8 [N, K / 32]) by the rule of the format"""
    w = _np(w.double() if isinstance(w, torch.Tensor) else w).astype(np.float64)
    N, K = w.shape
    blk = w.reshape(N, K // BLOCK, BLOCK)
    s = block_exponent(np.abs(blk).max(axis=-1))
    code = round_e2m1(np.abs(blk) * np.ldexp(1.0, -s)[..., None])
    nib = (code | ((blk < 0).astype(np.int64) << 3)).reshape(N, K // 2, 2)
    return (nib[..., 0] | (nib[..., 1] << 4)).astype(np.uint8), (s + 127).astype(np.uint8)


def gemv64(w4, w_scale, x):
    """sum_k W[n][k] x[k] in f64: (ref [N], magnitude sum_k |W||x| [N])"""
    xv = _np(x.double() if isinstance(x, torch.Tensor) else x).astype(np.float64).reshape(-1)
    w4, w_scale = _np(w4), _np(w_scale)
    ref, mag = np.empty(w4.shape[0]), np.empty(w4.shape[0])
    for r in range(0, w4.shape[0], 512):                   # (row chunks: the f64 matrix of a large bank is never whole in memory)
        w = decode(w4[r:r + 512], w_scale[r:r + 512])
        ref[r:r + 512], mag[r:r + 512] = w @ xv, np.abs(w) @ np.abs(xv)
    return ref, mag


# ------------------------------------------------------------------------------------------------------- exact cases
class MxBank:
    """A dense_ref Bank as MXFP4: w4 / w_scale of all launches stacked (torch uint8, CPU) and the exact outputs."""

    def __init__(self, bank, row_exp):
        self.bank, self.K, self.rows, self.launches = bank, bank.K, bank.rows, bank.launches
        R = bank.cols.shape[0]
        self.row_exp = row_exp.view(R).to(torch.int64)               # e_r
        r = torch.arange(R).view(R, 1)
        self.block_bit = lambda cols: (r + cols // BLOCK) & 1        # the alternation between the blocks of a row
        code = torch.zeros(R, bank.K, dtype=torch.uint8)
        mag = bank.vals.abs()
        c = torch.where(mag == 1, 2, torch.where(mag == 2, 4, 5)) | ((bank.vals < 0).to(torch.int64) << 3)
        code.scatter_(1, bank.cols, c.to(torch.uint8))
        pair = code.view(R, bank.K // 2, 2)
        self.w4 = (pair[..., 0] | (pair[..., 1] << 4)).contiguous()
        b = torch.arange(bank.K // BLOCK).view(1, -1)
        self.w_scale = (127 + self.row_exp.view(R, 1) + ((r + b) & 1)).to(torch.uint8).contiguous()
        assert int(self.w_scale.min()) >= 125 and int(self.w_scale.max()) <= 129
        assert bool((self.w_scale[:, 0] != self.w_scale[:, 1]).all())          # the blocks of one row differ

    def units(self, x):
        """x int64 [K] -> (units int64 [launches, rows], sum of |terms| in units): t = units * 2^e_r"""
        terms = x[self.bank.cols] * self.bank.vals * (1 + self.block_bit(self.bank.cols))
        return terms.sum(-1).view(self.launches, self.rows), terms.abs().sum(-1)

    def expected(self, x):
        """The exact outputs as bf16 [launches, rows], with the two assertions the construction rests on: every partial sum
        is exact in f32 (the magnitudes sum below 2^24 units), the total is a bf16 number; and the f64 decode of the packed
        bytes gives the same numbers."""
        u, mags = self.units(x)
        assert int(mags.max()) < 2 ** 24 and int(u.abs().max()) <= 256
        t = u.double() * torch.ldexp(torch.ones(self.row_exp.shape[0], dtype=torch.float64), self.row_exp).view(u.shape)
        assert torch.equal(t.bfloat16().double(), t)
        ref, _ = gemv64(self.w4, self.w_scale, x)
        assert np.array_equal(ref, t.view(-1).numpy())
        return t.bfloat16()


def row_exponents(n, seed):
    """int64 [n] from {-2 .. 1}"""
    return torch.randint(-2, 2, (n,), generator=torch.Generator().manual_seed(seed))


def plain_mx_bank(N, K, seed):
    bank = dr.plain_bank(N, K, seed, P=MX_P)
    assert bank.covers_every_column()
    return MxBank(bank, row_exponents(bank.cols.shape[0], seed + 1))


def pair_mx_bank(I, K, seed, colsign, x):
    """[gate; up] rows whose products share a sign (dense_ref.pair_bank).  A gate row's e_r is the largest of its draw that
    keeps |g| <= 48 and is raised where needed to |g| >= 4 - the range dense_ref states its SiLU bound for; |units| is in
    [4, 96], so e_r in {-1, 0} always satisfies both and every row keeps a scale from the set."""
    bank = dr.pair_bank(I, K, seed, colsign, P=MX_PAIR_P)
    R = bank.cols.shape[0]
    e = row_exponents(R, seed + 1)
    probe = MxBank(bank, e)
    u = probe.units(x)[0].abs().view(-1).double()
    assert bool((u >= 4).all()) and bool((u <= 96).all())
    hi = torch.floor(torch.log2(48.0 / u)).to(torch.int64)          # largest e with u 2^e <= 48
    lo = torch.ceil(torch.log2(4.0 / u)).to(torch.int64)            # smallest e with u 2^e >= 4
    gate = (torch.arange(R) % (2 * I)) < I
    e = torch.where(gate, torch.maximum(torch.minimum(e, hi), lo), e)
    mx = MxBank(bank, e)
    g = (mx.units(x)[0].double() * torch.ldexp(torch.ones(R, dtype=torch.float64), e).view(mx.launches, 2 * I))[:, :I].abs()
    assert bool((g >= 4).all()) and bool((g <= 48).all()) and int(e.min()) >= -2 and int(e.max()) <= 1
    return mx


def decode_probe_rows(lanes=(0, 1, 63), K=2048):
    """The single-element rows that pin the decode: (w4 [R, K / 2], w_scale [R, K / 32], col int64 [R], value f64 [R]).
    Part 1: all 16 nibble codes x both nibbles x all 16 byte positions of a lane's 16-byte load x `lanes`, the element's block
    at scale byte 128 (2.0) and every other block of the row at 125 (a scale taken from another block shows).
    Part 2: every code at scale bytes {27, 126, 127, 128, 227}.  Part 3: code 6 (4.0) at every scale byte 27 .. 227."""
    rows = [(32 * lane + 2 * byte + nib, code, 128) for code in range(16) for nib in range(2) for byte in range(16) for lane in lanes]
    rows += [(32 * 5 + 7, code, sb) for code in range(16) for sb in (27, 126, 127, 128, 227)]
    rows += [(32 * 40 + 18, 6, sb) for sb in range(27, 228)]
    R = len(rows)
    w4 = torch.zeros(R, K // 2, dtype=torch.uint8)
    sc = torch.full((R, K // BLOCK), 125, dtype=torch.uint8)
    col = torch.tensor([r[0] for r in rows])
    val = np.zeros(R)
    for i, (k, code, sb) in enumerate(rows):
        w4[i, k // 2] = code << (4 * (k & 1))
        sc[i, k // BLOCK] = sb
        val[i] = (-1.0 if code & 8 else 1.0) * E2M1[code & 7] * 2.0 ** (sb - 127)
    assert np.array_equal(decode(w4, sc)[np.arange(R), col.numpy()], val)
    return w4, sc, col, torch.from_numpy(val)
