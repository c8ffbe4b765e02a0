"""CPU references for the dense half of a decode layer (skv_gemv.hip, skv_rows_gemm.hip, skv_dense.hip, the epilogue of
skv_kvproj.h, the sampler's range keys) and the structured inputs that make those references EXACT.

The construction: weights with a few small-integer nonzeros per row, x dense in {+-1 .. +-4}, integer bias.  Every partial sum
is an integer far below 2^24 and the total has at most 8 significant bits, so every order of f32 accumulation gives the same
sum and the bf16 rounding is the identity: the expected output is an integer computed in int64, and the comparison is on raw
bits.  A dropped, doubled or misplaced k element changes the integer.  

No GPU import here: builders take a `device` only to place the dense weight tensor (plain torch ops); every expected value is
computed on the CPU from the sparse (column, value) form.  tests/test_dense_ref_cpu.py checks this module against independent
evaluations."""
import math

import torch

PLAIN_P = 16          # nonzeros of a plain weight row: |sum| <= 16 * 3 * 4 = 192, |sum + bias| <= 224 < 256
PAIR_P = 4            # nonzeros of a gate / up row: |g|, |u| <= 4 * 3 * 4 = 48
BIAS_MAX = 32
SILU_RTOL = 3 * 2.0 ** -9     # one bf16 ulp on the rounded SiLU + half an ulp on the product
NORM_RTOL = 2.0 ** -8         # half an ulp of output rounding + a margin for f32 rsqrt


def bits(t):
    """bf16 tensor -> int32 tensor of the raw 16-bit patterns."""
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _signs(shape, g):
    return torch.randint(0, 2, shape, generator=g, dtype=torch.int64) * 2 - 1


def stride_for(K, seed):
    """A step coprime to K near 0.618 K: j -> j * step mod K is a bijection of the columns, and neighbours in j land far apart."""
    s = (int(K * 0.6180339887) + 2 * seed) | 1
    while math.gcd(s, K) != 1:
        s += 2
    return s % K


# ---------------------------------------------------------------------------------------------------------------- inputs
def structured_x(M, K, seed):
    """(x int64 [M, K], colsign int64 [K]): dense, every element in {+-1 .. +-4}; sign(x[m][k]) = s_m * colsign[k], so a weight
    row can be built whose products share a sign for every token row (the up rows of the SiLU pairs)."""
    g = _gen(seed)
    colsign = _signs((K,), g)
    rowsign = _signs((M, 1), g)
    mag = torch.randint(1, 5, (M, K), generator=g, dtype=torch.int64)
    return rowsign * colsign * mag, colsign


def norm_inputs(K, seed, residual=True):
    """Inputs of the fused residual add + RMSNorm for which the norm is exact: x + residual in {+-2} element-wise, so
    mean(h^2) = 4, rstd = 0.5 (eps = 0) or 0.49999937 (eps = 1e-5) and bf16(h * rstd * w_norm) = sign(h) * w_norm with
    w_norm in {1, 2, 3, 4}.  Returns dict(x, residual (None without), w_norm, h, xn) of int64 tensors [K]."""
    g = _gen(seed)
    h = 2 * _signs((K,), g)
    w = torch.randint(1, 5, (K,), generator=g, dtype=torch.int64)
    res = torch.randint(-6, 7, (K,), generator=g, dtype=torch.int64) if residual else None
    x = h - res if residual else h.clone()
    return dict(x=x, residual=res, w_norm=w, h=h, xn=(h // 2) * w)


def integer_bias(N, seed):
    return torch.randint(-BIAS_MAX, BIAS_MAX + 1, (N,), generator=_gen(seed), dtype=torch.int64)


class Bank:
    """`launches` weight matrices of `rows` rows each, stacked: row r holds vals[r][p] at column cols[r][p] (P distinct columns),
    0 elsewhere.  Columns follow one stride walk over all rows of the bank (the rows of its first lap alone visit every column),
    so as soon as rows * launches * P >= K every column is nonzero in some row; shapes with few rows per launch get more
    launches, never denser rows."""

    def __init__(self, cols, vals, K, rows, launches):
        self.cols, self.vals, self.K, self.rows, self.launches = cols, vals, K, rows, launches

    def dense(self, device="cpu"):
        """bf16 [launches * rows, K]"""
        w = torch.zeros(self.cols.shape[0], self.K, dtype=torch.bfloat16, device=device)
        w.scatter_(1, self.cols.to(device), self.vals.to(torch.bfloat16).to(device))
        return w

    def covers_every_column(self):
        return bool((torch.bincount(self.cols.flatten(), minlength=self.K) > 0).all())

    def sums(self, x):
        """Exact W . x: x int64 [M, K] -> int64 [M, launches, rows]"""
        s = (x[:, self.cols] * self.vals).sum(-1)
        return s.view(x.shape[0], self.launches, self.rows)


def _walk(R, P, K, seed):
    assert P <= K
    j = torch.arange(R * P, dtype=torch.int64).view(R, P)
    lap = j[:, :1] // K                      # rows of a later lap over the columns are shifted: another set, not a repeat
    return (j * stride_for(K, seed) + 3 * seed + lap) % K


def plain_bank(N, K, seed, P=PLAIN_P):
    """Rows with exactly P nonzeros from {+-1, +-2, +-3}, N rows per launch."""
    L = max(1, -(-K // (N * P)))
    g = _gen(seed)
    cols = _walk(L * N, P, K, seed)
    vals = torch.randint(1, 4, cols.shape, generator=g, dtype=torch.int64) * _signs(cols.shape, g)
    return Bank(cols, vals, K, N, L)


def pair_bank(I, K, seed, colsign, P=PAIR_P):
    """[gate; up] matrices, 2 I rows per launch, P nonzeros per row.  Every row's weights carry t_row * colsign[column], so
    with x from structured_x / norm_inputs (sign(x[k]) = +-colsign[k]) the P products of a row share a sign: g and u are
    never 0 and 4 <= |g|, |u| <= 48, both signs occurring."""
    L = max(1, -(-K // (2 * I * P)))
    g = _gen(seed)
    cols = _walk(L * 2 * I, P, K, seed)
    t = _signs((cols.shape[0], 1), g)
    vals = torch.randint(1, 4, cols.shape, generator=g, dtype=torch.int64) * t * colsign[cols]
    return Bank(cols, vals, K, 2 * I, L)


def to_bf16(v):
    """int64 -> bf16, refusing values the format would round"""
    assert int(v.abs().max()) <= 256
    return v.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------ references
def gemv_ref(bank, x, bias=None):
    """Expected bf16 outputs [M, launches, rows] of y = W . x (+ bias): exact integers."""
    s = bank.sums(x)
    if bias is not None:
        s = s + bias
    return to_bf16(s)


def round_bf16(v):
    """f64 -> nearest bf16 value (ties to even) as f64, in ONE rounding (a detour through f32 rounds twice).  Values below the
    smallest normal take the f32 detour: the tests put only values there whose f32 image is exact."""
    b = v.contiguous().view(torch.int64)
    r = (b + ((1 << 44) - 1) + ((b >> 45) & 1)) & ~((1 << 45) - 1)
    out = r.view(torch.float64)
    return torch.where(v.abs() < 2.0 ** -126, v.float().bfloat16().double(), out)


def silu64(g):
    g = g.double()
    return g / (1.0 + torch.exp(-g))


def silu_mul_ref(g, u):
    """bf16(bf16(silu(g)) * u) as f64, for bf16-representable g and u (their product with an 8-bit factor is exact in f64)."""
    return round_bf16(round_bf16(silu64(g)) * u.double())


def pair_ref(bank, x):
    """(g, u, ref): the exact gate and up sums int64 [M, launches, I] and the expected SiLU * mul output (f64)."""
    s = bank.sums(x)
    I = bank.rows // 2
    g, u = s[..., :I], s[..., I:]
    return g, u, silu_mul_ref(g, u)


def add_ref(x, residual):
    """h = x + residual as the kernels form it: one f32 add of two bf16 values, one rounding to bf16."""
    return x if residual is None else (x.float() + residual.float()).bfloat16()


def rmsnorm_ref(h, w, eps):
    """f64 RMSNorm of bf16 rows h [..., hidden] with weight w [hidden]; not rounded."""
    h = h.double()
    return h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps) * w.double()


def _r(t):
    return t.bfloat16().float()


def rope_restate(x, cs, glm):
    """The rotation as the kernels state it - bf16 arithmetic, one rounding per operation, like the RoPE kernels of
    skv_rope.hip - in f32 torch ops.  The product of two bf16 values is exact in f32 and the f32 add is IEEE on both sides,
    so this predicts the kernel's bits.  x f32 [..., 128] (bf16 values); cs f32 [..., 128] = [cos(64) | sin(64)] (NeoX, pairs
    (t, t + 64)) or [..., 64] = [cos(32) | sin(32)] (GLM, pairs (2t, 2t + 1), dims 64..127 pass through).  Returns bf16."""
    if not glm:
        x1, x2, c, s = x[..., :64], x[..., 64:], cs[..., :64], cs[..., 64:]
        o1 = _r(_r(x1 * c) + _r(-x2 * s))
        o2 = _r(_r(x2 * c) + _r(x1 * s))
        return torch.cat((o1, o2), -1).bfloat16()
    x1, x2, c, s = x[..., 0:64:2], x[..., 1:64:2], cs[..., :32], cs[..., 32:]
    o1 = _r(_r(x1 * c) + _r(-x2 * s))
    o2 = _r(_r(x2 * c) + _r(x1 * s))
    return torch.cat((torch.stack((o1, o2), -1).flatten(-2), x[..., 64:]), -1).bfloat16()


def rope_true(x, cs, glm):
    """The rotation itself in f64, unrounded (the guard on rope_restate)."""
    x, cs = x.double(), cs.double()
    if not glm:
        x1, x2, c, s = x[..., :64], x[..., 64:], cs[..., :64], cs[..., 64:]
        return torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), -1)
    x1, x2, c, s = x[..., 0:64:2], x[..., 1:64:2], cs[..., :32], cs[..., 32:]
    return torch.cat((torch.stack((x1 * c - x2 * s, x2 * c + x1 * s), -1).flatten(-2), x[..., 64:]), -1)


def qkv_rope_cache_ref(qkv, cos_sin, pos, row, Hq, Hkv, cache_rows, q_override=None, sentinel=float("nan")):
    """Split + RoPE + cache push of skv_qkv_rope_update and of the QKV epilogue.  qkv bf16 [bs, (Hq + 2 Hkv) * 128];
    cos_sin bf16 [rows, 128 | 64] (the width selects NeoX | GLM); pos int [bs], clamped to the table; row: the cache row, the
    push is dropped when it lies outside [0, cache_rows); q_override bf16 [bs, Hq, 128] replaces q's bits.
    Returns (q [bs, Hq, 128], k_cache, v_cache [bs, Hkv, cache_rows, 128]) bf16, the caches `sentinel` outside the pushed row."""
    bs = qkv.shape[0]
    glm = cos_sin.shape[-1] == 64
    x = qkv.float().view(bs, Hq + 2 * Hkv, 128)
    p = torch.as_tensor(pos).view(bs).clamp(0, cos_sin.shape[0] - 1)
    rot = rope_restate(x[:, :Hq + Hkv], cos_sin.float()[p].unsqueeze(1), glm)
    q = rot[:, :Hq] if q_override is None else q_override.view(bs, Hq, 128).clone()
    k = torch.full((bs, Hkv, cache_rows, 128), sentinel).bfloat16()
    v = k.clone()
    if 0 <= int(row) < cache_rows:
        k[:, :, int(row)] = rot[:, Hq:]
        v[:, :, int(row)] = x[:, Hq + Hkv:].bfloat16()
    return q.contiguous(), k, v


def order_keys(t):
    """The sampler's order-preserving 16-bit key of bf16 values (x >= 0: bits | 0x8000; x < 0: ~bits), as int32."""
    b = bits(t)
    return torch.where((b & 0x8000) != 0, (~b) & 0xFFFF, b | 0x8000)


def range_max_ref(y):
    """Keys the lm_head launch leaves: the largest order key of every 16 consecutive outputs.  y bf16 [N], N % 16 == 0."""
    return order_keys(y.reshape(-1)).view(-1, 16).max(-1).values


# ------------------------------------------------------------------------------------------------------------ rows GEMM
def expected_branch(M, N, K):
    """The kernel skv_rows_pick (skv_rows_frame.h) launches for bf16 and for FP8 weights alike, from the thresholds its table
    documents: up to 8 token rows the first generation with the paired token operand; up to 16 the first generation, 2x8
    where 6144 <= N < 16384; from 17 on two token tiles: 4x4 for N >= 16384, 2x8 in the middle range, 1x8 for K >= 8192, else
    the first generation."""
    mid = 6144 <= N < 16384
    if M <= 8:
        return "g1 paired"
    if M <= 16:
        return "g2 1/2x8" if mid else "g1"
    if N >= 16384:
        return "g2 2/4x4"
    if mid:
        return "g2 2/2x8"
    return "g2 2/1x8" if K >= 8192 else "g1 two tiles"


# ------------------------------------------------------------------------------------ random-data companion (flip shares)
RANDOM_GEMV = dict(N=4101, K=13696, M=1, seed=4101 + 13696)
RANDOM_ROWS = dict(N=6160, K=1056, M=17, seed=17 + 6160 + 1056)


def random_case(N, K, M, seed):
    """Realistic magnitudes: weights N(0, 0.05^2), x N(0, 1), bias N(0, 0.1^2), all bf16, generated on the CPU.
    Returns (w, x, bias, ref64) with ref64 = bf16(W . x in f64) + bias in f64 [M, N] - the kernels round the sum to bf16 before
    the bias add - and the expected output is bf16(ref64)."""
    g = _gen(seed)
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    x = torch.randn(M, K, generator=g).bfloat16()
    bias = (torch.randn(N, generator=g) * 0.1).bfloat16()
    return w, x, bias, x.double() @ w.double().t()


def finish64(sum64, bias):
    """bf16(bf16(sum) + bias) from an f64 sum, as f64"""
    return round_bf16(round_bf16(sum64) + bias.double())


def f32_sequential(w, x):
    """W . x with one f32 accumulator per output, k ascending (products of bf16 values are exact in f32)."""
    wf, xf = w.float().t().contiguous(), x.float()
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k in range(w.shape[1]):
        acc += xf[:, k:k + 1] * wf[k]
    return acc


def f32_pairwise(w, x):
    """W . x as a balanced f32 tree over k (zero-padded to a power of two)."""
    K = w.shape[1]
    out = []
    for m in range(x.shape[0]):
        p = torch.zeros(w.shape[0], 1 << (K - 1).bit_length())
        p[:, :K] = w.float() * x[m].float()
        while p.shape[1] > 1:
            p = p[:, 0::2] + p[:, 1::2]
        out.append(p[:, 0])
    return torch.stack(out)


def flip_share(sum32, sum64, bias):
    """Share of outputs whose bf16 result differs from the f64 evaluation's."""
    got = finish64(sum32.double(), bias)
    return float((got != finish64(sum64, bias)).double().mean())
