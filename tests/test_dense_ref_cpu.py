"""CPU: tests/dense_ref.py (the references test_gpu_dense_exact.py pins the dense decode kernels to) against independent
evaluations, and the conditions its structured inputs must meet at every shape the GPU file uses."""
import math

import pytest
import torch

import dense_ref as dr
import util

# every (rows per launch, K, nonzeros per row) the GPU file builds a bank for
GEMV_PLAIN = [(N, K) for N in (1, 7, 8, 9, 4101) for K in (512, 520, 1024, 4104, 13696)] + \
             [(N, K) for N in (8193, 8209) for K in (512, 1000)]
GEMV_SILU = [(I, K) for I in (1, 7, 9, 1003, 3425) for K in (512, 520, 13696)]
NORM_PLAIN = [(N, 4096) for N in (1, 15, 17, 4101, 8193)]
NORM_SILU = [(I, 4096) for I in (1, 9, 1003)]
NORM_RMAX = [(N, 4096) for N in (16, 48, 32000)]
QKV = [((Hq + 2 * Hkv) * 128, K) for Hq, Hkv in ((32, 8), (4, 1), (32, 4), (2, 1)) for K in (520, 4096)]
ROWS_K = (32, 96, 288, 1056, 8224)
ROWS_PLAIN = [(N, K) for N in (48, 6160, 16400) for K in ROWS_K]
ROWS_SILU = [(1003, K) for K in ROWS_K]


@pytest.mark.parametrize("N,K", GEMV_PLAIN + NORM_PLAIN + NORM_RMAX + QKV + ROWS_PLAIN)
def test_plain_bank_conditions(N, K):
    b = dr.plain_bank(N, K, seed=N + K)
    assert b.rows == N and b.cols.shape == (b.launches * N, dr.PLAIN_P)
    assert b.covers_every_column()
    assert bool((b.vals != 0).all()) and int(b.vals.abs().max()) <= 3
    srt = b.cols.sort(-1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())                        # P distinct columns in every row
    lap = b.cols[:K // dr.PLAIN_P].flatten()                               # the rows of one lap: disjoint column sets
    assert lap.unique().numel() == lap.numel()
    head = srt[:4000].tolist()                                             # and never the same set twice in a row
    assert all(a != b for a, b in zip(head, head[1:]))
    x, _ = dr.structured_x(2, K, seed=K)
    assert int(x.abs().min()) >= 1 and int(x.abs().max()) <= 4
    s = b.sums(x) + dr.integer_bias(N, seed=1)
    assert int(s.abs().max()) <= 224


@pytest.mark.parametrize("I,K", GEMV_SILU + NORM_SILU + ROWS_SILU)
def test_pair_bank_conditions(I, K):
    x, colsign = dr.structured_x(3, K, seed=K + 1)
    b = dr.pair_bank(I, K, seed=I + K, colsign=colsign)
    assert b.rows == 2 * I and b.covers_every_column()
    assert bool((b.vals != 0).all()) and int(b.vals.abs().max()) <= 3
    g, u, ref = dr.pair_ref(b, x)
    assert bool((g != 0).all()) and bool((u != 0).all())
    assert int(g.abs().max()) <= 48 and int(u.abs().max()) <= 48
    assert bool((g > 0).any()) and bool((g < 0).any()) and bool((ref != 0).all())
    prod = x[:, b.cols] * b.vals                                           # the products of a row share a sign
    assert bool(((prod > 0).all(-1) | (prod < 0).all(-1)).all())


@pytest.mark.parametrize("N,K,P", [(9, 520, 16), (1000, 13696, 16), (4101, 512, 16), (48, 96, 16), (2 * 7, 520, 4)])
def test_integer_sums_against_int64_matmul(N, K, P):
    x, colsign = dr.structured_x(5, K, seed=3)
    b = dr.plain_bank(N, K, seed=7) if P == 16 else dr.pair_bank(N // 2, K, seed=7, colsign=colsign)
    w = b.dense()
    assert w.shape == (b.launches * N, K) and w.dtype == torch.bfloat16
    assert bool(((w != 0).sum(-1) == P).all())
    assert bool((w != 0).any(0).all())                                     # coverage, from the weight tensor itself
    want = (x @ w.to(torch.int64).t()).view(5, b.launches, N)
    assert torch.equal(b.sums(x), want)
    bias = dr.integer_bias(N, seed=2)
    assert torch.equal(dr.gemv_ref(b, x, bias).to(torch.int64), want + bias)
    # the premise of the construction: any order of f32 accumulation gives the integer, and bf16 holds it
    f32 = (x.float() @ w.float().t()).view(5, b.launches, N)
    assert torch.equal(f32.bfloat16().to(torch.int64), want)


@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("eps", [0.0, 1e-5])
def test_norm_inputs_make_the_norm_exact(residual, eps):
    n = dr.norm_inputs(4096, seed=5, residual=residual)
    x = dr.to_bf16(n["x"])
    res = dr.to_bf16(n["residual"]) if residual else None
    h = dr.add_ref(x, res)
    assert torch.equal(h.to(torch.int64), n["h"]) and bool((n["h"].abs() == 2).all())
    assert set(n["w_norm"].tolist()) == {1, 2, 3, 4}
    y64 = dr.rmsnorm_ref(h, dr.to_bf16(n["w_norm"]), eps)
    assert torch.equal(dr.round_bf16(y64).to(torch.int64), n["xn"])
    # and in f32, the way the kernels form it: h * rstd * w, each product rounded to f32
    rstd = 1.0 / torch.sqrt(h.float().pow(2).mean() + eps)
    assert torch.equal((h.float() * rstd * n["w_norm"].float()).bfloat16().to(torch.int64), n["xn"])
    assert int(n["xn"].abs().min()) >= 1 and int(n["xn"].abs().max()) <= 4


@pytest.mark.parametrize("hidden", [8, 520, 4096, 8192])
def test_rmsnorm_against_torch_f64(hidden):
    g = torch.Generator().manual_seed(hidden)
    h = torch.randn(3, hidden, generator=g).bfloat16()
    w = (1 + 0.1 * torch.randn(hidden, generator=g)).bfloat16()
    want = torch.nn.functional.rms_norm(h.double(), (hidden,), w.double(), 1e-5)
    assert torch.allclose(dr.rmsnorm_ref(h, w, 1e-5), want, rtol=1e-13, atol=0)


def test_add_ref_is_one_bf16_add():
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(4096, generator=g).bfloat16(), torch.randn(4096, generator=g).bfloat16()
    assert torch.equal(dr.bits(dr.add_ref(a, b)), dr.bits(a + b))
    assert dr.add_ref(a, None) is a


def test_round_bf16_is_round_to_nearest_even():
    g = torch.Generator().manual_seed(2)
    v = torch.randn(100000, generator=g) * torch.tensor(2.0) ** torch.randint(-60, 60, (100000,), generator=g)
    assert torch.equal(dr.round_bf16(v.double()), v.bfloat16().double())    # f32 -> bf16 is one rounding either way
    # ties: 1 + 2^-8 lies between 1 and 1 + 2^-7 -> even (1); 1 + 3 * 2^-8 -> 1 + 2^-6; just above a tie -> up (a detour
    # through f32 would round this one down first)
    t = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40, -(1 + 2.0 ** -8 + 2.0 ** -40)], dtype=torch.float64)
    assert dr.round_bf16(t).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -(1 + 2.0 ** -7)]
    assert dr.round_bf16(torch.tensor([2.0 ** -131, 0.0], dtype=torch.float64)).tolist() == [2.0 ** -131, 0.0]


def test_silu_reference():
    g = torch.tensor([0.0, 1.0, -1.0, 48.0, -48.0, 60.0, -60.0, 0.5], dtype=torch.float64)
    want = [0.0] + [float(v) / (1.0 + math.exp(-float(v))) for v in g[1:]]
    assert torch.allclose(dr.silu64(g), torch.tensor(want, dtype=torch.float64), rtol=1e-14, atol=0)
    u = torch.tensor([3.0, -7.0, 48.0, 1.0, 2.0, -1.0, 5.0, 0.25], dtype=torch.float64)
    ref = dr.silu_mul_ref(g.bfloat16(), u.bfloat16())
    assert torch.equal(ref, ref.bfloat16().double())                       # a bf16 value
    assert bool(((ref - dr.silu64(g) * u).abs() <= dr.SILU_RTOL * ref.abs()).all())
    assert float(ref[3]) == 48.0 and float(ref[0]) == 0.0 and float(ref[4]) < 0.0


def _cos_sin(rows, width, seed):
    return (torch.rand(rows, width, generator=torch.Generator().manual_seed(seed)) * 2 - 1).bfloat16()


def test_neox_restatement_against_the_torch_rotation():
    from shadowkv_amd import tensor_op
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 6, 1, 128, generator=g).bfloat16()
    cs = _cos_sin(50, 128, 4)
    pos = torch.tensor([[7], [49]])
    cos, sin = cs[:, :64].double().repeat(1, 2), cs[:, 64:].double().repeat(1, 2)
    want = tensor_op.apply_rotary_pos_emb_single(x.double(), cos, sin, pos)
    true = dr.rope_true(x.float(), cs.float()[pos.view(2)].view(2, 1, 1, 128), glm=False)
    assert torch.allclose(true, want, rtol=1e-14, atol=1e-300)
    got = dr.rope_restate(x.float(), cs.float()[pos.view(2)].view(2, 1, 1, 128), glm=False)
    assert got.dtype == torch.bfloat16
    assert bool(((got.double() - want).abs() <= util.rope_pair_bound(x, glm=False)).all())
    assert float((got.double() - want).abs().max()) > 0                    # (a restatement that rounds, not the f64 rotation)


def test_glm_restatement_against_a_per_pair_rotation():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 128, generator=g).bfloat16()
    cs = _cos_sin(3, 64, 6)
    want = x.double().clone()
    for r in range(3):
        for t in range(32):
            c, s = float(cs[r, t]), float(cs[r, 32 + t])
            a, b = float(x[r, 2 * t]), float(x[r, 2 * t + 1])
            want[r, 2 * t], want[r, 2 * t + 1] = a * c - b * s, b * c + a * s
    assert torch.allclose(dr.rope_true(x.float(), cs.float(), glm=True), want, rtol=1e-14, atol=1e-300)
    got = dr.rope_restate(x.float(), cs.float(), glm=True)
    assert bool(((got.double() - want).abs() <= util.rope_pair_bound(x, glm=True)).all())
    assert torch.equal(dr.bits(got[:, 64:]), dr.bits(x[:, 64:]))           # pass-through dims keep their bits


@pytest.mark.parametrize("glm", [False, True])
def test_qkv_split_rope_cache_reference(glm):
    Hq, Hkv, rows = 4, 2, 6
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(3, (Hq + 2 * Hkv) * 128, generator=g).bfloat16()
    cs = _cos_sin(10, 64 if glm else 128, 8)
    q, k, v = dr.qkv_rope_cache_ref(qkv, cs, [2, -5, 99], 4, Hq, Hkv, rows)
    heads = qkv.view(3, Hq + 2 * Hkv, 128)
    for b, p in enumerate((2, 0, 9)):                                      # positions clamp to the table's first / last row
        for hd in range(Hq + Hkv):
            want = dr.rope_restate(heads[b, hd].float(), cs[p].float(), glm)
            got = q[b, hd] if hd < Hq else k[b, hd - Hq, 4]
            assert torch.equal(dr.bits(got), dr.bits(want))
    assert torch.equal(dr.bits(v[:, :, 4]), dr.bits(heads[:, Hq + Hkv:]))
    keep = [r for r in range(rows) if r != 4]
    assert bool(torch.isnan(k[:, :, keep].float()).all()) and bool(torch.isnan(v[:, :, keep].float()).all())
    ov = torch.randn(3, Hq, 128, generator=g).bfloat16()
    for row in (-1, rows):                                                 # push dropped, q still there; override replaces q
        q2, k2, v2 = dr.qkv_rope_cache_ref(qkv, cs, [2, -5, 99], row, Hq, Hkv, rows, q_override=ov)
        assert bool(torch.isnan(k2.float()).all()) and bool(torch.isnan(v2.float()).all())
        assert torch.equal(dr.bits(q2), dr.bits(ov))


def test_order_keys_against_sorting():
    allb = torch.arange(0x10000, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    vals = allb[~torch.isnan(allb.float())]
    keys = dr.order_keys(vals)
    assert keys.unique().numel() == vals.numel() and int(keys.min()) >= 0 and int(keys.max()) <= 0xFFFF
    by_key = vals.float()[keys.argsort()]
    assert bool((by_key[1:] >= by_key[:-1]).all())                         # ascending keys = ascending values (-0 before +0)
    g = torch.Generator().manual_seed(9)
    y = (torch.randn(64 * 16, generator=g) * 5).bfloat16()
    rm = dr.range_max_ref(y)
    top = y.float().view(64, 16).max(-1).values
    assert torch.equal(rm, dr.order_keys(top.bfloat16()))


def test_flip_share_constants():
    """The shares test_gpu_dense_exact.py allows are 4 x what two plain f32 evaluations (sequential, pairwise) show against
    bf16(f64) on the same data; recomputed here for the rows-GEMM shape (the GEMV pair is in the record,
    profiles/dense_exact_flip_shares.txt)."""
    import test_gpu_dense_exact as gpu
    w, x, bias, s64 = dr.random_case(**dr.RANDOM_ROWS)
    seq, pw = dr.flip_share(dr.f32_sequential(w, x), s64, bias), dr.flip_share(dr.f32_pairwise(w, x), s64, bias)
    assert gpu.ROWS_CPU_SHARES == pytest.approx((seq, pw), rel=1e-6)
    assert gpu.ROWS_SHARE_BOUND == 4 * max(gpu.ROWS_CPU_SHARES) and gpu.GEMV_SHARE_BOUND == 4 * max(gpu.GEMV_CPU_SHARES)
