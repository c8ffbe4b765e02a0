"""GPU: the weight-only FP8 GEMV kernels (skv_gemv_fp8.hip) against tests/dense_ref.py, bit for bit.

The banks' weights {+-1, +-2, +-3} are exact in e4m3 and the per-row scales are powers of two from 2^-2 .. 2^2: the expected
output is scale * (an integer computed in int64), at most 8 significant bits, so every order of f32 accumulation gives it and
bf16 holds it - raw bits are compared.  SiLU carries dense_ref.SILU_RTOL; the Gaussian case a bound derived from the formats."""
import pytest
import torch

import dense_ref as dr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 1000.0
PAD = 8


def _L():
    from shadowkv_amd import _lib
    return _lib, _lib.lib(), _lib.current_stream_handle()


def sentinel_buf(*shape):
    return torch.full(shape, SENT, dtype=torch.bfloat16, device=DEV)


def dev16(v):
    return dr.to_bf16(v).to(DEV)


def assert_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    a, b = (torch.where(torch.isnan(t.float()), 0x7FC0, dr.bits(t)) for t in (got, want))
    bad = (a != b).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {a.numel()} bf16 values differ, first at {bad[0].tolist()}: " \
                             f"got {float(got.float()[tuple(bad[0])])}, want {float(want.float()[tuple(bad[0])])}"


def assert_silu(got, ref, what):
    err, tol = (got.cpu().double() - ref).abs(), dr.SILU_RTOL * ref.abs()
    worst = float((err / tol.clamp_min(1e-300)).max()) if bool((tol > 0).any()) else 0.0
    print(f"{what}: values {err.numel()}  differing {int((err > 0).sum())}  worst |err| / bound {worst:.3f}")
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} of {err.numel()} values over 3 * 2^-9 |ref|, worst x{worst:.2f}"


def pow2_scales(n, seed):
    """f32 [n] from {2^-2 .. 2^2}"""
    e = torch.randint(-2, 3, (n,), generator=torch.Generator().manual_seed(seed))
    return torch.ldexp(torch.ones(n), e)


def pair_scales(sums, I, seed):
    """Scales of [gate; up] rows (sums int64 [launches, 2 I]): drawn like pow2_scales; a gate row then keeps the largest power
    of two <= its draw with |scale * g| <= 48 - the range dense_ref states its SiLU bound for (4 <= |g| <= 48: the fast f32 exp
    of the epilogue neither overflows nor leaves the normal range there).  |g| >= 4, so every scale of the set still occurs."""
    L = sums.shape[0]
    sc = pow2_scales(L * 2 * I, seed).view(L, 2 * I).clone()
    g = sums[:, :I].abs().double()
    cap = torch.exp2(torch.floor(torch.log2(48.0 / g)))
    sc[:, :I] = torch.minimum(sc[:, :I].double(), cap).float()
    assert bool((sc[:, :I].double() * g <= 48).all())
    return sc.view(-1)


def fp8_weights(bank):
    assert bank.covers_every_column()
    w = bank.dense(DEV)
    w8 = w.to(torch.float8_e4m3fn)
    assert torch.equal(w8.to(torch.bfloat16), w)                   # {+-1, +-2, +-3} are e4m3 numbers
    return w8


def scaled(v_int, scale):
    """int64 [..., rows] * power-of-two scale [rows] -> bf16, exact (<= 8 significant bits)"""
    assert int(v_int.abs().max()) <= 256
    out = v_int.double() * scale.double()
    assert torch.equal(out.bfloat16().double(), out)
    return out.bfloat16()


def run(bank, w8, scale_d, x, bias, silu, norm=None, eps=0.0, rmax=False):
    """One launch per matrix of the bank: (y [launches, No + PAD], h | None, keys | None)"""
    _lib, L, st = _L()
    p = _lib.ptr
    N, K = bank.rows, bank.K
    No = N // 2 if silu else N
    y = sentinel_buf(bank.launches, No + PAD)
    h = sentinel_buf(K + PAD) if norm is not None and norm["residual"] is not None else None
    keys = torch.full((bank.launches, (N // 16 + 7) // 8 * 8 + PAD), -1, dtype=torch.int16, device=DEV) if rmax else None
    for l in range(bank.launches):
        wl, sl = w8[l * N:(l + 1) * N], scale_d[l * N:(l + 1) * N]
        if norm is None:
            rc = L.skv_gemv_fp8(p(wl), p(sl), p(x), p(bias), p(y[l]), N, K, int(silu), st)
        elif rmax:
            rc = L.skv_norm_gemv_rangemax_fp8(p(wl), p(sl), p(x), p(norm["res_d"]), p(norm["w_d"]), eps, p(h), p(bias), p(y[l]), N, K,
                                              p(keys[l]), st)
        else:
            rc = L.skv_norm_gemv_fp8(p(wl), p(sl), p(x), p(norm["res_d"]), p(norm["w_d"]), eps, p(h), p(bias), p(y[l]), N, K,
                                     int(silu), st)
        assert rc == 0, rc
    torch.cuda.synchronize()
    return y, h, keys


def norm_on_device(K, seed, residual):
    n = dr.norm_inputs(K, seed, residual)
    n["x_d"], n["w_d"] = dev16(n["x"]), dev16(n["w_norm"])
    n["res_d"] = dev16(n["residual"]) if residual else None
    return n


def add_rmsnorm_h(n):
    """h as skv_add_rmsnorm writes it for the same inputs"""
    from shadowkv_amd import tensor_op
    h, _ = tensor_op.add_rmsnorm(n["x_d"].view(1, -1), n["res_d"].view(1, -1), n["w_d"], 1e-5)
    return h.view(-1)


# K: one step; a tail of one lane; four steps; 13 steps + a 24-lane tail (GLM-4's intermediate size)
KS = (1024, 1040, 4096, 13696)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", [20, 4096, 8208])
def test_fp8_gemv_plain_and_bias_exact(N, K):
    """skv_gemv_fp8: R = 2 (N <= 8192; 20: a ragged last workgroup with clamped rows) and R = 4 (8208)."""
    bank = dr.plain_bank(N, K, seed=N + K)
    w8 = fp8_weights(bank)
    scale = pow2_scales(bank.launches * N, seed=N + K + 1)
    xi, _ = dr.structured_x(1, K, seed=K)
    sums = bank.sums(xi)[0]                                        # [launches, N]
    sv = scale.view(bank.launches, N)
    for bias in (None, dr.integer_bias(N, seed=N)):
        y, _, _ = run(bank, w8, scale.to(DEV), dev16(xi), None if bias is None else dev16(bias), silu=False)
        t = scaled(sums, sv)
        # bias: bf16(bf16r(t) + bias) - t is a bf16 number, t + bias has <= 8 + 7 bits above 2^-2: exact in f32, rounded once
        want = t if bias is None else (t.float() + bias.float()).bfloat16()
        assert_bits(y[:, :N], want, f"fp8 gemv N {N} K {K} bias {bias is not None}")
        assert bool((y[:, N:] == SENT).all()), "written past N"


@pytest.mark.parametrize("K", KS)
def test_fp8_gemv_silu_pair(K):
    I = 10
    xi, colsign = dr.structured_x(1, K, seed=K + 1)
    bank = dr.pair_bank(I, K, seed=I + K, colsign=colsign)
    w8 = fp8_weights(bank)
    s = bank.sums(xi)[0]                                           # [launches, 2 I]
    scale = pair_scales(s, I, seed=K + 2)
    t = scaled(s, scale.view(bank.launches, 2 * I))
    g, u = t[:, :I], t[:, I:]
    assert bool((g != 0).all()) and bool((u != 0).all())
    y, _, _ = run(bank, w8, scale.to(DEV), dev16(xi), None, silu=True)
    assert_silu(y[:, :I], dr.silu_mul_ref(g, u), f"fp8 gemv silu K {K}")
    assert bool((y[:, I:] == SENT).all()), "written past I"


@pytest.mark.parametrize("residual", [True, False])
def test_fp8_norm_gemv_exact(residual):
    """Norm prologue + plain / bias GEMV (N = 20, 4101: ragged) and + SiLU pair: outputs and h bit-equal to the references, h
    also bit-equal to skv_add_rmsnorm's."""
    K = 4096
    n = norm_on_device(K, seed=3 + residual, residual=residual)
    for N in (20, 4101):
        bank = dr.plain_bank(N, K, seed=N + K)
        w8 = fp8_weights(bank)
        scale = pow2_scales(bank.launches * N, seed=N)
        t = scaled(bank.sums(n["xn"].view(1, K))[0], scale.view(bank.launches, N))
        for bias in (None, dr.integer_bias(N, seed=N)):
            for eps in (0.0, 1e-5):
                what = f"fp8 norm gemv N {N} residual {residual} bias {bias is not None} eps {eps}"
                y, h, _ = run(bank, w8, scale.to(DEV), n["x_d"], None if bias is None else dev16(bias), False, norm=n, eps=eps)
                assert_bits(y[:, :N], t if bias is None else (t.float() + bias.float()).bfloat16(), what)
                assert bool((y[:, N:] == SENT).all()), what + ": written past N"
                if residual:
                    assert_bits(h[:K], dr.to_bf16(n["h"]), what + " h")
                    assert bool((h[K:] == SENT).all())
    if residual:
        assert_bits(h[:K], add_rmsnorm_h(n), "h against skv_add_rmsnorm")
    I = 10
    bank = dr.pair_bank(I, K, seed=I + K, colsign=n["h"] // 2)
    w8 = fp8_weights(bank)
    s = bank.sums(n["xn"].view(1, K))[0]
    scale = pair_scales(s, I, seed=I)
    t = scaled(s, scale.view(bank.launches, 2 * I))
    y, h, _ = run(bank, w8, scale.to(DEV), n["x_d"], None, True, norm=n, eps=1e-5)
    assert_silu(y[:, :I], dr.silu_mul_ref(t[:, :I], t[:, I:]), f"fp8 norm gemv silu residual {residual}")
    assert bool((y[:, I:] == SENT).all())
    if residual:
        assert_bits(h[:K], dr.to_bf16(n["h"]), "silu h")


def test_fp8_norm_gemv_range_max():
    K, N = 4096, 4096
    bank = dr.plain_bank(N, K, seed=N + K + 5)
    w8 = fp8_weights(bank)
    scale = pow2_scales(bank.launches * N, seed=77)
    n = norm_on_device(K, seed=N, residual=True)
    y, h, keys = run(bank, w8, scale.to(DEV), n["x_d"], None, False, norm=n, eps=1e-5, rmax=True)
    want = scaled(bank.sums(n["xn"].view(1, K))[0], scale.view(bank.launches, N))
    assert_bits(y[:, :N], want, "fp8 range-max gemv")
    assert bool((y[:, N:] == SENT).all())
    assert_bits(h[:K], dr.to_bf16(n["h"]), "fp8 range-max h")
    got = keys[:, :N // 16].cpu().to(torch.int32) & 0xFFFF
    assert torch.equal(got, torch.stack([dr.range_max_ref(r) for r in y[:, :N].cpu()]))      # of the PRODUCED row
    assert bool((keys[:, N // 16:] == -1).all()), "a key written past N / 16"


ROWS, CS_ROWS = 12, 40


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("glm", [False, True], ids=["neox", "glm"])
def test_fp8_qkv_epilogue(glm, with_bias):
    """skv_qkv_gemv_rope_update_fp8, Hq = 2, Hkv = 1 (N = 512): norm form (K = 4096) and plain form (K = 1040); q, the cache
    row and the untouched sentinel rows against qkv_rope_cache_ref (bit for bit: the reference restates the kernel's
    roundings)."""
    _lib, L, st = _L()
    p = _lib.ptr
    Hq, Hkv, N = 2, 1, 512
    g = torch.Generator().manual_seed(11 + glm)
    cs = (torch.rand(CS_ROWS, 64 if glm else 128, generator=g) * 2 - 1).bfloat16()
    ov = torch.randn(1, Hq, 128, generator=g).bfloat16()
    cs_d = cs.to(DEV)
    for K, norm in ((4096, True), (1040, False)):
        bank = dr.plain_bank(N, K, seed=N + K + glm)
        w8 = fp8_weights(bank)
        scale = pow2_scales(bank.launches * N, seed=K)
        bias = dr.integer_bias(N, seed=K) if with_bias else None
        if norm:
            n = norm_on_device(K, seed=K, residual=True)
            xin, x_d = n["xn"].view(1, K), n["x_d"]
        else:
            xin, _ = dr.structured_x(1, K, seed=K)
            x_d = dev16(xin)
        t = scaled(bank.sums(xin)[0], scale.view(bank.launches, N))
        qkv = t if bias is None else (t.float() + bias.float()).bfloat16()
        # (device operands live in names for the whole loop: a pointer taken from a temporary dangles once the allocator reuses it)
        scale_d, bias_d, ov_d = scale.to(DEV), dev16(bias) if with_bias else None, ov.to(DEV)
        for l in range(bank.launches):
            for pos, row, override in ((17, 5, False), (CS_ROWS + 2, ROWS - 1, False), (9, ROWS, False), (21, 7, True)):
                what = f"fp8 qkv glm {glm} K {K} launch {l} pos {pos} row {row} override {override}"
                k = torch.full((1, Hkv, ROWS, 128), float("nan"), device=DEV).bfloat16()
                v = k.clone()
                q, h = sentinel_buf(Hq * 128 + PAD), sentinel_buf(K + PAD)
                pos_d, row_d = torch.tensor([pos], device=DEV), torch.tensor([row], device=DEV)
                rc = L.skv_qkv_gemv_rope_update_fp8(
                    p(w8[l * N:(l + 1) * N]), p(scale_d[l * N:(l + 1) * N]), p(x_d), p(n["res_d"]) if norm else 0,
                    p(n["w_d"]) if norm else 0, 1e-5, p(h) if norm else 0, p(bias_d), p(cs_d), p(pos_d),
                    p(row_d), p(ov_d) if override else 0, p(q), p(k), p(v), K, Hq, Hkv, 128, cs_d.stride(0), CS_ROWS,
                    k.stride(1), ROWS, 2 if glm else 1, st)
                assert rc == 0, rc
                torch.cuda.synchronize()
                q_ref, k_ref, v_ref = dr.qkv_rope_cache_ref(qkv[l:l + 1], cs, [pos], row, Hq, Hkv, ROWS, ov if override else None)
                assert_bits(q[:-PAD].view(1, Hq, 128), q_ref, what + " q")
                assert bool((q[-PAD:] == SENT).all()), what + ": written past q"
                assert_bits(k, k_ref, what + " k cache")
                assert_bits(v, v_ref, what + " v cache")
                if norm:
                    assert_bits(h[:K], dr.to_bf16(n["h"]), what + " h")
                else:
                    assert bool((h == SENT).all())


def test_fp8_byte_decoding_is_ocp_e4m3fn():
    """Row n holds byte n once, at column 37 n mod 1024 (every lane and every byte position of a word occur), zeros elsewhere;
    x = 1, scale = 1: y[n] is the value of byte n.  OCP e4m3fn against fnuz differ by a factor 2 on every normal value and on
    the meaning of 0x80; a swapped low / high word of the conversion moves the value to a column whose x is read elsewhere."""
    _lib, L, st = _L()
    N, K = 256, 1024
    b = torch.arange(256, dtype=torch.uint8)
    b[0x7F] = 0
    b[0xFF] = 0
    w = torch.zeros(N, K, dtype=torch.uint8)
    cols = (37 * torch.arange(N)) % K
    w[torch.arange(N), cols] = b
    # x = 1 only tells the decode apart; a second launch with x[k] = 1 + (k mod 4) / 4 also pins the byte -> element order
    want = b.view(torch.float8_e4m3fn).float()
    assert float(want[0x08]) == 2.0 ** -6 and float(want[0x01]) == 2.0 ** -9 and float(want[0x7E]) == 448.0 and float(want[0x80]) == 0.0
    for xv in (torch.ones(K), 1 + (torch.arange(K) % 4) / 4.0):
        y = sentinel_buf(N + PAD)
        wd, sd, xd = w.to(DEV), torch.ones(N, device=DEV), xv.bfloat16().to(DEV)
        rc = L.skv_gemv_fp8(_lib.ptr(wd), _lib.ptr(sd), _lib.ptr(xd), 0, _lib.ptr(y), N, K, 0, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        exp = want * xv[cols]                       # <= 4 + 3 significant bits: exact in bf16 (subnormal e4m3 values included)
        assert torch.equal(exp.bfloat16().float(), exp)
        got = y[:N].cpu().float()
        bad = (got != exp).nonzero().view(-1)
        assert bad.numel() == 0, f"bytes {[hex(int(i)) for i in bad[:8]]} decode to {got[bad[:8]].tolist()}, e4m3fn says {exp[bad[:8]].tolist()}"
        assert bool((y[N:] == SENT).all())


@pytest.mark.parametrize("K", [4096, 13696])
def test_fp8_gemv_gaussian_within_the_f32_accumulation_bound(K):
    """|y - ref| <= 2^-9 |ref| + (K + 2) 2^-24 scale[n] sum_k |w||x| against an f64 evaluation of the same dequantised operands:
    the output rounding to bf16 plus the worst-case error of K f32 additions, the reduction and the scale multiply, each 2^-24
    relative of the running magnitude sum |w||x|.  (Half a bf16 ulp is 2^-9 |ref| at the top of a binade and 2^-8 |ref| at its
    bottom; on Gaussian data sum |w||x| is ~0.6 sqrt(K) |ref|, so the accumulation term - 2^-7 |ref| and more here - covers
    the difference.  Both ratios are printed.)"""
    _lib, L, st = _L()
    from shadowkv_amd import tensor_op
    N = 64
    g = torch.Generator().manual_seed(K)
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    x = torch.randn(K, generator=g).bfloat16()
    w8, scale = tensor_op.quantize_fp8_rows(w)
    y = sentinel_buf(N + PAD)
    wd, sd, xd = w8.to(DEV), scale.to(DEV), x.to(DEV)
    rc = L.skv_gemv_fp8(_lib.ptr(wd), _lib.ptr(sd), _lib.ptr(xd), 0, _lib.ptr(y), N, K, 0, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((y[N:] == SENT).all())
    wq = w8.double()
    ref = scale.double() * (wq @ x.double())
    mag = scale.double() * (wq.abs() @ x.double().abs())
    # half a bf16 ulp of ref: ulp = 2^(floor(log2 |ref|) - 7)
    half_ulp = torch.ldexp(torch.ones(N, dtype=torch.float64), torch.frexp(ref)[1] - 1 - 8)
    assert bool((half_ulp <= 2.0 ** -8 * ref.abs()).all()) and bool((half_ulp >= 2.0 ** -9 * ref.abs()).all())
    acc = (K + 2) * 2.0 ** -24 * mag
    err = (y[:N].cpu().double() - ref).abs()
    bound = 2.0 ** -9 * ref.abs() + acc
    print(f"K {K}: worst |err| / bound {float((err / bound).max()):.3f}; worst |err| / (half ulp + acc) {float((err / (half_ulp + acc)).max()):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {N} outputs over the bound"


def test_fp8_near_pull_launches_change_no_bit_and_stage_like_bf16():
    """The gate/up and down FP8 launches with the near-miss pull role in front of their grid: y bit-equal to the launches
    without it, and the staged chunks (near_published_ids) equal what the bf16 launches publish from the same state."""
    from shadowkv_amd import tensor_op
    from test_gpu_kv_cache import _headline_cache
    caches = []
    for _ in range(2):
        c, cs, g = _headline_cache(8, False, L=16384, seed=41)
        c.near_lists = 2
        c.enable_early_fetch(near=True)
        caches.append((c, cs, g))
    ca, cb = caches[0][0], caches[1][0]
    gw = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(1, 1, 4096, device=DEV, generator=gw).bfloat16()
    res = torch.randn(1, 1, 4096, device=DEV, generator=gw).bfloat16()
    nw = (1 + 0.1 * torch.randn(4096, device=DEV, generator=gw)).bfloat16()
    w = (torch.randn(2 * 512, 4096, device=DEV, generator=gw) * 0.02).bfloat16()
    a = torch.randn(1, 1, 1024, device=DEV, generator=gw).bfloat16()
    wd = (torch.randn(4096, 1024, device=DEV, generator=gw) * 0.02).bfloat16()
    w8, ws = tensor_op.quantize_fp8_rows(w)
    wd8, wds = tensor_op.quantize_fp8_rows(wd)
    kv_len = ca.sparse_end + 2
    staged = 0
    for step in range(3):
        outs = []
        for c, cs, g in caches:             # (the two generators are in the same state: the same query walk)
            q = (torch.randn(1, 32, 1, 128, device=DEV, generator=g) * 1.5).bfloat16()
            outs.append(c.select_fetch_attend_inplace(0, q, cs, kv_len=kv_len))
        torch.cuda.synchronize()
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
        assert torch.equal(ca.near_published_ids(0), cb.near_published_ids(0))
        h0, y0 = tensor_op.norm_linear_decode(x, res, nw, 1e-5, w8, fuse_silu_mul=True, w_scale=ws)
        args = ca.near_pull_args(0)
        assert args is not None
        h1, y1 = tensor_op.norm_linear_decode(x, res, nw, 1e-5, w8, fuse_silu_mul=True, near_pull=args, w_scale=ws)
        tensor_op.norm_linear_decode(x, res, nw, 1e-5, w, fuse_silu_mul=True, near_pull=cb.near_pull_args(0))
        torch.cuda.synchronize()
        assert torch.equal(h0.view(torch.int16), h1.view(torch.int16)) and torch.equal(y0.view(torch.int16), y1.view(torch.int16))
        assert torch.equal(ca.near_published_ids(0), cb.near_published_ids(0)), (step, "gate/up")
        d0 = tensor_op.linear_decode(a, wd8, bias=h0, w_scale=wds)
        args1 = ca.near_pull_args(0, 1)
        assert args1 is not None and args1[-1] == 1
        d1 = tensor_op.linear_decode(a, wd8, bias=h0, near_pull=args1, w_scale=wds)
        tensor_op.linear_decode(a, wd, bias=h0, near_pull=cb.near_pull_args(0, 1))
        torch.cuda.synchronize()
        assert torch.equal(d0.view(torch.int16), d1.view(torch.int16))
        pa, pb = ca.near_published_ids(0), cb.near_published_ids(0)
        assert torch.equal(pa, pb), (step, "down")
        staged += int((pa >= 0).sum())
    assert staged > 0
