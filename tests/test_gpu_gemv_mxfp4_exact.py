"""GPU: the weight-only MXFP4 GEMV kernels (skv_gemv_mxfp4.hip) against tests/mxfp4_ref.py, bit for bit.

The banks' weights {+-1, +-2, +-3} are e2m1 numbers, the block scales powers of two from 2^-2 .. 2^2 that alternate between
the blocks of a row, x and the bias small integers: every partial sum in every order is exact in f32 and the result is a bf16
number (mxfp4_ref.MxBank.expected asserts both) - raw bits are compared.  SiLU carries dense_ref.SILU_RTOL; the decode of
nibbles and scale bytes is pinned element by element; the Gaussian case carries a bound derived from the formats."""
import numpy as np
import pytest
import torch

import dense_ref as dr
import mxfp4_ref as mr

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


def run(mx, x, bias, silu, norm=None, eps=0.0, rmax=False):
    """One launch per matrix of the bank: (y [launches, No + PAD], h | None, keys | None)"""
    _lib, L, st = _L()
    p = _lib.ptr
    N, K = mx.rows, mx.K
    No = N // 2 if silu else N
    w4, sc = mx.w4.to(DEV), mx.w_scale.to(DEV)
    y = sentinel_buf(mx.launches, No + PAD)
    h = sentinel_buf(K + PAD) if norm is not None and norm["residual"] is not None else None
    keys = torch.full((mx.launches, (N // 16 + 7) // 8 * 8 + PAD), -1, dtype=torch.int16, device=DEV) if rmax else None
    for l in range(mx.launches):
        wl, sl = w4[l * N:(l + 1) * N], sc[l * N:(l + 1) * N]
        if norm is None:
            rc = L.skv_gemv_mxfp4(p(wl), p(sl), p(x), p(bias), p(y[l]), N, K, int(silu), st)
        elif rmax:
            rc = L.skv_norm_gemv_rangemax_mxfp4(p(wl), p(sl), p(x), p(norm["res_d"]), p(norm["w_d"]), eps, p(h), p(bias), p(y[l]), N, K,
                                                p(keys[l]), st)
        else:
            rc = L.skv_norm_gemv_mxfp4(p(wl), p(sl), p(x), p(norm["res_d"]), p(norm["w_d"]), eps, p(h), p(bias), p(y[l]), N, K,
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


def with_bias(t, bias):
    # bf16(bf16r(t) + bias): t is a bf16 number, t + bias is exact in f32 (<= 9 + 2 bits), rounded once
    return t if bias is None else (t.float() + bias.float()).bfloat16()


# K: the tail alone (32 lanes); one step; one step + a tail of one lane; two steps; 6 steps + a 44-lane tail (GLM-4's
# intermediate size).  N: 37 = ragged against 4 waves x 2 rows (clamped rows in the last workgroup)
KS = (1024, 2048, 2048 + 32, 4096, 13696)


@pytest.mark.parametrize("K", KS)
def test_mxfp4_gemv_plain_and_bias_exact(K):
    """skv_gemv_mxfp4 at R = 2 (N <= 8192), N = 37."""
    N = 37
    mx = mr.plain_mx_bank(N, K, seed=N + K)
    xi, _ = dr.structured_x(1, K, seed=K)
    t = mx.expected(xi[0])
    for bias in (None, dr.integer_bias(N, seed=N)):
        y, _, _ = run(mx, dev16(xi), None if bias is None else dev16(bias), silu=False)
        assert_bits(y[:, :N], with_bias(t, bias), f"mxfp4 gemv N {N} K {K} bias {bias is not None}")
        assert bool((y[:, N:] == SENT).all()), "written past N"


def test_mxfp4_gemv_four_rows_per_wave_exact():
    """N > 8192 takes the R = 4 instance: 8200 x 2048 (a ragged last workgroup), and x 2080 for its tail."""
    for N, K in ((8200, 2048), (8200, 2080)):
        mx = mr.plain_mx_bank(N, K, seed=N + K)
        assert mx.launches == 1
        xi, _ = dr.structured_x(1, K, seed=K)
        t = mx.expected(xi[0])
        bias = dr.integer_bias(N, seed=N)
        for b in (None, bias):
            y, _, _ = run(mx, dev16(xi), None if b is None else dev16(b), silu=False)
            assert_bits(y[:, :N], with_bias(t, b), f"mxfp4 gemv N {N} K {K} bias {b is not None}")
            assert bool((y[:, N:] == SENT).all()), "written past N"


@pytest.mark.parametrize("K", KS)
def test_mxfp4_gemv_silu_pair(K):
    I = 11                                                          # odd: the last wave holds one pair and one clamped pair
    xi, colsign = dr.structured_x(1, K, seed=K + 1)
    mx = mr.pair_mx_bank(I, K, seed=I + K, colsign=colsign, x=xi[0])
    t = mx.expected(xi[0])
    g, u = t[:, :I], t[:, I:]
    assert bool((g != 0).all()) and bool((u != 0).all())
    y, _, _ = run(mx, dev16(xi), None, silu=True)
    assert_silu(y[:, :I], dr.silu_mul_ref(g, u), f"mxfp4 gemv silu K {K}")
    assert bool((y[:, I:] == SENT).all()), "written past I"


@pytest.mark.parametrize("residual", [True, False])
def test_mxfp4_norm_gemv_exact(residual):
    """Norm prologue + plain / bias GEMV (N = 37, 4101: ragged against 4 waves x 4 rows) and + SiLU pair: outputs and h
    bit-equal to the references, h also bit-equal to skv_add_rmsnorm's."""
    K = 4096
    n = norm_on_device(K, seed=3 + residual, residual=residual)
    for N in (37, 4101):
        mx = mr.plain_mx_bank(N, K, seed=N + K)
        t = mx.expected(n["xn"])
        for bias in (None, dr.integer_bias(N, seed=N)):
            for eps in (0.0, 1e-5):
                what = f"mxfp4 norm gemv N {N} residual {residual} bias {bias is not None} eps {eps}"
                y, h, _ = run(mx, n["x_d"], None if bias is None else dev16(bias), False, norm=n, eps=eps)
                assert_bits(y[:, :N], with_bias(t, bias), what)
                assert bool((y[:, N:] == SENT).all()), what + ": written past N"
                if residual:
                    assert_bits(h[:K], dr.to_bf16(n["h"]), what + " h")
                    assert bool((h[K:] == SENT).all())
    if residual:
        assert_bits(h[:K], add_rmsnorm_h(n), "h against skv_add_rmsnorm")
    I = 11
    mx = mr.pair_mx_bank(I, K, seed=I + K, colsign=n["h"] // 2, x=n["xn"])
    t = mx.expected(n["xn"])
    y, h, _ = run(mx, n["x_d"], None, True, norm=n, eps=1e-5)
    assert_silu(y[:, :I], dr.silu_mul_ref(t[:, :I], t[:, I:]), f"mxfp4 norm gemv silu residual {residual}")
    assert bool((y[:, I:] == SENT).all())
    if residual:
        assert_bits(h[:K], dr.to_bf16(n["h"]), "silu h")


def test_mxfp4_norm_gemv_range_max():
    K, N = 4096, 4096
    mx = mr.plain_mx_bank(N, K, seed=N + K + 5)
    n = norm_on_device(K, seed=N, residual=True)
    y, h, keys = run(mx, n["x_d"], None, False, norm=n, eps=1e-5, rmax=True)
    assert_bits(y[:, :N], mx.expected(n["xn"]), "mxfp4 range-max gemv")
    assert bool((y[:, N:] == SENT).all())
    assert_bits(h[:K], dr.to_bf16(n["h"]), "mxfp4 range-max h")
    got = keys[:, :N // 16].cpu().to(torch.int32) & 0xFFFF
    assert torch.equal(got, torch.stack([dr.range_max_ref(r) for r in y[:, :N].cpu()]))      # of the PRODUCED row
    assert bool((keys[:, N // 16:] == -1).all()), "a key written past N / 16"


ROWS, CS_ROWS = 12, 40


@pytest.mark.parametrize("bias_on", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("glm", [False, True], ids=["neox", "glm"])
def test_mxfp4_qkv_epilogue(glm, bias_on):
    """skv_qkv_gemv_rope_update_mxfp4, Hq = 2, Hkv = 1 (N = 512): norm form (K = 4096) and plain form (K = 2080); q, the cache
    row and the untouched sentinel rows against qkv_rope_cache_ref (bit for bit: the reference restates the kernel's
    roundings); a position past the table, a row past the cache, q_override."""
    _lib, L, st = _L()
    p = _lib.ptr
    Hq, Hkv, N = 2, 1, 512
    g = torch.Generator().manual_seed(11 + glm)
    cs = (torch.rand(CS_ROWS, 64 if glm else 128, generator=g) * 2 - 1).bfloat16()
    ov = torch.randn(1, Hq, 128, generator=g).bfloat16()
    cs_d = cs.to(DEV)
    for K, norm in ((4096, True), (2080, False)):
        mx = mr.plain_mx_bank(N, K, seed=N + K + glm)
        bias = dr.integer_bias(N, seed=K) if bias_on else None
        if norm:
            n = norm_on_device(K, seed=K, residual=True)
            xin, x_d = n["xn"], n["x_d"]
        else:
            xin = dr.structured_x(1, K, seed=K)[0][0]
            x_d = dev16(xin)
        qkv = with_bias(mx.expected(xin), bias)
        # (device operands live in names for the whole loop: a pointer taken from a temporary dangles once the allocator reuses it)
        w4_d, sc_d, bias_d, ov_d = mx.w4.to(DEV), mx.w_scale.to(DEV), dev16(bias) if bias_on else None, ov.to(DEV)
        for l in range(mx.launches):
            for pos, row, override in ((17, 5, False), (CS_ROWS + 2, ROWS - 1, False), (9, ROWS, False), (21, 7, True)):
                what = f"mxfp4 qkv glm {glm} K {K} launch {l} pos {pos} row {row} override {override}"
                k = torch.full((1, Hkv, ROWS, 128), float("nan"), device=DEV).bfloat16()
                v = k.clone()
                q, h = sentinel_buf(Hq * 128 + PAD), sentinel_buf(K + PAD)
                pos_d, row_d = torch.tensor([pos], device=DEV), torch.tensor([row], device=DEV)
                rc = L.skv_qkv_gemv_rope_update_mxfp4(
                    p(w4_d[l * N:(l + 1) * N]), p(sc_d[l * N:(l + 1) * N]), p(x_d), p(n["res_d"]) if norm else 0,
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


def test_mxfp4_nibble_byte_and_scale_decoding():
    """Rows with ONE non-zero nibble (mxfp4_ref.decode_probe_rows): all 16 codes x both nibbles x all 16 byte positions of a
    lane's 16-byte load x lanes {0, 1, 63}; every code at scale bytes {27, 126, 127, 128, 227}; code 6 at every scale byte
    27 .. 227.  x = 1 gives the element's value (sign, e2m1 code, e8m0 byte - the other blocks of the row carry another scale
    byte).  Two more launches tell where the element was read: x[k] = 1 + (k mod 32) / 32 separates the 32 elements of a lane
    (nibble order, byte order within the load), x[k] = 1 + (k / 32 mod 32) / 32 the lanes.  Products have <= 2 + 6 significant
    bits: exact in bf16."""
    _lib, L, st = _L()
    K = 2048
    w4, sc, col, val = mr.decode_probe_rows(K=K)
    N = w4.shape[0]
    k = torch.arange(K)
    w4_d, sc_d = w4.to(DEV), sc.to(DEV)
    for name, xv in (("ones", torch.ones(K)), ("element", 1 + (k % 32) / 32.0), ("lane", 1 + (k // 32 % 32) / 32.0)):
        y = sentinel_buf(N + PAD)
        xd = xv.bfloat16().to(DEV)
        assert torch.equal(xd.cpu().float(), xv)
        rc = L.skv_gemv_mxfp4(_lib.ptr(w4_d), _lib.ptr(sc_d), _lib.ptr(xd), 0, _lib.ptr(y), N, K, 0, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        exp = val * xv[col].double()
        assert torch.equal(exp.bfloat16().double(), exp)
        got = y[:N].cpu().double()
        bad = (got != exp).nonzero().view(-1)
        assert bad.numel() == 0, f"x = {name}: {bad.numel()} of {N} rows differ, rows {bad[:8].tolist()} (columns " \
                                 f"{col[bad[:8]].tolist()}) give {got[bad[:8]].tolist()}, the format says {exp[bad[:8]].tolist()}"
        assert bool((y[N:] == SENT).all())


@pytest.mark.parametrize("K", [4096, 13696])
def test_mxfp4_gemv_gaussian_within_the_f32_accumulation_bound(K):
    """Against the f64 restatement over the same (w4, w_scale) bytes.  The products 2^s e2m1 x are exact in f32 (2 + 8 bits).
    Any order of summing K f32 terms errs by at most gamma = (K - 1) u / (1 - (K - 1) u) times sum_k |w||x|, u = 2^-24 (the
    f32 FMAs and the reduction tree are such an order; there is no multiply after the reduction).  The sum t is then rounded
    once to bf16: |y - t| <= 2^-8 |t| (8 significant bits), and |t| <= |ref| + gamma mag.  So
        |y - ref| <= gamma mag + 2^-8 (|ref| + gamma mag).
    This is the derivation of tests/test_gpu_gemv_fp8_exact.py's Gaussian case without the scale multiply and with the output
    rounding stated at its worst case; the share of the bound that is used is printed."""
    _lib, L, st = _L()
    from shadowkv_amd import tensor_op
    N = 64
    g = torch.Generator().manual_seed(K)
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    x = torch.randn(K, generator=g).bfloat16()
    w4, sc = tensor_op.quantize_mxfp4_rows(w)
    y = sentinel_buf(N + PAD)
    wd, sd, xd = w4.to(DEV), sc.to(DEV), x.to(DEV)
    rc = L.skv_gemv_mxfp4(_lib.ptr(wd), _lib.ptr(sd), _lib.ptr(xd), 0, _lib.ptr(y), N, K, 0, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((y[N:] == SENT).all())
    ref, mag = mr.gemv64(w4, sc, x)
    u = 2.0 ** -24
    gamma = (K - 1) * u / (1 - (K - 1) * u)
    bound = gamma * mag + 2.0 ** -8 * (np.abs(ref) + gamma * mag)
    err = np.abs(y[:N].cpu().double().numpy() - ref)
    print(f"K {K}: worst |err| / bound {float((err / bound).max()):.3f}; gamma mag / |ref| up to {float((gamma * mag / np.abs(ref)).max()):.3e}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {N} outputs over the bound"


def test_mxfp4_near_pull_launches_change_no_bit_and_stage_like_bf16():
    """The gate/up and down MXFP4 launches with the near-miss pull role in front of their grid: y bit-equal to the launches
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
    w4, ws = tensor_op.quantize_mxfp4_rows(w)
    wd4, wds = tensor_op.quantize_mxfp4_rows(wd)
    kv_len = ca.sparse_end + 2
    staged = 0
    n0, f0 = tensor_op.mxfp4_native_calls, tensor_op.mxfp4_fallback_calls
    for step in range(3):
        outs = []
        for c, cs, g in caches:             # (the two generators are in the same state: the same query walk)
            q = (torch.randn(1, 32, 1, 128, device=DEV, generator=g) * 1.5).bfloat16()
            outs.append(c.select_fetch_attend_inplace(0, q, cs, kv_len=kv_len))
        torch.cuda.synchronize()
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
        assert torch.equal(ca.near_published_ids(0), cb.near_published_ids(0))
        h0, y0 = tensor_op.norm_linear_decode(x, res, nw, 1e-5, w4, fuse_silu_mul=True, w_scale=ws)
        args = ca.near_pull_args(0)
        assert args is not None
        h1, y1 = tensor_op.norm_linear_decode(x, res, nw, 1e-5, w4, fuse_silu_mul=True, near_pull=args, w_scale=ws)
        tensor_op.norm_linear_decode(x, res, nw, 1e-5, w, fuse_silu_mul=True, near_pull=cb.near_pull_args(0))
        torch.cuda.synchronize()
        assert torch.equal(h0.view(torch.int16), h1.view(torch.int16)) and torch.equal(y0.view(torch.int16), y1.view(torch.int16))
        assert torch.equal(ca.near_published_ids(0), cb.near_published_ids(0)), (step, "gate/up")
        d0 = tensor_op.linear_decode(a, wd4, bias=h0, w_scale=wds)
        args1 = ca.near_pull_args(0, 1)
        assert args1 is not None and args1[-1] == 1
        d1 = tensor_op.linear_decode(a, wd4, bias=h0, near_pull=args1, w_scale=wds)
        tensor_op.linear_decode(a, wd, bias=h0, near_pull=cb.near_pull_args(0, 1))
        torch.cuda.synchronize()
        assert torch.equal(d0.view(torch.int16), d1.view(torch.int16))
        pa, pb = ca.near_published_ids(0), cb.near_published_ids(0)
        assert torch.equal(pa, pb), (step, "down")
        staged += int((pa >= 0).sum())
    assert staged > 0
    assert tensor_op.mxfp4_native_calls - n0 == 12 and tensor_op.mxfp4_fallback_calls == f0
    # the launch's y is the dequantised weights' product, not merely self-consistent: against the f64 restatement of the down
    # projection (bias h0), under the Gaussian case's bound plus the bias add's rounding (bf16(bf16r(t) + bias))
    ref, mag = mr.gemv64(wd4, wds, a.view(-1).cpu())
    K = 1024
    gamma = (K - 1) * 2.0 ** -24 / (1 - (K - 1) * 2.0 ** -24)
    t_err = gamma * mag + 2.0 ** -8 * (np.abs(ref) + gamma * mag)
    hb = h0.view(-1).cpu().double().numpy()
    bound = t_err + 2.0 ** -8 * (np.abs(ref) + t_err + np.abs(hb))
    assert bool((np.abs(d0.view(-1).cpu().double().numpy() - (ref + hb)) <= bound).all())
