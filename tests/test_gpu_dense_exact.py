"""GPU: the dense kernels of a decode layer - skv_gemv.hip (every template path of launch_gemv), skv_rows_gemm.hip (every
branch of skv_rows_pick), skv_dense.hip, the QKV epilogue and the k/v role of skv_kvproj.h, the sampler's range keys - against
tests/dense_ref.py.  The inputs are built so that the exact result is a small integer: every order of
f32 accumulation gives it and bf16 holds it, so the comparison is on raw bits and one dropped, doubled or misplaced k element
fails it.  SiLU (fast exp) and RMSNorm on random data (f32 rsqrt) carry bounds from the number formats alone.  No expected
value here comes from another kernel of the family.  Every output buffer carries sentinels past its end."""
import pytest
import torch

import dense_ref as dr
import util
from dense_ref import expected_branch
from test_gpu_kv_proj_split import PLACEMENTS, run_selection, select_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 1000.0                    # bf16-exact, outside every expected output
PAD = 8


def _L():
    from shadowkv_amd import _lib
    return _lib, _lib.lib(), _lib.current_stream_handle()


def dev16(v):
    return dr.to_bf16(v).to(DEV)


def sentinel_buf(*shape):
    return torch.full(shape, SENT, dtype=torch.bfloat16, device=DEV)


def assert_bits(got, want, what):
    """Raw bits; a NaN (the caches' sentinel, whose payload is the host's or the device's) equals any NaN and nothing else."""
    got, want = got.cpu(), want.cpu()
    a, b = (torch.where(torch.isnan(t.float()), 0x7FC0, dr.bits(t)) for t in (got, want))
    bad = (a != b).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {a.numel()} bf16 values differ, first at {bad[0].tolist()}: " \
                             f"got {float(got.float()[tuple(bad[0])])}, want {float(want.float()[tuple(bad[0])])}"


def assert_silu(got, ref, what):
    """|out - ref| <= 3 * 2^-9 |ref| (dense_ref.SILU_RTOL); the worst ratio is printed before the assertion."""
    err, tol = (got.cpu().double() - ref).abs(), dr.SILU_RTOL * ref.abs()
    worst = float((err / tol.clamp_min(1e-300)).max()) if bool((tol > 0).any()) else 0.0
    print(f"{what}: values {err.numel()}  differing {int((err > 0).sum())}  worst |err| / bound {worst:.3f}")
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} of {err.numel()} values over 3 * 2^-9 |ref|, worst x{worst:.2f}"


def weights_on_device(bank):
    w = bank.dense(DEV)
    assert bool((w != 0).any(0).all()), "a column of the weight bank is zero in every row"      # the coverage condition
    return w


def run_gemv(bank, w, x, bias, silu, norm=None, eps=0.0, rmax=False):
    """One launch per matrix of the bank.  Returns (y [launches, No + PAD], h_out [K + PAD] | None, keys [launches, ..] | None)."""
    _lib, L, st = _L()
    N, K = bank.rows, bank.K
    No = N // 2 if silu else N
    y = sentinel_buf(bank.launches, No + PAD)
    h = sentinel_buf(K + PAD) if norm is not None and norm["residual"] is not None else None
    nkeys = (N // 16 + 7) // 8 * 8 + PAD
    keys = torch.full((bank.launches, nkeys), -1, dtype=torch.int16, device=DEV) if rmax else None
    p = _lib.ptr
    for l in range(bank.launches):
        wl = w[l * N:(l + 1) * N]
        if norm is None:
            rc = L.skv_gemv_bf16(p(wl), p(x), p(bias), p(y[l]), N, K, int(silu), st)
        elif rmax:
            rc = L.skv_norm_gemv_rangemax_bf16(p(wl), p(x), p(norm["res_d"]), p(norm["w_d"]), eps, p(h), p(bias), p(y[l]), N, K,
                                               p(keys[l]), st)
        else:
            rc = L.skv_norm_gemv_bf16(p(wl), p(x), p(norm["res_d"]), p(norm["w_d"]), eps, p(h), p(bias), p(y[l]), N, K, int(silu), st)
        assert rc == 0, rc
    torch.cuda.synchronize()
    return y, h, keys


def norm_on_device(K, seed, residual):
    n = dr.norm_inputs(K, seed, residual)
    n["x_d"], n["w_d"] = dev16(n["x"]), dev16(n["w_norm"])
    n["res_d"] = dev16(n["residual"]) if residual else None
    return n


def check_h(h, n, what):
    if h is not None:
        assert_bits(h[:-PAD], dr.to_bf16(n["h"]), what + " h_out")
        assert bool((h[-PAD:] == SENT).all()), what + ": written past h_out"


# --------------------------------------------------------------------------------------------------------------- GEMV
@pytest.mark.parametrize("N,K", [(N, K) for N in (1, 7, 8, 9, 4101) for K in (512, 520, 1024, 4104, 13696)] +
                                [(N, K) for N in (8193, 8209) for K in (512, 1000)])
def test_gemv_plain_exact(N, K):
    """skv_gemv_kernel<2> (N <= 8192) and <4>: K % 512 tails of 1, 61 and 48 lanes, none; ragged N (clamped rows)."""
    bank = dr.plain_bank(N, K, seed=N + K)
    w = weights_on_device(bank)
    xi, _ = dr.structured_x(1, K, seed=K)
    x = dev16(xi)
    for bias in (None, dr.integer_bias(N, seed=N)):
        y, _, _ = run_gemv(bank, w, x, None if bias is None else dev16(bias), silu=False)
        assert_bits(y[:, :N], dr.gemv_ref(bank, xi, bias)[0], f"gemv N {N} K {K} bias {bias is not None}")
        assert bool((y[:, N:] == SENT).all()), "written past N"


@pytest.mark.parametrize("I,K", [(I, K) for I in (1, 7, 9, 1003, 3425) for K in (512, 520, 13696)])
def test_gemv_silu_pair(I, K):
    xi, colsign = dr.structured_x(1, K, seed=K + 1)
    bank = dr.pair_bank(I, K, seed=I + K, colsign=colsign)
    w = weights_on_device(bank)
    g, u, ref = dr.pair_ref(bank, xi)
    assert bool((g != 0).all()) and bool((u != 0).all())
    y, _, _ = run_gemv(bank, w, dev16(xi), None, silu=True)
    assert_silu(y[:, :I], ref[0], f"gemv silu I {I} K {K}")
    assert bool((y[:, I:] == SENT).all()), "written past I"


@pytest.mark.parametrize("N", [1, 15, 17, 4101, 8193])
def test_norm_gemv_plain_exact(N):
    K = 4096
    bank = dr.plain_bank(N, K, seed=N + K)
    w = weights_on_device(bank)
    for residual in (True, False):
        n = norm_on_device(K, seed=N + residual, residual=residual)
        for bias in (None, dr.integer_bias(N, seed=N)):
            for eps in (0.0, 1e-5):
                what = f"norm gemv N {N} residual {residual} bias {bias is not None} eps {eps}"
                y, h, _ = run_gemv(bank, w, n["x_d"], None if bias is None else dev16(bias), silu=False, norm=n, eps=eps)
                assert_bits(y[:, :N], dr.gemv_ref(bank, n["xn"].view(1, K), bias)[0], what)
                assert bool((y[:, N:] == SENT).all()), what + ": written past N"
                check_h(h, n, what)


@pytest.mark.parametrize("I", [1, 9, 1003])
def test_norm_gemv_silu_pair(I):
    K = 4096
    for eps in (0.0, 1e-5):
        n = norm_on_device(K, seed=I, residual=True)
        bank = dr.pair_bank(I, K, seed=I + K, colsign=n["h"] // 2)
        w = weights_on_device(bank)
        g, u, ref = dr.pair_ref(bank, n["xn"].view(1, K))
        assert bool((g != 0).all()) and bool((u != 0).all())
        y, h, _ = run_gemv(bank, w, n["x_d"], None, silu=True, norm=n, eps=eps)
        assert_silu(y[:, :I], ref[0], f"norm gemv silu I {I} eps {eps}")
        assert bool((y[:, I:] == SENT).all()), "written past I"
        check_h(h, n, f"norm gemv silu I {I}")


@pytest.mark.parametrize("N", [16, 48, 32000])
def test_norm_gemv_range_max_exact(N):
    K = 4096
    bank = dr.plain_bank(N, K, seed=N + K)
    w = weights_on_device(bank)
    n = norm_on_device(K, seed=N, residual=True)
    for bias in (None, dr.integer_bias(N, seed=N)):
        y, h, keys = run_gemv(bank, w, n["x_d"], None if bias is None else dev16(bias), silu=False, norm=n, eps=1e-5, rmax=True)
        ref = dr.gemv_ref(bank, n["xn"].view(1, K), bias)[0]
        assert_bits(y[:, :N], ref, f"range-max gemv N {N}")
        assert bool((y[:, N:] == SENT).all())
        check_h(h, n, f"range-max gemv N {N}")
        want = torch.stack([dr.range_max_ref(r) for r in ref])
        assert torch.equal(keys[:, :N // 16].cpu().to(torch.int32) & 0xFFFF, want)
        assert bool((keys[:, N // 16:] == -1).all()), "a key written past N / 16"


def near_cache():
    """A fresh early state as test_gpu_gemv_fp8_exact's near-pull test builds it (8 KV heads, 16,384 tokens, two near-miss lists)
    after one selection step: its near-miss lists are what the pull role of a launch stages; no launch has staged into it."""
    from test_gpu_kv_cache import _headline_cache
    c, cs, g = _headline_cache(8, False, L=16384, seed=41)
    c.near_lists = 2
    c.enable_early_fetch(near=True)
    q = (torch.randn(1, 32, 1, 128, device=DEV, generator=g) * 1.5).bfloat16()
    c.select_fetch_attend_inplace(0, q, cs, kv_len=c.sparse_end + 2)
    torch.cuda.synchronize()
    return c


@pytest.mark.parametrize("launch", ["gate_up", "down"])
def test_near_pull_launches_change_no_bit(launch):
    """skv_norm_gemv_near_pull_bf16 (gate/up, K = 4096, I = 9) and skv_gemv_near_pull_bf16 (down, N = 9, K = 520: ragged last
    workgroup, a K tail): y and h bit-equal to the launch without the pull role in front of its grid, and the role staged."""
    _lib, L, st = _L()
    p = _lib.ptr
    c = near_cache()
    if launch == "gate_up":
        I, K = 9, 4096
        n = norm_on_device(K, seed=I, residual=True)
        bank = dr.pair_bank(I, K, seed=I + K, colsign=n["h"] // 2)
        w = weights_on_device(bank)
        y0, h0, _ = run_gemv(bank, w, n["x_d"], None, silu=True, norm=n, eps=1e-5)
        args = c.near_pull_args(0)
        assert args is not None
        y1, h1 = sentinel_buf(bank.launches, I + PAD), sentinel_buf(K + PAD)
        for l in range(bank.launches):
            rc = L.skv_norm_gemv_near_pull_bf16(p(w[l * 2 * I:(l + 1) * 2 * I]), p(n["x_d"]), p(n["res_d"]), p(n["w_d"]), 1e-5, p(h1),
                                                p(y1[l]), 2 * I, K, *args, st)
            assert rc == 0, rc
        torch.cuda.synchronize()
        check_h(h1, n, "near-pull gate/up")
        assert torch.equal(h0.view(torch.int16), h1.view(torch.int16))
    else:
        N, K = 9, 520
        bank = dr.plain_bank(N, K, seed=N + K)
        w = weights_on_device(bank)
        xi, _ = dr.structured_x(1, K, seed=K)
        x, bias = dev16(xi), dev16(dr.integer_bias(N, seed=N))
        y0, _, _ = run_gemv(bank, w, x, bias, silu=False)
        args = c.near_pull_args(0, 1)
        assert args is not None and args[-1] == 1
        y1 = sentinel_buf(bank.launches, N + PAD)
        for l in range(bank.launches):
            rc = L.skv_gemv_near_pull_bf16(p(w[l * N:(l + 1) * N]), p(x), p(bias), p(y1[l]), N, K, *args, st)
            assert rc == 0, rc
        torch.cuda.synchronize()
        assert_bits(y1[:, :N], dr.gemv_ref(bank, xi, dr.integer_bias(N, seed=N))[0], "near-pull down")
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16)), "the pull role changed an output bit (sentinels included)"
    own = c.near_published_ids(0)[:, 64:] if launch == "down" else c.near_published_ids(0)[:, :64]     # the launch's own list
    assert int((own >= 0).sum()) > 0, "the pull role staged no chunk of its list"


# ---------------------------------------------------------------------------------------------- QKV epilogue, k/v role
ROWS = 12                        # cache rows per head
CS_ROWS = 40
QKV_CFG = {"neox_32_8": (32, 8, False, False), "neox_4_1": (4, 1, False, False), "glm_32_4": (32, 4, True, False),
           "glm_2_1_bias": (2, 1, True, True)}
# (pos, row, q_override): pos inside / negative / past the table; row inside / -1 / = cache rows; override
QKV_VARIANTS = [(17, 5, False), (-3, 0, False), (CS_ROWS + 2, ROWS - 1, False), (9, -1, False), (9, ROWS, False), (21, 7, True)]


def cos_sin_table(glm, seed, rows=CS_ROWS):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(rows, 64 if glm else 128, generator=g) * 2 - 1).bfloat16()


def qkv_case(Hq, Hkv, glm, with_bias, K, norm, seed):
    """Weights, inputs and the exact projection output (bf16 [1, N]) of one token."""
    N = (Hq + 2 * Hkv) * 128
    bank = dr.plain_bank(N, K, seed=seed + N + K)
    assert bank.launches == 1
    c = dict(Hq=Hq, Hkv=Hkv, glm=glm, K=K, N=N, w=weights_on_device(bank), bias=dr.integer_bias(N, seed) if with_bias else None)
    if norm:
        c["n"] = norm_on_device(K, seed, residual=True)
        xin = c["n"]["xn"].view(1, K)
    else:
        xin, _ = dr.structured_x(1, K, seed)
        c["x_d"] = dev16(xin)
    c["bias_d"] = dev16(c["bias"]) if with_bias else None
    c["qkv"] = dr.gemv_ref(bank, xin, c["bias"])[0]
    c["cs"] = cos_sin_table(glm, seed)
    c["cs_d"] = c["cs"].to(DEV)
    c["ov"] = torch.randn(1, Hq, 128, generator=torch.Generator().manual_seed(seed + 1)).bfloat16()
    return c


def nan_caches(bs, Hkv):
    k = torch.full((bs, Hkv, ROWS, 128), float("nan"), device=DEV).bfloat16()
    return k, k.clone()


@pytest.mark.parametrize("form", ["norm_k4096", "plain_k520", "plain_k4096"])
@pytest.mark.parametrize("cfg", list(QKV_CFG))
def test_qkv_gemv_epilogue_exact(cfg, form):
    """skv_qkv_gemv_rope_update, one launch: residual add, norm, GEMV, bias, split, RoPE, cache push - predicted bit for bit."""
    _lib, L, st = _L()
    p = _lib.ptr
    Hq, Hkv, glm, with_bias = QKV_CFG[cfg]
    norm, K = form.startswith("norm"), int(form.split("_k")[1])
    c = qkv_case(Hq, Hkv, glm, with_bias, K, norm, seed=len(cfg) + K)
    for pos, row, override in QKV_VARIANTS:
        what = f"{cfg} {form} pos {pos} row {row} override {override}"
        k, v = nan_caches(1, Hkv)
        q = sentinel_buf(Hq * 128 + PAD)
        h = sentinel_buf(K + PAD)
        ov = c["ov"].to(DEV) if override else None
        pos_d, row_d = torch.tensor([pos], device=DEV), torch.tensor([row], device=DEV)
        n = c.get("n")
        rc = L.skv_qkv_gemv_rope_update(p(c["w"]), p(n["x_d"] if norm else c["x_d"]), p(n["res_d"]) if norm else 0,
                                        p(n["w_d"]) if norm else 0, 1e-5, p(h) if norm else 0, p(c["bias_d"]), p(c["cs_d"]), p(pos_d),
                                        p(row_d), p(ov), p(q), p(k), p(v), K, Hq, Hkv, 128, c["cs_d"].stride(0), CS_ROWS,
                                        k.stride(1), ROWS, 2 if glm else 1, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        q_ref, k_ref, v_ref = dr.qkv_rope_cache_ref(c["qkv"], c["cs"], [pos], row, Hq, Hkv, ROWS, c["ov"] if override else None)
        assert_bits(q[:-PAD].view(1, Hq, 128), q_ref, what + " q")
        assert bool((q[-PAD:] == SENT).all()), what + ": written past q"
        assert_bits(k, k_ref, what + " k cache")           # (every other row keeps its NaN sentinel)
        assert_bits(v, v_ref, what + " v cache")
        if norm:
            check_h(h, n, what)
        else:
            assert bool((h == SENT).all())


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("cfg", ["neox_kv8", "glm_kv4_bias"])
def test_q_launch_and_kv_role_exact(cfg, placement):
    """skv_q_gemv_rope + the k/v role of the selection launches (skv_kvproj.h), both placements, against the same reference."""
    from shadowkv_amd import _lib, tensor_op
    Hq, Hkv, glm = 32, 8 if cfg == "neox_kv8" else 4, cfg != "neox_kv8"
    c = qkv_case(Hq, Hkv, glm, glm, 4096, True, seed=31 + Hkv)
    n = c["n"]
    lm, idx, cached, S = select_inputs(Hkv, 520, seed=3)
    for pos, row, override in QKV_VARIANTS:
        what = f"{cfg} {placement} pos {pos} row {row} override {override}"
        k, v = nan_caches(1, Hkv)
        row_d, pos_d = torch.tensor([row], device=DEV), torch.tensor([[pos]], device=DEV)
        h, q, desc = tensor_op.norm_q_rope(n["x_d"].view(1, 1, 4096), n["res_d"].view(1, 1, 4096), n["w_d"], 1e-5, c["w"], c["bias_d"],
                                           c["cs_d"], pos_d, row_d, k, v, Hq, Hkv, q_override=c["ov"].to(DEV) if override else None,
                                           placement=PLACEMENTS[placement])
        torch.cuda.synchronize()
        q_ref, k_ref, v_ref = dr.qkv_rope_cache_ref(c["qkv"], c["cs"], [pos], row, Hq, Hkv, ROWS, c["ov"] if override else None)
        assert_bits(q.view(1, Hq, 128), q_ref, what + " q")
        assert_bits(h.view(-1), dr.to_bf16(n["h"]), what + " h")
        assert bool(torch.isnan(k.float()).all()) and bool(torch.isnan(v.float()).all()), what + ": the q launch touched the caches"
        run_selection(_lib.lib(), q, lm, idx, cached, S, desc)
        assert_bits(k, k_ref, what + " k cache")
        assert_bits(v, v_ref, what + " v cache")


@pytest.mark.parametrize("bs", [1, 3])
@pytest.mark.parametrize("glm", [False, True], ids=["neox", "glm"])
def test_qkv_rope_update_standalone_exact(glm, bs):
    """skv_qkv_rope_update on random bf16 projections: bit-exact against the one-rounding-per-operation restatement."""
    _lib, L, st = _L()
    p = _lib.ptr
    Hq, Hkv = 8, 2
    g = torch.Generator().manual_seed(50 + bs + glm)
    qkv = (torch.randn(bs, (Hq + 2 * Hkv) * 128, generator=g) * 2).bfloat16()
    cs = cos_sin_table(glm, seed=60 + glm)
    ov = torch.randn(bs, Hq, 128, generator=g).bfloat16()
    qkv_d, cs_d, ov_d = qkv.to(DEV), cs.to(DEV), ov.to(DEV)
    variants = [([17, -3, CS_ROWS + 2], 5, False), ([-1, CS_ROWS, 0], 0, False), ([CS_ROWS - 1, 3, -9], ROWS - 1, False),
                ([9, 8, 7], -1, False), ([9, 8, 7], ROWS, False), ([21, 0, 39], 7, True)]
    for pos, row, override in variants:
        pos = pos[:bs]
        what = f"glm {glm} bs {bs} pos {pos} row {row} override {override}"
        k, v = nan_caches(bs, Hkv)
        q = sentinel_buf(bs * Hq * 128 + PAD)
        pos_d, row_d = torch.tensor(pos, device=DEV), torch.tensor([row], device=DEV)
        rc = L.skv_qkv_rope_update(p(qkv_d), p(cs_d), p(pos_d), p(row_d), p(ov_d) if override else 0, p(q), p(k), p(v), bs, Hq, Hkv,
                                   128, cs_d.stride(0), CS_ROWS, k.stride(0), k.stride(1), ROWS, 2 if glm else 1, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        q_ref, k_ref, v_ref = dr.qkv_rope_cache_ref(qkv, cs, pos, row, Hq, Hkv, ROWS, ov if override else None)
        assert_bits(q[:-PAD].view(bs, Hq, 128), q_ref, what + " q")
        assert bool((q[-PAD:] == SENT).all()), what + ": written past q"
        assert_bits(k, k_ref, what + " k cache")
        assert_bits(v, v_ref, what + " v cache")
        if glm and not override:     # pass-through dims: the input's bits
            assert_bits(q[:-PAD].view(bs, Hq, 128)[..., 64:], qkv.view(bs, -1, 128)[:, :Hq, 64:], what + " q pass-through")
            if 0 <= row < ROWS:
                assert_bits(k[:, :, row, 64:], qkv.view(bs, -1, 128)[:, Hq:Hq + Hkv, 64:], what + " k pass-through")


# ------------------------------------------------------------------------------------------- add_rmsnorm, silu_and_mul
def run_add_rmsnorm(x, res, w, eps):
    """x, res [rows, hidden] (res may be None), w [hidden] on the device -> (h | None, y), sentinel row checked."""
    _lib, L, st = _L()
    p = _lib.ptr
    rows, hidden = x.shape
    y = sentinel_buf(rows + 1, hidden)
    h = sentinel_buf(rows + 1, hidden) if res is not None else None
    rc = L.skv_add_rmsnorm(p(x), p(res), p(w), p(h), p(y), rows, hidden, eps, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((y[rows] == SENT).all()) and (h is None or bool((h[rows] == SENT).all())), "written past the last row"
    return (h[:rows] if h is not None else None), y[:rows]


def assert_norm(y, ref, what):
    err, tol = (y.cpu().double() - ref).abs(), dr.NORM_RTOL * ref.abs()
    print(f"{what}: worst |err| / bound {float((err / tol.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} values over 2^-8 |ref|"


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("hidden", [8, 520, 2048, 2056, 4096, 8192])
def test_add_rmsnorm(hidden, rows):
    g = torch.Generator().manual_seed(hidden + rows)
    # exact probe: |h| = 2 everywhere -> y = sign(h) * w_norm bit for bit, h one bf16 add
    ns = [dr.norm_inputs(hidden, seed=hidden + r, residual=True) for r in range(rows)]
    w = ns[0]["w_norm"]
    x, res = torch.stack([n["x"] for n in ns]), torch.stack([n["residual"] for n in ns])
    for eps in (0.0, 1e-5):
        h, y = run_add_rmsnorm(dev16(x), dev16(res), dev16(w), eps)
        assert_bits(h, dr.to_bf16(x + res), f"add_rmsnorm hidden {hidden} h")
        assert_bits(y, dr.to_bf16(torch.stack([(n["h"] // 2) * w for n in ns])), f"add_rmsnorm hidden {hidden} eps {eps} y")
    # random data: h bit-exact, y within 2^-8 |ref| of the f64 norm
    xr, rr = torch.randn(rows, hidden, generator=g).bfloat16(), torch.randn(rows, hidden, generator=g).bfloat16()
    wr = (1 + 0.1 * torch.randn(hidden, generator=g)).bfloat16()
    for res_r in (rr, None):
        h, y = run_add_rmsnorm(xr.to(DEV), res_r.to(DEV) if res_r is not None else None, wr.to(DEV), 1e-5)
        href = dr.add_ref(xr, res_r)
        if res_r is not None:
            assert_bits(h, href, f"add_rmsnorm hidden {hidden} random h")
        assert_norm(y, dr.rmsnorm_ref(href, wr, 1e-5), f"add_rmsnorm hidden {hidden} rows {rows} residual {res_r is not None}")


def test_add_rmsnorm_refuses_hidden_8200():
    _lib, L, st = _L()
    x = torch.zeros(1, 8200, dtype=torch.bfloat16, device=DEV)
    y = sentinel_buf(1, 8200)
    assert L.skv_add_rmsnorm(_lib.ptr(x), 0, _lib.ptr(x), 0, _lib.ptr(y), 1, 8200, 1e-5, st) == -2
    torch.cuda.synchronize()
    assert bool((y == SENT).all())


def spike_positions(hidden):
    return sorted({p for p in (0, 7, 8, 2047, 2048, hidden - 8, hidden - 1) if 0 <= p < hidden})


def spiked_rows(hidden, seed):
    """N(0, 1) rows, row i with h[spike i] = 64 (x = 64, residual = 0 there): the first and last elements of the per-thread
    16-byte vectors.  The spike is 4096 / hidden of the mean square of the rest: dropping it moves rstd by ~30 % at 4096."""
    g = torch.Generator().manual_seed(seed)
    sp = spike_positions(hidden)
    x = torch.randn(len(sp), hidden, generator=g).bfloat16()
    res = (0.5 * torch.randn(len(sp), hidden, generator=g)).bfloat16()
    for i, p in enumerate(sp):
        x[i, p], res[i, p] = 64.0, 0.0
    w = (1 + 0.1 * torch.randn(hidden, generator=g)).bfloat16()
    return sp, x, res, w


@pytest.mark.parametrize("hidden", [8, 520, 2048, 2056, 4096, 8192])
def test_add_rmsnorm_statistics_see_every_element(hidden):
    sp, x, res, w = spiked_rows(hidden, seed=hidden)
    h, y = run_add_rmsnorm(x.to(DEV), res.to(DEV), w.to(DEV), 1e-5)
    href = dr.add_ref(x, res)
    assert_bits(h, href, f"spiked rows hidden {hidden} h")
    assert all(float(href[i, p]) == 64.0 for i, p in enumerate(sp))
    assert_norm(y, dr.rmsnorm_ref(href, w, 1e-5), f"spiked rows hidden {hidden}")


def test_norm_gemv_statistics_see_every_element():
    """The same spiked rows through the norm prologue of skv_norm_gemv_bf16: one nonzero (1.0) per weight row reads xn back."""
    _lib, L, st = _L()
    p = _lib.ptr
    K = 4096
    sp, x, res, w = spiked_rows(K, seed=K)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(12))
    W = torch.zeros(K, K, dtype=torch.bfloat16, device=DEV)
    W[torch.arange(K), perm.to(DEV)] = 1.0
    wd, xd, rd = w.to(DEV), x.to(DEV), res.to(DEV)
    for i in range(len(sp)):
        y, h = sentinel_buf(K + PAD), sentinel_buf(K + PAD)
        rc = L.skv_norm_gemv_bf16(p(W), p(xd[i]), p(rd[i]), p(wd), 1e-5, p(h), 0, p(y), K, K, 0, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        href = dr.add_ref(x[i], res[i])
        assert_bits(h[:K], href, f"norm gemv spike {sp[i]} h")
        assert bool((y[K:] == SENT).all()) and bool((h[K:] == SENT).all())
        assert_norm(y[:K], dr.rmsnorm_ref(href, w, 1e-5)[perm], f"norm gemv spike at {sp[i]}")


# (300 x 14336: 537,600 vectors of 8 - the grid is capped at 2,048 workgroups x 256 vectors, so the grid-stride loop repeats)
@pytest.mark.parametrize("I,rows", [(I, rows) for rows in (1, 3) for I in (8, 1000, 13696, 14336)] + [(14336, 300)])
def test_silu_and_mul(I, rows):
    _lib, L, st = _L()
    g = torch.Generator().manual_seed(I + rows)
    gate = (3 * torch.randn(rows, I, generator=g)).bfloat16()
    up = torch.randn(rows, I, generator=g).bfloat16()
    special = torch.tensor([0.0, 60.0, -60.0, 2.0 ** -126, -2.0 ** -126, 2.0 ** -120, 2.0 ** -130, -2.0 ** -130]).bfloat16()
    uspec = torch.tensor([3.0, 1.5, -2.0, 1.0, 2.0, -0.5, 2.0, 4.0]).bfloat16()
    gate[:, -8:], up[:, -8:] = special.flip(0), uspec.flip(0)
    gate[:, :8], up[:, :8] = special, uspec   # 0, +-large, the smallest normal, bf16 subnormals (silu = g / 2, exact)
    xin = torch.cat((gate, up), -1).to(DEV)
    out = sentinel_buf(rows + 1, I)
    rc = L.skv_silu_and_mul(_lib.ptr(xin), _lib.ptr(out), rows, I, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((out[rows] == SENT).all())
    ref = dr.silu_mul_ref(gate, up)
    assert bool((ref[:, 0] == 0).all()) and bool((ref[:, 1:8] != 0).all())
    assert_silu(out[:rows], ref, f"silu_and_mul I {I} rows {rows}")


# ------------------------------------------------------------------------------------------------------------ rows GEMM
ROWS_M = (2, 8, 9, 16, 17, 32)
ROWS_K = (32, 96, 288, 1056, 8224)
ROWS_N = (48, 2 * 1003, 6160, 16400)          # 2 * 1003: the SiLU pair form


def test_rows_gemm_shapes_reach_every_branch():
    reached = {expected_branch(M, N, K) for M in ROWS_M for N in ROWS_N for K in ROWS_K}
    assert reached == {"g1 paired", "g2 1/2x8", "g1", "g2 2/4x4", "g2 2/2x8", "g2 2/1x8", "g1 two tiles"}
    assert len(reached) == 7                                               # the seven return statements of skv_rows_pick
    assert expected_branch(17, 48, 8224) == "g2 2/1x8" and expected_branch(17, 48, 1056) == "g1 two tiles"
    assert expected_branch(16, 6160, 32) == "g2 1/2x8" and expected_branch(32, 16400, 32) == "g2 2/4x4"


def run_rows(bank, w, x, bias, silu, M):
    _lib, L, st = _L()
    p = _lib.ptr
    N, K = bank.rows, bank.K
    No = N // 2 if silu else N
    y = sentinel_buf(bank.launches, M + 1, No)
    for l in range(bank.launches):
        rc = L.skv_linear_rows_bf16(p(w[l * N:(l + 1) * N]), p(x), p(bias), p(y[l]), M, N, K, int(silu), st)
        assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((y[:, M] == SENT).all()), "the row past M was written"
    return y[:, :M]


@pytest.mark.parametrize("K", ROWS_K)
@pytest.mark.parametrize("N", ROWS_N)
def test_rows_gemm_exact(N, K):
    """skv_linear_rows_bf16 at every M of ROWS_M: K / 32 = 1, 3, 9 (fewer k-steps than the 8 split-K waves, or barely more),
    33 (single steps only in the first generation), 257 (unrolled batches + a tail); ragged N (48, 6160 = 385 tiles, 1003)."""
    silu = N == 2 * 1003
    xi, colsign = dr.structured_x(max(ROWS_M), K, seed=N + K)
    bank = dr.pair_bank(N // 2, K, seed=N + K, colsign=colsign) if silu else dr.plain_bank(N, K, seed=N + K)
    w = weights_on_device(bank)
    x_d = dev16(xi)
    for M in ROWS_M:
        what = f"rows gemm M {M} N {N} K {K} [{expected_branch(M, N, K)}]"
        xm = x_d[:M].contiguous()
        if silu:
            g, u, ref = dr.pair_ref(bank, xi[:M])
            assert bool((g != 0).all()) and bool((u != 0).all())
            y = run_rows(bank, w, xm, None, True, M)
            assert_silu(y.permute(1, 0, 2), ref, what)
        else:
            for bias in (None, dr.integer_bias(N, seed=N + M)):
                y = run_rows(bank, w, xm, None if bias is None else dev16(bias), False, M)
                assert_bits(y.permute(1, 0, 2), dr.gemv_ref(bank, xi[:M], bias), what + f" bias {bias is not None}")


# ------------------------------------------------------------------------------------------------ random-data companion
# Share of outputs whose bf16 result differs from bf16(f64), for two plain CPU f32 evaluations of the same dot products
# (sequential k order, pairwise tree), measured from dense_ref alone (profiles/dense_exact_flip_shares.txt;
# tests/test_dense_ref_cpu.py recomputes the rows-GEMM pair).  The kernels' order - per-lane chains, a DPP tree, split-K
# partials - is neither of the two, hence the factor 4 on the larger share.
GEMV_CPU_SHARES = (2 / 4101, 0 / 4101)            # (sequential, pairwise) at (N, K) = (4101, 13696): 2 and 0 of 4,101 outputs
ROWS_CPU_SHARES = (6 / 104720, 3 / 104720)        # (sequential, pairwise) at (M, N, K) = (17, 6160, 1056): 6 and 3 of 104,720
GEMV_SHARE_BOUND = 4 * max(GEMV_CPU_SHARES)
ROWS_SHARE_BOUND = 4 * max(ROWS_CPU_SHARES)


def check_random(y, s64, bias, bound, what):
    want = dr.finish64(s64, bias).bfloat16()
    d = util.ulp_diff_bf16(y.cpu(), want)
    share = float((d > 0).double().mean())
    print(f"{what}: values {d.numel()}  differing {int((d > 0).sum())} (share {share:.3e}, bound {bound:.3e})  max ulp {int(d.max())}")
    assert int(d.max()) <= 1, f"{what}: an output is {int(d.max())} bf16 ulps from bf16(f64)"
    assert share <= bound, f"{what}: share of outputs that differ from bf16(f64) {share:.3e} > {bound:.3e}"


def test_gemv_random_data_within_one_ulp():
    _lib, L, st = _L()
    c = dr.RANDOM_GEMV
    w, x, bias, s64 = dr.random_case(**c)
    y = sentinel_buf(c["N"] + PAD)
    wd, xd, bd = w.to(DEV), x.to(DEV), bias.to(DEV)
    rc = L.skv_gemv_bf16(_lib.ptr(wd), _lib.ptr(xd), _lib.ptr(bd), _lib.ptr(y), c["N"], c["K"], 0, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((y[c["N"]:] == SENT).all())
    check_random(y[:c["N"]].view(1, -1), s64, bias, GEMV_SHARE_BOUND, "gemv random data")


def test_rows_gemm_random_data_within_one_ulp():
    _lib, L, st = _L()
    c = dr.RANDOM_ROWS
    w, x, bias, s64 = dr.random_case(**c)
    y = sentinel_buf(c["M"] + 1, c["N"])
    wd, xd, bd = w.to(DEV), x.to(DEV), bias.to(DEV)
    rc = L.skv_linear_rows_bf16(_lib.ptr(wd), _lib.ptr(xd), _lib.ptr(bd), _lib.ptr(y), c["M"], c["N"], c["K"], 0, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((y[c["M"]] == SENT).all())
    check_random(y[:c["M"]], s64, bias, ROWS_SHARE_BOUND, "rows gemm random data")
