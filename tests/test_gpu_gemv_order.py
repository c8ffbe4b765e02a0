"""GPU: the decode GEMV's bits against the host restatement of its summation order (tests/gemv_order_ref.py) on Gaussian
data.  The integer banks of the exact tests give one sum in every order, so a loop that multiplies its k-steps in another
order passes them; here every odd weight row cancels exactly and returns the rounding residue of its f32 chains, which any
change of order replaces by another number (tests/test_gemv_order_ref_cpu.py shows it on these very inputs).  Raw bits, no
tolerance; sentinels past every output."""
import pytest
import torch

import dense_ref as dr
import gemv_order_ref as go
from test_gpu_dense_exact import PAD, SENT, assert_bits, sentinel_buf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5


def _L():
    from shadowkv_amd import _lib
    return _lib.lib(), _lib.ptr, _lib.current_stream_handle()


@pytest.mark.parametrize("N,K,seed", go.PLAIN_CASES)
def test_gemv_plain_order(N, K, seed):
    L, p, st = _L()
    w, x, bias = go.gaussian(N, K, seed)
    wd, xd, bd = w.to(DEV), x.to(DEV), bias.to(DEV)
    for b, b_d in ((None, None), (bias, bd)):
        y = sentinel_buf(N + PAD)
        assert L.skv_gemv_bf16(p(wd), p(xd), p(b_d), p(y), N, K, 0, st) == 0
        torch.cuda.synchronize()
        assert_bits(y[:N], go.restate(w, x, b), f"gemv N {N} K {K} bias {b is not None}")
        assert bool((y[N:] == SENT).all()), "written past N"


def test_norm_gemv_plain_order():
    L, p, st = _L()
    c = go.norm_case()
    N, K, n = c["N"], c["K"], c["n"]
    wd, bd = c["w"].to(DEV), c["bias"].to(DEV)
    xd, rd, gd = n["x"].to(DEV), n["residual"].to(DEV), n["w_norm"].to(DEV)
    for b, b_d in ((None, None), (c["bias"], bd)):
        y, h = sentinel_buf(N + PAD), sentinel_buf(K + PAD)
        assert L.skv_norm_gemv_bf16(p(wd), p(xd), p(rd), p(gd), EPS, p(h), p(b_d), p(y), N, K, 0, st) == 0
        torch.cuda.synchronize()
        assert_bits(h[:K], n["h"], "h_out")
        assert_bits(y[:N], go.restate(c["w"], c["xn"], b), f"norm gemv N {N} bias {b is not None}")
        assert bool((y[N:] == SENT).all()) and bool((h[K:] == SENT).all()), "written past an output"


@pytest.mark.parametrize("override", [False, True], ids=["rotated", "override"])
@pytest.mark.parametrize("glm", [False, True], ids=["neox", "glm"])
def test_q_launch_order(glm, override):
    """skv_q_gemv_rope, one KV group: the restated totals of the q rows, then dense_ref's rotation (bf16 arithmetic, one
    rounding per operation) at the token's position, or the q_override bits.  No bias: it would bury the residues."""
    L, p, st = _L()
    c = go.q_case(glm)
    Hq, Hkv, K, n = c["Hq"], c["Hkv"], c["K"], c["n"]
    Nq, pos = Hq * 128, 17
    qkv = torch.zeros(1, (Hq + 2 * Hkv) * 128, dtype=torch.bfloat16)          # (the k / v rows belong to another launch)
    qkv[0, :Nq] = go.restate(c["w"][:Nq], c["xn"])
    q_ref, _, _ = dr.qkv_rope_cache_ref(qkv, c["cs"], [pos], -1, Hq, Hkv, 1, c["ov"] if override else None)
    wd, csd, ovd = c["w"].to(DEV), c["cs"].to(DEV), c["ov"].to(DEV)
    xd, rd, gd = n["x"].to(DEV), n["residual"].to(DEV), n["w_norm"].to(DEV)
    pos_d = torch.tensor([pos], device=DEV)
    q, h = sentinel_buf(Nq + PAD), sentinel_buf(K + PAD)
    rc = L.skv_q_gemv_rope(p(wd), p(xd), p(rd), p(gd), EPS, p(h), 0, p(csd), p(pos_d), p(ovd) if override else 0, p(q), K, Hq,
                           Hkv, 128, csd.stride(0), csd.shape[0], 2 if glm else 1, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert_bits(h[:K], n["h"], "h_out")
    assert_bits(q[:Nq].view(1, Hq, 128), q_ref, f"q glm {glm} override {override}")
    assert bool((q[Nq:] == SENT).all()) and bool((h[K:] == SENT).all()), "written past an output"
