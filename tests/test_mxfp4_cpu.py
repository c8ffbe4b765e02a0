"""CPU: the weight-only MXFP4 path without a GPU - the block quantiser / dequantiser (tensor_op) over every finite bf16
pattern and against the independent restatement of tests/mxfp4_ref.py, the host-side argument checks of every MXFP4 export
(they run before any HIP call), the ValueErrors of the host paths, DecoderLM's weight_dtype handling and byte accounting."""
import numpy as np
import pytest
import torch

import mxfp4_ref as mr


def _q():
    from shadowkv_amd import tensor_op
    return tensor_op


def all_finite_bf16():
    """bf16 [65280]: every finite bit pattern (both zeros and the subnormals included)"""
    b = torch.arange(65536, dtype=torch.int32)
    b = b[(b & 0x7F80) != 0x7F80]
    assert b.numel() == 65280
    return b.to(torch.int16).view(torch.bfloat16)


def blocks_of_all_patterns():
    """[4080, 32] bf16: every finite pattern once; a block holds 16 consecutive magnitudes of one binade-neighbourhood with
    both signs, so within a block the ratios to the block maximum stay close to 1 and every pattern is quantised on a fine
    scale - and a second arrangement (column-major) mixes magnitudes 2^8 apart in one block, where small ones round to 0."""
    v = all_finite_bf16()
    pos, neg = v[:32640], v[32640:]
    near = torch.stack((pos.view(-1, 16), neg.view(-1, 16)), dim=-1).reshape(-1, 32)
    mixed = v.view(32, -1).t().contiguous()
    return torch.cat((near, mixed))


# ------------------------------------------------------------------------------------------------------------ quantiser
def test_quantiser_properties_over_every_finite_bf16_pattern():
    t = _q()
    w = blocks_of_all_patterns()
    N = w.shape[0]
    w4, sc = t.quantize_mxfp4_rows(w)
    assert w4.dtype == torch.uint8 and w4.shape == (N, 16) and sc.dtype == torch.uint8 and sc.shape == (N, 1)
    assert int(sc.min()) >= 27 and int(sc.max()) <= 227
    s = sc.double().view(N) - 127
    amax = w.double().abs().amax(dim=1)
    two_s = torch.exp2(s)
    # the scale rule: the smallest power of two with amax / 2^s <= 6, clamped; an all-zero block: s = 0
    free = (amax > 0) & (s > -100) & (s < 100)
    assert bool((amax[free] <= 6 * two_s[free]).all()) and bool((amax[free] > 3 * two_s[free]).all())
    assert bool((s[amax == 0] == 0).all())
    low = (amax > 0) & (s == -100)
    assert bool((amax[low] <= 6 * two_s[low]).all())                  # clamped from below: still nothing clipped
    high = s == 100
    assert bool(high.any()) and bool((amax[high] > 3 * two_s[high]).all())      # clamped from above (bf16 reaches 2^127)
    # the element error, in units of the block scale: <= 0.25 up to 2, <= 0.5 in [2, 4], <= 1 in [4, 6]
    back = t.dequantize_mxfp4_rows(w4, sc, dtype=torch.float32).double()
    a = w.double().abs() / two_s.view(N, 1)
    err = (back - w.double()).abs() / two_s.view(N, 1)
    ok = ~high.view(N, 1).expand_as(a)
    assert bool((err[ok & (a <= 2)] <= 0.25).all())
    assert bool((err[ok & (a > 2) & (a <= 4)] <= 0.5).all())
    assert bool((err[ok & (a > 4)] <= 1.0).all()) and bool((a[ok] <= 6).all())
    assert bool((back[~ok].abs() <= 6 * two_s.view(N, 1).expand_as(a)[~ok]).all())
    # signs are kept, and the dequantised values are bf16 numbers
    assert bool(((back == 0) | (torch.sign(back) == torch.sign(w.double()))).all())
    b16 = t.dequantize_mxfp4_rows(w4, sc)
    assert b16.dtype == torch.bfloat16 and torch.equal(b16.double(), back)
    # agreement with the independent restatement, byte for byte
    r4, rs = mr.quantize(w)
    assert np.array_equal(w4.numpy(), r4) and np.array_equal(sc.numpy(), rs)
    assert np.array_equal(back.numpy(), mr.decode(w4, sc))
    # idempotent on grid values (as values: a negative element that rounded to -0 comes back as +0)
    a4, asc = t.quantize_mxfp4_rows(b16)
    assert torch.equal(t.dequantize_mxfp4_rows(a4, asc), b16)


def test_ties_go_to_the_even_mantissa_and_nibble_order():
    t = _q()
    w = torch.zeros(2, 32)
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    w[0, :7] = torch.tensor(ties)
    w[0, 7] = 6.0                                  # block maximum 6: s = 0
    w[1, :7] = -torch.tensor(ties) * 8
    w[1, 7] = -48.0                                # s = 3
    w4, sc = t.quantize_mxfp4_rows(w.bfloat16())
    assert sc.view(-1).tolist() == [127, 130]
    back = t.dequantize_mxfp4_rows(w4, sc, dtype=torch.float32)
    assert back[0, :8].tolist() == want + [6.0] and back[1, :8].tolist() == [-8 * v for v in want] + [-48.0]
    # element 2i in the low nibble of byte i, element 2i + 1 in the high nibble; code 0..7 <-> E2M1, bit 3 the sign
    assert int(w4[0, 0]) == (0 | (2 << 4)) and int(w4[0, 1]) == (2 | (4 << 4)) and int(w4[0, 3]) == (6 | (7 << 4))
    assert int(w4[1, 3]) == ((8 | 6) | ((8 | 7) << 4))
    one = torch.zeros(1, 32)
    one[0, 5] = 1.5
    b4, bs = t.quantize_mxfp4_rows(one)
    assert int(bs) == 125 and b4.view(-1).tolist() == [0, 0, 7 << 4] + [0] * 13          # 1.5 = 6 * 2^-2, element 5 = byte 2 high


def test_zero_tiny_and_huge_blocks():
    t = _q()
    w = torch.zeros(1, 128)
    w[0, 32:64] = 1e-30
    w[0, 64:96] = 3e38
    w[0, 96] = 1e-38                               # below what s = -100 can represent: rounds towards 0
    w4, sc = t.quantize_mxfp4_rows(w)
    assert sc.view(-1).tolist() == [127, 27, 227, 27]
    back = t.dequantize_mxfp4_rows(w4, sc, dtype=torch.float32)
    assert bool((w4[0, :16] == 0).all()) and bool((back[0, :32] == 0).all())
    assert bool(((back[0, 32:64].double() - 1e-30).abs() <= 0.25 * 2.0 ** -100).all())
    assert bool((back[0, 64:96] == 6 * 2.0 ** 100).all())             # the clamped scale saturates at its largest value
    assert bool((back[0, 96:] == 0).all())
    assert not bool((sc == 0xFF).any())


def test_quantiser_agrees_with_the_restatement_on_gaussian_rows():
    t = _q()
    g = torch.Generator().manual_seed(4)
    w = (torch.randn(37, 2080, generator=g) * torch.logspace(-4, 3, 37).unsqueeze(1)).bfloat16()
    w[3, 64:96] = 0
    w4, sc = t.quantize_mxfp4_rows(w)
    r4, rs = mr.quantize(w)
    assert np.array_equal(w4.numpy(), r4) and np.array_equal(sc.numpy(), rs)
    deq = t.dequantize_mxfp4_rows(w4, sc)
    assert np.array_equal(deq.double().numpy(), mr.decode(w4, sc))
    # relative error of a Gaussian row: e2m1 keeps one mantissa bit
    rel = float((deq.double() - w.double()).norm() / w.double().norm())
    assert rel < 0.2, rel
    with pytest.raises(ValueError):
        t.quantize_mxfp4_rows(torch.zeros(4, 1040))        # K % 32 != 0
    with pytest.raises(ValueError):
        t.quantize_mxfp4_rows(torch.zeros(1024))


# --------------------------------------------------------------------------------------------------------- host paths
def test_decode_ops_refuse_inconsistent_mxfp4_pairs():
    t = _q()
    w4, sc = t.quantize_mxfp4_rows(torch.ones(4, 1024))
    x = torch.ones(1, 1, 1024, dtype=torch.bfloat16)
    kc = torch.zeros(1, 1, 8, 128)
    bad = [(w4, None), (w4, sc[:3]), (w4, sc[:, :31]), (w4, sc.float()), (w4, torch.ones(4)), (w4[:, :500], sc)]
    for w, s in bad:
        with pytest.raises(ValueError, match=r"K / 32"):
            t.linear_decode(x, w, w_scale=s)
        with pytest.raises(ValueError, match=r"K / 32"):
            t.norm_linear_decode(x, None, x.view(-1), 1e-5, w, w_scale=s)
        with pytest.raises(ValueError, match=r"K / 32"):
            t.norm_qkv_rope_update(x, None, x.view(-1), 1e-5, w, None, x, x, x, kc, kc, 1, 1, w_scale=s)
    with pytest.raises(ValueError, match=r"K / 2"):
        t.linear_decode(torch.ones(1, 1, 2048, dtype=torch.bfloat16), w4, w_scale=sc)          # x does not match K
    with pytest.raises(ValueError):
        t.linear_decode(x, torch.ones(4, 1024, dtype=torch.bfloat16), w_scale=sc)              # bf16 weights with scale bytes
    with pytest.raises(ValueError):
        t.dequantize_mxfp4_rows(w4, sc[:2])
    assert t.kv_proj_split_supported(x, w4, kc) is False
    with pytest.raises(ValueError, match="MXFP4"):
        t.norm_q_rope(x, None, x, 1e-5, w4, None, x, x, x, kc, kc, 1, 1)
    assert t.mxfp4_native_calls == 0 or isinstance(t.mxfp4_native_calls, int)
    assert isinstance(t.mxfp4_fallback_calls, int)


def test_multi_row_fallback_on_the_cpu_is_the_dequantised_linear():
    t = _q()
    g = torch.Generator().manual_seed(8)
    w = (torch.randn(12, 1024, generator=g) * 0.05).bfloat16()
    w4, sc = t.quantize_mxfp4_rows(w)
    x = torch.randn(3, 1, 1024, generator=g).bfloat16()
    f0, n0 = t.mxfp4_fallback_calls, t.mxfp4_native_calls
    y = t.linear_decode(x, w4, w_scale=sc, fp8_rows="native")          # fp8_rows does not apply to MXFP4 weights
    assert t.mxfp4_fallback_calls == f0 + 1 and t.mxfp4_native_calls == n0
    assert torch.equal(y, torch.nn.functional.linear(x, t.dequantize_mxfp4_rows(w4, sc)))


# ------------------------------------------------------------------------------------------------ host-side argument checks
P = 0x1000            # a non-null pointer that is never dereferenced on the host
NEAR = (P, 8, 4, 1000, 2000, 64, P, 8 * 2000 * 1024, 1)      # early state, blocks, groups, landmarks, chunks, E, V table, stride, parts
EXPORTS = ("skv_gemv_mxfp4", "skv_norm_gemv_mxfp4", "skv_norm_gemv_rangemax_mxfp4", "skv_qkv_gemv_rope_update_mxfp4",
           "skv_norm_gemv_near_pull_mxfp4", "skv_gemv_near_pull_mxfp4")


def test_the_exports_exist_and_the_abi_version_stays():
    from shadowkv_amd import _lib
    L = _lib.lib()
    for name in EXPORTS:
        assert callable(getattr(L, name)), name
    assert L.skv_abi_version() == 1


def _entries(fmt):
    """name -> call(W, scale, x, y, N, K): every export of the format with otherwise valid arguments."""
    from shadowkv_amd import _lib
    L = _lib.lib()

    def f(name):
        return getattr(L, name.format(fmt))
    ct = (P, P, P, 0)          # cos_sin, pos, row_idx, q_override
    return {
        "gemv": lambda W, s, x, y, N, K: f("skv_gemv_{}")(W, s, x, 0, y, N, K, 0, 0),
        "gemv_silu": lambda W, s, x, y, N, K: f("skv_gemv_{}")(W, s, x, 0, y, N, K, 1, 0),
        "norm": lambda W, s, x, y, N, K: f("skv_norm_gemv_{}")(W, s, x, 0, P, 1e-5, 0, 0, y, N, K, 0, 0),
        "rangemax": lambda W, s, x, y, N, K: f("skv_norm_gemv_rangemax_{}")(W, s, x, 0, P, 1e-5, 0, 0, y, N, K, P, 0),
        "near_gate_up": lambda W, s, x, y, N, K: f("skv_norm_gemv_near_pull_{}")(W, s, x, 0, P, 1e-5, 0, y, N, K, *NEAR, 1, 0),
        "near_down": lambda W, s, x, y, N, K: f("skv_gemv_near_pull_{}")(W, s, x, 0, y, N, K, *NEAR, 1, 0),
        # (N is (q_heads + 2 kv_heads) * 128 there: q_heads = N / 128 - 2, one KV head; y: q_out)
        "qkv": lambda W, s, x, y, N, K: f("skv_qkv_gemv_rope_update_{}")(W, s, x, 0, P, 1e-5, 0, 0, *ct, y, P, P, K, N // 128 - 2, 1,
                                                                         128, 128, 64, 8 * 128, 8, 1, 0),
    }


NORM_ENTRIES = ("norm", "rangemax", "near_gate_up", "qkv")
NAMES = ["gemv", "gemv_silu", "norm", "rangemax", "near_gate_up", "near_down", "qkv"]


@pytest.mark.parametrize("name", NAMES)
def test_mxfp4_entries_refuse_bad_arguments_before_any_launch(name):
    """-1 (SKV_ERR_ARG) for a missing pointer or N < 1; -2 (SKV_ERR_UNSUPPORTED) for K % 32 != 0, K below 1024 and, norm
    variants, K != 4096.  No GPU is present: a call that reached the HIP runtime could not return these codes.  Wherever the
    FP8 entry of the same name refuses the same arguments, both return the same code."""
    call, fp8 = _entries("mxfp4")[name], _entries("fp8")[name]
    N, K = 512, 4096
    for W, s, x, y in ((0, P, P, P), (P, 0, P, P), (P, P, 0, P), (P, P, P, 0), (0, 0, 0, 0)):
        assert call(W, s, x, y, N, K) == -1 == fp8(W, s, x, y, N, K), (name, W, s, x, y)
        assert call(W, s, x, y, N, 4104) == -1 == fp8(W, s, x, y, N, 4104)           # pointers before K
    if name != "qkv":
        assert call(P, P, P, P, 0, K) == -1 and call(P, P, P, P, -16, K) == -1
        assert fp8(P, P, P, P, 0, K) == -1
    else:
        assert call(P, P, P, P, 2 * 128, K) == -1 == fp8(P, P, P, P, 2 * 128, K)    # no query head
    for bad_k in (4104, 4112, 512, 992, 1016, 0):                                    # K % 32 != 0 (4112: fine for FP8), K < 1024
        assert call(P, P, P, P, N, bad_k) == -2, bad_k
    for bad_k in (4104, 512, 1016):
        assert fp8(P, P, P, P, N, bad_k) == -2
    if name in NORM_ENTRIES:
        for bad_k in (1024, 2048, 8192):                                             # the norm prologue: K == 4096
            assert call(P, P, P, P, N, bad_k) == -2 == fp8(P, P, P, P, N, bad_k)


@pytest.mark.parametrize("fmt", ["mxfp4", "fp8"])
def test_entry_specific_checks_match_the_fp8_entries(fmt):
    from shadowkv_amd import _lib
    L = _lib.lib()

    def f(name):
        return getattr(L, name.format(fmt))
    assert f("skv_norm_gemv_rangemax_{}")(P, P, P, 0, P, 1e-5, 0, 0, P, 4104, 4096, P, 0) == -2       # N % 16 != 0
    assert f("skv_norm_gemv_rangemax_{}")(P, P, P, 0, P, 1e-5, 0, 0, P, 4096, 4096, 0, 0) == -1       # no keys buffer
    assert f("skv_norm_gemv_rangemax_{}")(P, P, P, 0, P, 1e-5, 0, 0, P, 4096, 4104, 0, 0) == -1       # the keys buffer is checked first
    assert f("skv_norm_gemv_{}")(P, P, P, 0, 0, 1e-5, 0, 0, P, 512, 4096, 0, 0) == -2                 # norm without a norm weight
    assert f("skv_norm_gemv_{}")(0, P, P, 0, 0, 1e-5, 0, 0, P, 512, 4096, 0, 0) == -1
    assert f("skv_gemv_{}")(P, P, P, 0, P, 513, 4096, 1, 0) == -1                                     # odd [gate; up] rows
    assert f("skv_gemv_{}")(P, P, P, P, P, 512, 4096, 1, 0) == -1                                     # bias with fused SiLU
    q = (P, P, P, 0, P, 1e-5, 0, 0)
    qk = f("skv_qkv_gemv_rope_update_{}")
    assert qk(*q, 0, P, P, 0, P, P, P, 4096, 2, 1, 128, 128, 64, 1024, 8, 1, 0) == -1   # no RoPE table
    assert qk(*q, P, 0, P, 0, P, P, P, 4096, 2, 1, 128, 128, 64, 1024, 8, 1, 0) == -1   # no position
    assert qk(*q, P, P, P, 0, P, P, 0, 4096, 2, 1, 128, 128, 64, 1024, 8, 1, 0) == -1   # no v cache
    assert qk(*q, P, P, P, 0, P, P, P, 4096, 2, 1, 64, 128, 64, 1024, 8, 1, 0) == -2    # head_dim 64
    assert qk(*q, P, P, P, 0, P, P, P, 4096, 2, 1, 128, 128, 64, 1024, 8, 3, 0) == -2   # rope mode
    assert qk(0, *q[1:], P, P, P, 0, P, P, P, 4096, 2, 1, 64, 128, 64, 1024, 8, 1, 0) == -2   # the entry's own checks first
    assert qk(*q, P, P, P, 0, P, P, P, 4096, 0, 1, 128, 128, 64, 1024, 8, 1, 0) == -1   # no query head
    # near-pull: the role's own arguments, after the GEMV's
    down, gate = f("skv_gemv_near_pull_{}"), f("skv_norm_gemv_near_pull_{}")
    assert down(P, P, P, 0, P, 4096, 4096, 0, *NEAR[1:], 1, 0) == -1                    # no early state
    assert down(P, P, P, 0, P, 4096, 4096, *NEAR[:-1], 8, 1, 0) == -1                   # 8 pull parts
    assert down(P, P, P, 0, P, 4096, 4096, *NEAR[:-1], 3, 1, 0) == -1
    assert down(P, P, P, 0, P, 4096, 4104, *NEAR[:-1], 3, 1, 0) == -2                   # the GEMV's own checks first
    assert down(P, P, P, 0, P, 4096, 4096, *NEAR, 2, 0) == -1 and down(P, P, P, 0, P, 4096, 4096, *NEAR, -1, 0) == -1     # list
    assert down(P, P, P, 0, P, 8208, 4096, *NEAR, 1, 0) == -2                           # more than 8,192 rows
    assert gate(P, P, P, 0, P, 1e-5, 0, P, 1024, 4096, *NEAR, 0, 0) == -1 and gate(P, P, P, 0, P, 1e-5, 0, P, 1024, 4096, *NEAR, 3, 0) == -1
    assert gate(P, P, P, 0, P, 1e-5, 0, P, 1023, 4096, *NEAR, 1, 0) == -2               # an odd number of [gate; up] rows
    assert gate(P, P, P, 0, 0, 1e-5, 0, P, 1024, 4096, *NEAR, 1, 0) == -2               # no norm weight
    big = NEAR[:4] + ((1 << 18) + 1,) + NEAR[5:]
    assert down(P, P, P, 0, P, 4096, 4096, *big, 1, 0) == -2                            # the early state's limit


# ------------------------------------------------------------------------------------------------------------- the model
def _tiny(**kw):
    from shadowkv_amd import llama
    cfg = llama.ModelConfig(name="tiny", hidden_size=1024, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=8,
                            num_key_value_heads=2, vocab_size=2000, qkv_bias=True)
    return llama.DecoderLM(cfg=cfg, device="cpu", max_length=256, attn_mode="full", max_new_tokens=16, **kw), llama


def test_unknown_weight_dtypes_are_still_refused():
    from shadowkv_amd import llama
    assert llama.WEIGHT_DTYPES == ("bf16", "fp8_e4m3", "mxfp4")
    for bad in ("int4", "fp4", "MXFP4", "mxfp8", None):
        with pytest.raises(ValueError):
            llama.DecoderLM(weight_dtype=bad)         # (the full-size default config: refused before anything is allocated)


def test_mxfp4_model_is_the_quantised_bf16_model_and_counts_its_bytes():
    t = _q()
    m4, _ = _tiny(weight_dtype="mxfp4", seed=9)
    mb, _ = _tiny(seed=9)
    assert m4.weight_dtype == "mxfp4" and mb.weight_dtype == "bf16"
    want = 0
    for l4, lb in zip(m4.layers, mb.layers):
        for name in ("wqkv", "wo", "gate_up_proj", "down_proj"):
            w4, sc = getattr(l4, name), getattr(l4, name + "_scale")
            N, K = getattr(lb, name).shape
            assert w4.dtype == torch.uint8 and w4.shape == (N, K // 2) and sc.dtype == torch.uint8 and sc.shape == (N, K // 32)
            q4, qs = t.quantize_mxfp4_rows(getattr(lb, name))
            assert torch.equal(w4, q4) and torch.equal(sc, qs), name
            assert torch.equal(l4.prefill_weight(name), t.dequantize_mxfp4_rows(w4, sc)) and l4.prefill_weight(name).dtype == torch.bfloat16
            want += N * K // 2 + N * K // 32
        assert l4.bqkv.dtype == torch.bfloat16 and l4.input_layernorm_weight.dtype == torch.bfloat16
    assert m4.lm_head.dtype == torch.uint8 and m4.lm_head_scale.shape == (2000, 1024 // 32)
    assert m4.embed_tokens.dtype == torch.bfloat16 and m4.norm_weight.dtype == torch.bfloat16
    want += 2000 * 1024 // 2 + 2000 * 1024 // 32
    assert m4.weight_bytes() == want
    assert mb.weight_bytes() * 17 == want * 64                        # 4.25 bits against 16
    # idempotent; in place on a bf16 model; the other format is refused in both directions; existing calls are unchanged
    before = m4.layers[0].wqkv
    assert m4.quantize_weights(dtype="mxfp4") is m4 and m4.layers[0].wqkv is before
    with pytest.raises(ValueError):
        m4.quantize_weights()
    with pytest.raises(ValueError):
        m4.quantize_weights(dtype="fp8_e4m3")
    with pytest.raises(ValueError):
        mb.quantize_weights(dtype="int4")
    assert mb.weight_dtype == "bf16"
    mb.quantize_weights(dtype="mxfp4")
    assert mb.weight_dtype == "mxfp4" and mb.weight_bytes() == want
    m8, _ = _tiny(seed=9)
    m8.quantize_weights(True)                                         # positional pow2_scale, default dtype: FP8 as before
    assert m8.weight_dtype == "fp8_e4m3" and m8.lm_head.dtype == torch.float8_e4m3fn
    with pytest.raises(ValueError):
        m8.quantize_weights(dtype="mxfp4")


def test_cpu_model_prefills_through_the_dequantising_path():
    """The dense half of a prefill layer on a CPU-device MXFP4 model (the attention between the two halves is a native kernel):
    pre_attention_compute, post_attention_compute and the lm_head read the matrices through prefill_weight.  The bf16 model
    overwritten with the dequantised weights holds the same numbers and runs the same torch ops: the same bits."""
    t = _q()
    a, _ = _tiny(weight_dtype="mxfp4", seed=3)
    b, _ = _tiny(seed=3)
    for la, lb in zip(a.layers, b.layers):
        for name in ("wqkv", "wo", "gate_up_proj", "down_proj"):
            getattr(lb, name).copy_(t.dequantize_mxfp4_rows(getattr(la, name), getattr(la, name + "_scale")))
    b.lm_head.copy_(t.dequantize_mxfp4_rows(a.lm_head, a.lm_head_scale))
    ids = torch.randint(0, 2000, (1, 40), generator=torch.Generator().manual_seed(3))
    with torch.inference_mode():
        hs = torch.nn.functional.embedding(ids, a.embed_tokens)
        for la, lb in zip(a.layers, b.layers):
            qa, qb = a.pre_attention_compute(hs, la), b.pre_attention_compute(hs, lb)
            for u, v in zip(qa, qb):
                assert torch.equal(u, v)
            attn = qa[0].contiguous()                          # [1, 40, hidden]: stands in for the attention output
            oa, ob = a.post_attention_compute(attn, hs, la), b.post_attention_compute(attn, hs, lb)
            assert oa.shape == hs.shape and torch.equal(oa, ob) and bool(torch.isfinite(oa.float()).all())
            hs = oa
        last = t.layer_norm(hs[:, -1:, :], a.norm_variance_epsilon, a.norm_weight)
        la, lb = torch.nn.functional.linear(last, a._lm_head_prefill()), torch.nn.functional.linear(last, b._lm_head_prefill())
    assert la.shape == (1, 1, 2000) and torch.equal(la, lb) and float(la.float().abs().max()) > 0
    assert a.layers[0].wqkv.dtype == torch.uint8 and a.lm_head.dtype == torch.uint8          # the temporaries were temporaries
