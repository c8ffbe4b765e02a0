"""CPU: the weight-only FP8 (e4m3) path without a GPU - the row quantiser / dequantiser (tensor_op), the host-side argument
checks of every FP8 export (they run before any HIP call), DecoderLM's weight_dtype handling and byte accounting."""
import pytest
import torch


def _q():
    from shadowkv_amd import tensor_op
    return tensor_op


# ------------------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("pow2", [False, True])
def test_round_trip_within_half_an_e4m3_ulp(pow2):
    """e4m3 has 3 mantissa bits: a normal value is within 2^-4 relative of its rounding; below the smallest normal (2^-6 in
    units of the row scale) the spacing is 2^-9, half of it 2^-10.  The f32 division and multiplication by the scale add a few
    2^-24 relative (nothing for a power-of-two scale): 2^-20 covers them."""
    t = _q()
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(37, 1040, generator=g) * 0.02).bfloat16()
    w8, scale = t.quantize_fp8_rows(w, pow2_scale=pow2)
    assert w8.dtype == torch.float8_e4m3fn and w8.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (37,)
    back = t.dequantize_fp8_rows(w8, scale, dtype=torch.float32).double()
    wd, sd = w.double(), scale.double().unsqueeze(1)
    bound = (2.0 ** -4 + 2.0 ** -20) * wd.abs() + 2.0 ** -10 * sd
    assert bool(((back - wd).abs() <= bound).all()), float(((back - wd).abs() - bound).max())
    # the largest element of every row maps to +-448 (pow2: to at least 224), so the range is used
    top = w8.float().abs().amax(dim=1)
    assert bool((top == 448).all()) if not pow2 else bool(((top > 224 - 1e-9) & (top <= 448)).all())
    # the bf16 form: one more rounding, half a bf16 ulp = at most 2^-8 relative
    b16 = t.dequantize_fp8_rows(w8, scale)
    assert b16.dtype == torch.bfloat16
    assert bool(((b16.double() - back).abs() <= 2.0 ** -8 * back.abs()).all())


def test_no_nan_byte_for_extreme_rows():
    """torch's cast to float8_e4m3fn does not saturate (500 -> 0x7F): the quantiser clamps first.  Rows with bf16's largest
    finite values, mixed magnitudes, tiny values and a row of equal values."""
    t = _q()
    big = torch.finfo(torch.bfloat16).max
    rows = torch.zeros(6, 1024)
    rows[0, :] = big
    rows[0, 1::2] = -big
    rows[1, 0], rows[1, 1], rows[1, 2] = big, -1.0, 1e-30
    rows[2, :] = torch.finfo(torch.bfloat16).tiny
    rows[3, :] = torch.linspace(-3, 3, 1024)
    rows[4, 5] = -7.0
    rows[5, :] = 1e-38
    w = rows.bfloat16()
    for pow2 in (False, True):
        w8, scale = t.quantize_fp8_rows(w, pow2_scale=pow2)
        b = w8.view(torch.uint8)
        assert not bool(((b == 0x7F) | (b == 0xFF)).any())
        assert bool(torch.isfinite(scale).all()) and bool((scale > 0).all())
        if not pow2:      # (rounded up to a power of two, bf16's largest value comes back as 2^128: beyond f32, not a byte matter)
            assert bool(torch.isfinite(t.dequantize_fp8_rows(w8, scale, dtype=torch.float32)).all())
    assert int(torch.tensor(500.0).to(torch.float8_e4m3fn).view(torch.uint8)) == 0x7F          # why the clamp is there


def test_pow2_scales_are_powers_of_two_and_not_smaller():
    t = _q()
    g = torch.Generator().manual_seed(2)
    w = (torch.randn(64, 1024, generator=g) * torch.logspace(-3, 2, 64).unsqueeze(1)).bfloat16()
    w[7] = 0
    w[8, :] = 0
    w[8, 3] = 448.0           # amax / 448 == 1: a power of two already, must stay 1
    _, s0 = t.quantize_fp8_rows(w)
    _, s2 = t.quantize_fp8_rows(w, pow2_scale=True)
    m, _ = torch.frexp(s2)
    assert bool((m == 0.5).all())
    assert bool((s2 >= s0).all()) and bool((s2 < 2 * s0)[s0 != 1].all())
    assert float(s2[8]) == 1.0 and float(s0[8]) == 1.0


def test_all_zero_row_gets_scale_one_and_zero_bytes():
    t = _q()
    w = torch.zeros(3, 1024, dtype=torch.bfloat16)
    w[1, 10] = 0.5
    for pow2 in (False, True):
        w8, scale = t.quantize_fp8_rows(w, pow2_scale=pow2)
        assert float(scale[0]) == 1.0 and float(scale[2]) == 1.0
        assert bool((w8.view(torch.uint8)[0] == 0).all()) and bool((w8.view(torch.uint8)[2] == 0).all())
        assert float(t.dequantize_fp8_rows(w8, scale, dtype=torch.float32)[1, 10]) == 0.5


def test_decode_ops_refuse_fp8_weights_without_matching_scales():
    t = _q()
    w8, scale = t.quantize_fp8_rows(torch.ones(4, 1024))
    x = torch.ones(1, 1, 1024, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        t.linear_decode(x, torch.ones(4, 1024, dtype=torch.bfloat16), w_scale=scale)       # bf16 weights with a scale
    with pytest.raises(ValueError):
        t.linear_decode(x, w8, w_scale=scale[:3])
    assert t.kv_proj_split_supported(x, w8, torch.zeros(1, 1, 8, 128)) is False
    with pytest.raises(ValueError):
        t.norm_q_rope(x, None, x, 1e-5, w8, None, x, x, x, torch.zeros(1, 1, 8, 128), torch.zeros(1, 1, 8, 128), 1, 1)


# ------------------------------------------------------------------------------------------------ host-side argument checks
P = 0x1000            # a non-null pointer that is never dereferenced on the host
NEAR = (P, 8, 4, 1000, 2000, 64, P, 8 * 2000 * 1024, 1)      # early state, blocks, groups, landmarks, chunks, E, V table, stride, parts


def _entries():
    """name -> call(W, scale, x, y, N, K): every FP8 export with otherwise valid arguments."""
    from shadowkv_amd import _lib
    L = _lib.lib()
    qkv_tail = (P, P, P, 0, P, P, P)          # cos_sin, pos, row_idx, q_override, q_out, k_cache, v_cache
    return {
        "gemv": lambda W, s, x, y, N, K: L.skv_gemv_fp8(W, s, x, 0, y, N, K, 0, 0),
        "gemv_silu": lambda W, s, x, y, N, K: L.skv_gemv_fp8(W, s, x, 0, y, N, K, 1, 0),
        "norm": lambda W, s, x, y, N, K: L.skv_norm_gemv_fp8(W, s, x, 0, P, 1e-5, 0, 0, y, N, K, 0, 0),
        "rangemax": lambda W, s, x, y, N, K: L.skv_norm_gemv_rangemax_fp8(W, s, x, 0, P, 1e-5, 0, 0, y, N, K, P, 0),
        "near_gate_up": lambda W, s, x, y, N, K: L.skv_norm_gemv_near_pull_fp8(W, s, x, 0, P, 1e-5, 0, y, N, K, *NEAR, 1, 0),
        "near_down": lambda W, s, x, y, N, K: L.skv_gemv_near_pull_fp8(W, s, x, 0, y, N, K, *NEAR, 1, 0),
        # (N is (q_heads + 2 kv_heads) * 128 there: q_heads = N / 128 - 2, one KV head; y: q_out)
        "qkv": lambda W, s, x, y, N, K: L.skv_qkv_gemv_rope_update_fp8(W, s, x, 0, P, 1e-5, 0, 0, qkv_tail[0], qkv_tail[1],
                                                                         qkv_tail[2], 0, y, P, P, K, N // 128 - 2, 1, 128, 128, 64,
                                                                         8 * 128, 8, 1, 0),
    }


NORM_ENTRIES = ("norm", "rangemax", "near_gate_up", "qkv")


@pytest.mark.parametrize("name", ["gemv", "gemv_silu", "norm", "rangemax", "near_gate_up", "near_down", "qkv"])
def test_fp8_entries_refuse_bad_arguments_before_any_launch(name):
    """-1 (SKV_ERR_ARG) for a missing pointer or N < 1; -2 (SKV_ERR_UNSUPPORTED) for K % 16 != 0, K = 512 and, norm variants,
    K != 4096.  No GPU is present: a call that reached the HIP runtime could not return these codes."""
    call = _entries()[name]
    N, K = 512, 4096
    for W, s, x, y in ((0, P, P, P), (P, 0, P, P), (P, P, 0, P), (P, P, P, 0)):
        assert call(W, s, x, y, N, K) == -1, (name, W, s, x, y)
    if name != "qkv":
        assert call(P, P, P, P, 0, K) == -1 and call(P, P, P, P, -16, K) == -1
    else:
        assert call(P, P, P, P, 2 * 128, K) == -1                    # no query head
    assert call(P, P, P, P, N, 4104) == -2                           # K % 16 != 0
    assert call(P, P, P, P, N, 512) == -2                            # below one k-step
    assert call(P, P, P, P, N, 1016) == -2
    if name in NORM_ENTRIES:
        assert call(P, P, P, P, N, 2048) == -2 and call(P, P, P, P, N, 8192) == -2          # the norm prologue: K == 4096


def test_fp8_rangemax_and_qkv_specific_checks():
    from shadowkv_amd import _lib
    L = _lib.lib()
    assert L.skv_norm_gemv_rangemax_fp8(P, P, P, 0, P, 1e-5, 0, 0, P, 4104, 4096, P, 0) == -2       # N % 16 != 0
    assert L.skv_norm_gemv_rangemax_fp8(P, P, P, 0, P, 1e-5, 0, 0, P, 4096, 4096, 0, 0) == -1       # no keys buffer
    assert L.skv_norm_gemv_fp8(P, P, P, 0, 0, 1e-5, 0, 0, P, 512, 4096, 0, 0) == -2                 # norm without a norm weight
    q = (P, P, P, 0, P, 1e-5, 0, 0)
    assert L.skv_qkv_gemv_rope_update_fp8(*q, 0, P, P, 0, P, P, P, 4096, 2, 1, 128, 128, 64, 1024, 8, 1, 0) == -1   # no RoPE table
    assert L.skv_qkv_gemv_rope_update_fp8(*q, P, P, P, 0, P, P, P, 4096, 2, 1, 64, 128, 64, 1024, 8, 1, 0) == -2    # head_dim 64
    assert L.skv_qkv_gemv_rope_update_fp8(*q, P, P, P, 0, P, P, P, 4096, 2, 1, 128, 128, 64, 1024, 8, 3, 0) == -2   # rope mode
    # near-pull: the role's own arguments (no early state: -1; 8 pull parts: -1); a SiLU launch has no bias slot
    assert L.skv_gemv_near_pull_fp8(P, P, P, 0, P, 4096, 4096, 0, *NEAR[1:], 1, 0) == -1
    assert L.skv_gemv_near_pull_fp8(P, P, P, 0, P, 4096, 4096, *NEAR[:-1], 8, 1, 0) == -1
    assert L.skv_gemv_near_pull_fp8(P, P, P, 0, P, 8208, 4096, *NEAR, 1, 0) == -2                   # more than 8,192 rows
    assert L.skv_gemv_fp8(P, P, P, P, P, 512, 4096, 1, 0) == -1                                     # bias with fused SiLU
    assert _lib.lib().skv_abi_version() == 1


# ------------------------------------------------------------------------------------------------------------- the model
def _tiny(**kw):
    from shadowkv_amd import llama
    cfg = llama.ModelConfig(name="tiny", hidden_size=1024, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=8,
                            num_key_value_heads=2, vocab_size=2000, qkv_bias=True)
    return llama.DecoderLM(cfg=cfg, device="cpu", max_length=256, attn_mode="full", max_new_tokens=16, **kw), llama


def test_unknown_weight_dtype_is_refused():
    from shadowkv_amd import llama
    for bad in ("int4", "fp8", "FP8_E4M3", None):
        with pytest.raises(ValueError):
            llama.DecoderLM(weight_dtype=bad)         # (the full-size default config: refused before anything is allocated)


def test_fp8_model_is_the_quantised_bf16_model_and_counts_its_bytes():
    t = _q()
    m8, _ = _tiny(weight_dtype="fp8_e4m3", seed=9)
    mb, _ = _tiny(seed=9)
    assert m8.weight_dtype == "fp8_e4m3" and mb.weight_dtype == "bf16"
    want = 0
    for l8, lb in zip(m8.layers, mb.layers):
        for name in ("wqkv", "wo", "gate_up_proj", "down_proj"):
            w8, sc = getattr(l8, name), getattr(l8, name + "_scale")
            assert w8.dtype == torch.float8_e4m3fn and sc.dtype == torch.float32 and sc.shape == (w8.shape[0],)
            q8, qs = t.quantize_fp8_rows(getattr(lb, name))
            assert torch.equal(w8.view(torch.uint8), q8.view(torch.uint8)) and torch.equal(sc, qs), name
            assert getattr(lb, name + "_scale") is None
            want += w8.numel() + 4 * w8.shape[0]
        assert l8.bqkv.dtype == torch.bfloat16 and l8.input_layernorm_weight.dtype == torch.bfloat16
    assert m8.lm_head.dtype == torch.float8_e4m3fn and m8.lm_head_scale.shape == (2000,)
    assert m8.embed_tokens.dtype == torch.bfloat16 and m8.norm_weight.dtype == torch.bfloat16
    want += m8.lm_head.numel() + 4 * 2000
    assert m8.weight_bytes() == want
    n = mb.lm_head.numel() + sum(getattr(l, k).numel() for l in mb.layers for k in ("wqkv", "wo", "gate_up_proj", "down_proj"))
    assert mb.weight_bytes() == 2 * n and want < mb.weight_bytes() * 0.51
    # idempotent, and in place on a bf16 model
    before = m8.layers[0].wqkv
    m8.quantize_weights(pow2_scale=True)
    assert m8.layers[0].wqkv is before
    mb.quantize_weights(pow2_scale=True)
    assert mb.weight_dtype == "fp8_e4m3" and mb.weight_bytes() == want
    m, _ = torch.frexp(mb.layers[1].down_proj_scale)
    assert bool((m == 0.5).all())
