"""CPU: the FP8 rows path (2..32 token rows against e4m3 weights) without a GPU - the export and its
host-side argument checks (they run before any HIP call), the fp8_rows keyword of the decode ops and of DecoderLM."""
import pytest
import torch

P = 0x1000            # a non-null pointer that is never dereferenced on the host


def _rows(W=P, s=P, X=P, bias=0, Y=P, M=8, N=512, K=4096, silu=0):
    from shadowkv_amd import _lib
    return _lib.lib().skv_linear_rows_fp8(W, s, X, bias, Y, M, N, K, silu, 0)


def test_the_export_exists_and_the_abi_version_is_unchanged():
    from shadowkv_amd import _lib
    assert hasattr(_lib.lib(), "skv_linear_rows_fp8")
    assert _lib.lib().skv_abi_version() == 1


def test_rows_fp8_refuses_bad_arguments_before_any_launch():
    """-1 (SKV_ERR_ARG): a null W8 / scale / X / Y, M < 1, N < 1, the SiLU pair form with an odd N or with a bias.
    -2 (SKV_ERR_UNSUPPORTED): M > 32, K % 64 != 0, K < 64.  No GPU is present: a call that reached the HIP runtime could not
    return these codes."""
    assert _rows(W=0) == -1 and _rows(s=0) == -1 and _rows(X=0) == -1 and _rows(Y=0) == -1
    assert _rows(M=0) == -1 and _rows(M=-3) == -1
    assert _rows(N=0) == -1 and _rows(N=-16) == -1
    assert _rows(N=511, silu=1) == -1
    assert _rows(bias=P, silu=1) == -1
    assert _rows(M=33) == -2 and _rows(M=1000) == -2
    assert _rows(K=4096 + 32) == -2 and _rows(K=4096 + 16) == -2 and _rows(K=100) == -2
    assert _rows(K=32) == -2 and _rows(K=0) == -2
    assert _rows(K=4096 + 32, silu=1) == -2 and _rows(M=33, bias=P) == -2


def test_linear_decode_refuses_an_unknown_fp8_rows():
    from shadowkv_amd import tensor_op as t
    w8, scale = t.quantize_fp8_rows(torch.ones(4, 1024))
    x = torch.ones(2, 1, 1024, dtype=torch.bfloat16)
    nw = torch.ones(1024, dtype=torch.bfloat16)
    cache = torch.zeros(2, 1, 8, 128, dtype=torch.bfloat16)
    for bad in ("Native", "fast", None, True):
        with pytest.raises(ValueError, match="fp8_rows"):
            t.linear_decode(x, w8, w_scale=scale, fp8_rows=bad)
        with pytest.raises(ValueError, match="fp8_rows"):
            t.linear_decode(x, torch.ones(4, 1024, dtype=torch.bfloat16), fp8_rows=bad)          # bf16 weights: refused all the same
        with pytest.raises(ValueError, match="fp8_rows"):
            t.norm_linear_decode(x, None, nw, 1e-5, w8, w_scale=scale, fp8_rows=bad)
        with pytest.raises(ValueError, match="fp8_rows"):
            t.norm_qkv_rope_update(x, None, nw, 1e-5, w8, None, x, x, x, cache, cache, 1, 1, w_scale=scale, fp8_rows=bad)
    assert t.FP8_ROWS_MODES == ("fallback", "native")


def _tiny(**kw):
    from shadowkv_amd import llama
    cfg = llama.ModelConfig(name="tiny", hidden_size=1024, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=8,
                            num_key_value_heads=2, vocab_size=2000, qkv_bias=True)
    return llama.DecoderLM(cfg=cfg, device="cpu", max_length=256, attn_mode="full", max_new_tokens=16, **kw), llama


def test_unknown_fp8_rows_is_refused_before_anything_is_allocated():
    from shadowkv_amd import llama
    for bad in ("Native", "fast", None, 1):
        with pytest.raises(ValueError, match="fp8_rows"):
            llama.DecoderLM(fp8_rows=bad)                 # (the full-size default config: nothing may be allocated)
        with pytest.raises(ValueError, match="fp8_rows"):
            llama.DecoderLM(weight_dtype="fp8_e4m3", fp8_rows=bad)
        with pytest.raises(ValueError, match="fp8_rows"):
            llama.GLM(fp8_rows=bad)


def test_a_tiny_model_carries_fp8_rows_through_quantize_weights():
    m, _ = _tiny(seed=9)
    assert m.fp8_rows == "fallback"                       # the default stays the fallback
    m, _ = _tiny(seed=9, fp8_rows="native")
    assert m.fp8_rows == "native" and m.weight_dtype == "bf16"          # inert on a bf16 model
    before = m.weight_bytes()
    m.quantize_weights(pow2_scale=True)
    assert m.fp8_rows == "native" and m.weight_dtype == "fp8_e4m3"
    m8, _ = _tiny(seed=9, weight_dtype="fp8_e4m3", fp8_rows="native")
    assert m8.fp8_rows == "native" and m8.weight_dtype == "fp8_e4m3"
    ref, _ = _tiny(seed=9, weight_dtype="fp8_e4m3")
    assert m8.weight_bytes() == ref.weight_bytes() == m.weight_bytes() < before         # weight_bytes() does not read the option


def test_the_cpu_flip_counts_of_the_random_case_are_the_constants_of_the_gpu_test():
    """The two CPU f32 evaluations of the random case (tests/fp8_rows_ref.py), recomputed: the GPU test's bound is 4 x the larger."""
    import fp8_rows_ref as rr
    import test_gpu_rows_gemm_fp8_exact as gpu
    (seq, total), (pair, total2) = rr.cpu_flips()
    print(f"sequential {seq} of {total}, pairwise {pair} of {total2}")
    assert total == total2 == gpu.ROWS_FP8_OUTPUTS
    assert (seq, pair) == gpu.ROWS_FP8_CPU_FLIPS
    assert gpu.ROWS_FP8_SHARE_BOUND == 4 * max(seq, pair) / total
