"""CPU: the MXFP4 rows path (2..32 token rows against e2m1 nibbles + e8m0 block scales) without a GPU -
the export and its host-side argument checks (they run before any HIP call), the mxfp4_rows keyword of the decode ops and of
DecoderLM, and the builders of the GPU tests' exact and random cases."""
import pytest
import torch

P = 0x1000            # a non-null pointer that is never dereferenced on the host


def _rows(W=P, s=P, X=P, bias=0, Y=P, M=8, N=512, K=4096, silu=0):
    from shadowkv_amd import _lib
    return _lib.lib().skv_linear_rows_mxfp4(W, s, X, bias, Y, M, N, K, silu, 0)


def test_the_export_exists_and_the_abi_version_is_unchanged():
    from shadowkv_amd import _lib
    assert hasattr(_lib.lib(), "skv_linear_rows_mxfp4")
    assert _lib.lib().skv_abi_version() == 1


def test_rows_mxfp4_refuses_bad_arguments_before_any_launch():
    """-1 (SKV_ERR_ARG): a null W4 / scale_e8m0 / X / Y, M < 1, N < 1, the SiLU pair form with an odd N or with a bias.
    -2 (SKV_ERR_UNSUPPORTED): M > 32, K % 128 != 0, K < 128.  No GPU is present: a call that reached the HIP runtime could not
    return these codes."""
    assert _rows(W=0) == -1 and _rows(s=0) == -1 and _rows(X=0) == -1 and _rows(Y=0) == -1
    assert _rows(M=0) == -1 and _rows(M=-3) == -1
    assert _rows(N=0) == -1 and _rows(N=-16) == -1
    assert _rows(N=511, silu=1) == -1
    assert _rows(bias=P, silu=1) == -1
    assert _rows(M=33) == -2 and _rows(M=1000) == -2
    assert _rows(K=4096 + 64) == -2 and _rows(K=4096 + 32) == -2 and _rows(K=200) == -2
    assert _rows(K=64) == -2 and _rows(K=0) == -2 and _rows(K=-128) == -2
    assert _rows(K=4096 + 64, silu=1) == -2 and _rows(M=33, bias=P) == -2


def _pair(N=4, K=1024):
    from shadowkv_amd import tensor_op as t
    return t.quantize_mxfp4_rows(torch.ones(N, K))


def test_the_decode_ops_refuse_an_unknown_mxfp4_rows():
    from shadowkv_amd import tensor_op as t
    w4, sc = _pair()
    x = torch.ones(2, 1, 1024, dtype=torch.bfloat16)
    nw = torch.ones(1024, dtype=torch.bfloat16)
    cache = torch.zeros(2, 1, 8, 128, dtype=torch.bfloat16)
    for bad in ("Native", "fast", None, True):
        with pytest.raises(ValueError, match="mxfp4_rows"):
            t.linear_decode(x, w4, w_scale=sc, mxfp4_rows=bad)
        with pytest.raises(ValueError, match="mxfp4_rows"):
            t.linear_decode(x, torch.ones(4, 1024, dtype=torch.bfloat16), mxfp4_rows=bad)        # bf16 weights: refused all the same
        with pytest.raises(ValueError, match="mxfp4_rows"):
            t.norm_linear_decode(x, None, nw, 1e-5, w4, w_scale=sc, mxfp4_rows=bad)
        with pytest.raises(ValueError, match="mxfp4_rows"):
            t.norm_qkv_rope_update(x, None, nw, 1e-5, w4, None, x, x, x, cache, cache, 1, 1, w_scale=sc, mxfp4_rows=bad)
    assert t.MXFP4_ROWS_MODES == ("fallback", "native")


def test_native_on_a_cpu_device_still_takes_the_fallback_and_counts_there():
    """x on the CPU: mxfp4_rows="native" launches nothing - the dequantising fallback answers, bit-equal to the default's."""
    from shadowkv_amd import tensor_op as t
    g = torch.Generator().manual_seed(3)
    w4, sc = t.quantize_mxfp4_rows(torch.randn(6, 1024, generator=g) * 0.05)
    x = torch.randn(2, 1, 1024, generator=g).bfloat16()
    n0, f0 = t.mxfp4_native_calls, t.mxfp4_fallback_calls
    y0 = t.linear_decode(x, w4, w_scale=sc)
    y1 = t.linear_decode(x, w4, w_scale=sc, mxfp4_rows="native")
    out = torch.empty(2, 1, 6, dtype=torch.bfloat16)
    y2 = t.linear_decode(x, w4, w_scale=sc, mxfp4_rows="native", out=out)
    assert y2 is out and torch.equal(y0, y1) and torch.equal(y0, y2)
    assert torch.equal(y0, torch.nn.functional.linear(x, t.dequantize_mxfp4_rows(w4, sc)))
    assert t.mxfp4_fallback_calls - f0 == 3 and t.mxfp4_native_calls == n0


def _tiny(**kw):
    from shadowkv_amd import llama
    cfg = llama.ModelConfig(name="tiny", hidden_size=1024, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=8,
                            num_key_value_heads=2, vocab_size=2000, qkv_bias=True)
    return llama.DecoderLM(cfg=cfg, device="cpu", max_length=256, attn_mode="full", max_new_tokens=16, **kw), llama


def test_unknown_mxfp4_rows_is_refused_before_anything_is_allocated():
    from shadowkv_amd import llama
    for bad in ("Native", "fast", None, 1):
        with pytest.raises(ValueError, match="mxfp4_rows"):
            llama.DecoderLM(mxfp4_rows=bad)               # (the full-size default config: nothing may be allocated)
        with pytest.raises(ValueError, match="mxfp4_rows"):
            llama.DecoderLM(weight_dtype="mxfp4", mxfp4_rows=bad)
        with pytest.raises(ValueError, match="mxfp4_rows"):
            llama.GLM(mxfp4_rows=bad)


def test_a_tiny_model_carries_mxfp4_rows_through_quantize_weights():
    m, _ = _tiny(seed=9)
    assert m.mxfp4_rows == "fallback"                     # the default stays the fallback
    m, _ = _tiny(seed=9, mxfp4_rows="native")
    assert m.mxfp4_rows == "native" and m.weight_dtype == "bf16"        # inert on a bf16 model
    before = m.weight_bytes()
    m.quantize_weights(dtype="mxfp4")
    assert m.mxfp4_rows == "native" and m.weight_dtype == "mxfp4"
    m4, _ = _tiny(seed=9, weight_dtype="mxfp4", mxfp4_rows="native")
    assert m4.mxfp4_rows == "native" and m4.weight_dtype == "mxfp4" and m4.fp8_rows == "fallback"
    ref, _ = _tiny(seed=9, weight_dtype="mxfp4")
    assert m4.weight_bytes() == ref.weight_bytes() == m.weight_bytes() < before         # weight_bytes() does not read the option


@pytest.mark.parametrize("N", [48, 2 * 1003, 6160, 16400])
def test_the_exact_case_builders_hold_for_every_shape_of_the_gpu_grid(N):
    """RowsBank.expected's assertions (exact partial sums, bf16 totals, the f64 decode of the packed bytes) for every (M, N, K)
    of tests/test_gpu_rows_gemm_mxfp4_exact.py; the block-scale bytes stay in 125 .. 129 and the blocks of a row alternate."""
    import mxfp4_rows_ref as rr
    assert N in rr.ROWS_N and len(rr.ROWS_N) == 4
    for K in rr.ROWS_K:
        rb, xi, silu = rr.exact_case(N, K)
        assert rb.rows == N and rb.K == K and xi.shape == (32, K)
        t32 = rb.expected(xi)
        for M in rr.ROWS_M:
            assert torch.equal(rb.expected(xi[:M], decode=False), t32[:M])
        sc = rb.pack().w_scale
        assert int(sc.min()) >= 125 and int(sc.max()) <= 129
        assert bool((sc[:, 0] != sc[:, 1]).all())
        if silu:
            assert bool((t32 != 0).all())


def test_the_decode_probe_covers_every_position_of_the_k_step():
    import mxfp4_rows_ref as rr
    w4, sc, col, val = rr.decode_probe_rows()
    assert w4.shape == (16 * 2 * 16 * 4 * 2 + 16 * 5 + 201, rr.PROBE_K // 2)
    assert set((col[:4096] % 32).tolist()) == set(range(32)) and set((col[:4096] // 32).tolist()) == set(range(8))
    assert set(sc[4096 + 80:, 6].tolist()) == set(range(27, 228))


def test_the_cpu_flip_counts_of_the_random_case_are_the_constants_of_the_gpu_test():
    """The two CPU f32 evaluations of the random case (tests/mxfp4_rows_ref.py), recomputed: the GPU test's bound is 4 x the larger;
    and the rule that chose the case's seed."""
    import mxfp4_rows_ref as rr
    import test_gpu_rows_gemm_mxfp4_exact as gpu
    (seq, total, seq_ulp), (pair, total2, pair_ulp) = rr.cpu_flips()
    print(f"sequential {seq} of {total} (max {seq_ulp} ulp), pairwise {pair} of {total2} (max {pair_ulp} ulp)")
    assert seq_ulp <= 1 and pair_ulp <= 1             # the case's seed: a plain f32 accumulation meets the one-ulp criterion
    base = dict(rr.RANDOM_ROWS_MXFP4, seed=17 + 6160 + 1152)
    assert rr.RANDOM_ROWS_MXFP4["seed"] == base["seed"] + 1 and max(r[2] for r in rr.cpu_flips(base)) > 1     # and it is the first
    assert total == total2 == gpu.ROWS_MXFP4_OUTPUTS
    assert (seq, pair) == gpu.ROWS_MXFP4_CPU_FLIPS
    assert gpu.ROWS_MXFP4_SHARE_BOUND == 4 * max(seq, pair) / total
