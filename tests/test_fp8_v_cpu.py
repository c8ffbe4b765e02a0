"""CPU: the FP8 (e4m3) V offload table - the contract's own properties on the reference quantiser, the
cache built on a CPU device against that reference and against its bf16 twin, the refusals, and the argument checks of the
new C entries (no device is touched)."""
import os
import re

import pytest
import torch

import fp8_v_ref as R
import gen_inputs as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("skv_quantize_v_rows", "skv_land_chunks_fp8", "skv_fetch_kv_fp8", "skv_fetch_kv_inplace_fp8")


# ---------------------------------------------------------------------------------------------------- the contract
def test_reference_properties_on_every_finite_bf16_pattern():
    """No NaN byte; scale * e4m3(byte) is a bf16 number; |v' - v| <= half an e4m3 ulp of |v| / scale, times scale, wherever
    |v| / scale <= 448.  (Beyond that - only possible once the scale sits at its upper clamp 2^100 - the byte saturates: v' is
    +-448 * scale.  Nearly every row of the pattern set holds a value above 448 * 2^100, so this is not a corner.)"""
    v = R.pattern_rows()
    b, scale = R.quantize_rows(v)
    assert b.dtype == torch.uint8 and scale.dtype == torch.float32
    assert not bool(((b & 0x7F) == 0x7F).any()), "a NaN byte (0x7F / 0xFF) was produced"
    k = torch.log2(scale.double())
    assert torch.equal(k, k.round()) and float(k.min()) >= -100 and float(k.max()) <= 100
    assert float(scale[510]) == 1.0                                                   # the all-zero row
    assert bool((scale[511:515] == 2.0 ** -100).all())                                # magnitudes of 1e-30: the lower clamp
    assert float(scale[515]) == 2.0 ** 100 and float(scale[516]) < 2.0 ** 100         # 3e38: the upper clamp; 3e30: below it
    vq, prod = R.dequantize_rows(b, scale)
    assert torch.equal(vq.double(), prod), "scale * e4m3(byte) must be exactly representable in bf16"
    vd, sd = v.double(), scale.double().unsqueeze(-1)
    x = vd / sd
    inside = x.abs() <= R.E4M3_MAX
    err = (vq.double() - vd).abs()
    bound = 0.5 * R.e4m3_ulp(x.clamp(-R.E4M3_MAX, R.E4M3_MAX)) * sd
    assert bool((err[inside] <= bound[inside]).all())
    assert torch.equal(vq.double()[~inside], (torch.sign(vd) * R.E4M3_MAX * sd)[~inside])
    assert int(inside.sum()) > 60000 and int((~inside).sum()) > 0
    # the scale is the SMALLEST admissible power of two (inside the clamp)
    amax = vd.abs().amax(-1)
    free = (scale.double() > 2.0 ** -100) & (amax > 0)
    assert bool((amax[free] / (scale.double()[free] / 2) > R.E4M3_MAX).all())
    assert bool((amax[scale.double() < 2.0 ** 100] / scale.double()[scale.double() < 2.0 ** 100] <= R.E4M3_MAX).all())


def test_torch_mirror_equals_the_reference():
    """tensor_op.quantize_v_rows_torch (what a CPU cache fills its table with, and what the GPU kernel is pinned to through
    the same reference) gives the reference's bytes and scales; the Gaussian rows' relative RMS round-trip error is recorded
    in DESIGN.md section 11 (2.7 % per element)."""
    from shadowkv_amd import tensor_op
    g = torch.Generator().manual_seed(5)
    v = torch.cat((R.pattern_rows(), R.sweep_rows(), torch.randn(64, 128, generator=g).to(torch.bfloat16)))
    b, scale = R.quantize_rows(v)
    v8, sc = tensor_op.quantize_v_rows_torch(v)
    assert torch.equal(v8.view(torch.uint8), b) and torch.equal(sc, scale)
    assert torch.equal(tensor_op.dequantize_v_rows(v8, sc).view(torch.int16), R.dequantize_rows(b, scale)[0].view(torch.int16))
    gauss = v[-64:].double()
    rt = R.dequantize_rows(b[-64:], scale[-64:])[1]
    rel_rms = float(((rt - gauss) ** 2).mean().sqrt() / (gauss ** 2).mean().sqrt())
    assert 0.015 < rel_rms < 0.04, rel_rms       # e4m3 keeps 3 mantissa bits: 2^-4 / sqrt(3) = 3.6 % at worst, ~2.7 % measured


# ---------------------------------------------------------------------------------------------------- the cache, CPU device
def _build(case, v_dtype, extra=0):
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    c, inp = G.CASES[case], G.make_inputs(case)
    cache = ShadowKVCache_CPU(G.config_of(case), batch_size=1, max_length=c["L"] + extra, device="cpu", dtype=torch.bfloat16,
                              sparse_budget=c["budget"], chunk_size=c["chunk"], rank=c["rank"], v_dtype=v_dtype)
    cache.get_svd(inp["k_pre"], 0)
    k_roped = G.rope_torch(case, inp["k_pre"], inp["cos_sin"], torch.arange(c["L"]).unsqueeze(0))
    cache.prefill_kv_cache(inp["v"], 0, k_roped, inp["q_last"])
    return cache, [inp["v"]]


def _build_subbatched(case, v_dtype):
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    c = G.SUBBATCH_CASES[case]
    inputs = G.subbatch_inputs(case)
    cache = ShadowKVCache_CPU(G.config_of(case), batch_size=c["batch"], max_length=c["L"], device="cpu", dtype=torch.bfloat16,
                              sparse_budget=c["budget"], chunk_size=c["chunk"], rank=c["rank"], v_dtype=v_dtype)
    for i in range(0, c["batch"], c["sub"]):
        idx = list(range(i, i + c["sub"]))
        for l, inp in enumerate(inputs):
            cache.get_svd(inp["k_pre"][idx], l)
            cache.prefill_kv_cache(inp["v"][idx], l, inp["k_roped"][idx], inp["q_last"][idx])
    return cache, [inp["v"] for inp in inputs]


def check_fp8_cache_against_reference_and_twin(a, b, v_layers):
    """a: FP8-V cache, b: its bf16 twin, v_layers: the prompt's V per layer [bs, kv, L, D] (CPU).  Shared with the GPU tests."""
    C, D, S = a.chunk_size, a.head_dim, a.select_sets
    assert a.v_cache_cpu.dtype == torch.float8_e4m3fn and a.v_cache_cpu.shape == b.v_cache_cpu.shape
    assert a.v_scale.dtype == torch.float32 and tuple(a.v_scale.shape) == tuple(a.v_cache_cpu.shape[:-1]) + (C,)
    assert a.v_scale.device == a.k_cache_buffer.device
    for n in ("position_ids", "k_cache_buffer", "k_landmark", "k_landmark_idx", "U", "SV"):
        assert torch.equal(getattr(a, n).cpu(), getattr(b, n).cpu()), n
    n_chunks = v_layers[0].shape[2] // C
    for l, v in enumerate(v_layers):
        bs, kv = v.shape[:2]
        want_b, want_s = R.quantize_rows(v[:, :, :n_chunks * C])
        table = a.v_cache_cpu[l].cpu().view(torch.uint8)
        scale = a.v_scale[l].cpu()
        assert torch.equal(table[:, :, :n_chunks], want_b.view(bs, kv, n_chunks, C * D)), f"layer {l}: table bytes"
        assert torch.equal(scale[:, :, :n_chunks], want_s.view(bs, kv, n_chunks, C)), f"layer {l}: scales"
        assert not bool(table[:, :, n_chunks:].any()), "rows behind the prompt stay untouched"
        va, vb = a.v_cache_buffer[l].cpu(), b.v_cache_buffer[l].cpu()
        assert torch.equal(va[:, :, :a.sparse_start].view(torch.int16), vb[:, :, :a.sparse_start].view(torch.int16)), \
            f"layer {l}: local and outlier V rows are exact"
        assert torch.equal(va[:, :, a.sparse_end:].view(torch.int16), vb[:, :, a.sparse_end:].view(torch.int16))
        check_sparse_rows_are_dequantised_table_rows(a, l)


def check_sparse_rows_are_dequantised_table_rows(a, l):
    """The invariant: slot i of the sparse region holds dequant(table[position_ids[i]]) (empty slots, id -1, are skipped)."""
    C, D = a.chunk_size, a.head_dim
    pos = a.position_ids[l].cpu()                                                   # [bs, kv, R]
    bs, kv, Rs = pos.shape
    table = a.v_cache_cpu[l].cpu().view(torch.uint8)
    scale = a.v_scale[l].cpu()
    idx = pos.clamp_min(0)
    rows_b = table.gather(2, idx.unsqueeze(-1).expand(-1, -1, -1, C * D)).view(bs, kv, Rs, C, D)
    rows_s = scale.gather(2, idx.unsqueeze(-1).expand(-1, -1, -1, C))
    want = R.dequantize_rows(rows_b, rows_s)[0].view(torch.int16)
    got = a.v_cache_buffer[l].cpu()[:, :, a.sparse_start:a.sparse_start + Rs * C].reshape(bs, kv, Rs, C, D).view(torch.int16)
    live = (pos >= 0)[..., None, None].expand_as(got)
    assert torch.equal(got[live], want[live]), f"layer {l}: sparse-region V rows != dequant(table[position_ids])"


@pytest.mark.parametrize("extra", [0, 64])
def test_cpu_cache_matches_the_reference_and_its_bf16_twin(extra):
    a, v = _build("llama_small", "fp8_e4m3", extra)
    b, _ = _build("llama_small", "bf16", extra)
    check_fp8_cache_against_reference_and_twin(a, b, v)
    assert a.v_cache_cpu.shape[-2] == (G.CASES["llama_small"]["L"] + extra) // 8


def test_cpu_cache_subbatched_prefill():
    a, v = _build_subbatched("subbatch_llama", "fp8_e4m3")
    b, _ = _build_subbatched("subbatch_llama", "bf16")
    assert a.prefilled_batch == G.SUBBATCH_CASES["subbatch_llama"]["batch"]
    check_fp8_cache_against_reference_and_twin(a, b, v)


# ---------------------------------------------------------------------------------------------------- refusals
def test_bad_v_dtype_is_refused_before_any_allocation():
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    from shadowkv_amd.llama import DecoderLM
    c = G.CASES["llama_small"]
    with pytest.raises(ValueError, match="v_dtype"):
        ShadowKVCache_CPU(G.config_of("llama_small"), batch_size=1, max_length=1 << 40, device="cpu", sparse_budget=c["budget"],
                          v_dtype="fp8")                      # (a table of this size could not be allocated)
    with pytest.raises(ValueError, match="v_dtype"):
        DecoderLM(v_dtype="e4m3", device="cpu", max_length=1 << 40)


def test_full_attention_mode_ignores_v_dtype():
    """attn_mode='full' has no chunk table: v_dtype is validated, kept, and changes nothing of the KV_Cache."""
    from shadowkv_amd import llama
    from shadowkv_amd.kv_cache import KV_Cache
    cfg = llama.ModelConfig(name="tiny", hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2,
                            num_key_value_heads=1, vocab_size=100)
    kw = dict(cfg=cfg, batch_size=1, max_length=64, device="cpu", attn_mode="full", max_new_tokens=8)
    a, b = llama.DecoderLM(v_dtype="fp8_e4m3", **kw), llama.DecoderLM(v_dtype="bf16", **kw)
    assert a.v_dtype == "fp8_e4m3" and type(a.kv_cache) is KV_Cache and not hasattr(a.kv_cache, "v_scale")
    assert a.kv_cache.v_cache.dtype == b.kv_cache.v_cache.dtype == torch.bfloat16
    assert a.kv_cache.v_cache.shape == b.kv_cache.v_cache.shape and a.kv_cache.k_cache.shape == b.kv_cache.k_cache.shape
    with pytest.raises(ValueError, match="v_dtype"):
        llama.DecoderLM(v_dtype="fp8", **kw)


def test_refusals_name_v_dtype():
    a, _ = _build("llama_small", "fp8_e4m3")
    c = G.CASES["llama_small"]
    q = torch.zeros(1, c["q_heads"], 1, c["head_dim"], dtype=torch.bfloat16)
    cs = torch.zeros(16, 128, dtype=torch.bfloat16)
    a.reference_calls = True
    with pytest.raises(RuntimeError, match="v_dtype.*bf16 rows"):
        a.get_retrieval_position_ids(0, q)
    with pytest.raises(RuntimeError, match="v_dtype"):
        a.get_value_cache(0, a.position_ids[0])
    with pytest.raises(RuntimeError, match="v_dtype"):
        a.get_key_cache(0, a.position_ids[0], None, cs)
    a.reference_calls = False
    assert a.early_fetch_supported() is False and a.can_overlap_attention() is False
    for kw in (dict(), dict(early_max=8), dict(early_max=8, near=False)):
        with pytest.raises(RuntimeError, match="v_dtype"):
            a.enable_early_fetch(**kw)
    a.enable_early_fetch(early_max=0)                          # switching it off stays a no-op
    with pytest.raises(RuntimeError, match="v_dtype"):
        a.select_fetch_attend_inplace(0, q, cs, kv_len=a.sparse_end + 1)


# ---------------------------------------------------------------------------------------------------- C ABI
def test_new_symbols_are_exported_and_declared():
    import ctypes
    from shadowkv_amd import _lib
    text = open(os.path.join(ROOT, "include", "shadowkv_hip.h")).read()
    declared = set(re.findall(r"SKV_EXPORT\s+[\w\s\*]+?\b(skv_\w+)\s*\(", text))
    l = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared and hasattr(l, n) and n in _lib.EXPORTS, n


def test_new_entries_refuse_bad_arguments_before_any_launch():
    """-1 = SKV_ERR_ARG for a null table, a null scale and a misaligned stride; all on the host, no device needed."""
    from shadowkv_amd import _lib
    L = _lib.lib()
    p = 0x1000                                                 # non-null, 16-byte aligned, never dereferenced on the host

    def quant(v=p, st=1024, table=p, tstride=16 * 128, scale=p):
        return L.skv_quantize_v_rows(v, 8 * 1024, 128, st, 1, 8, 16, 128, table, tstride, scale, 16, 0)
    assert quant(table=0) == -1 and quant(scale=0) == -1 and quant(v=0) == -1
    assert quant(st=1028) == -1 and quant(tstride=16 * 128 + 4) == -1 and quant(v=p + 8) == -1
    assert quant(tstride=15 * 128) == -1                       # rows would overlap the next block

    def land(table=p, scale=p, hstride=256 * 1024, sstride=256 * 8):
        return L.skv_land_chunks_fp8(table, p, p, p, p, hstride, 512 * 128, 64 * 128, 8, 32, scale, sstride, 0)
    assert land(table=0) == -1 and land(scale=0) == -1 and land(hstride=256 * 1024 + 8) == -1 and land(sstride=256 * 8 + 4) == -1

    def fetch(table=p, scale=p, hstride=256 * 1024, sstride=256 * 8):
        return L.skv_fetch_kv_fp8(p, p, p, p, p, p, p, p, table, p, p, 1, 8, 2048, 128, 160, 32, 8, 128, 8 * 512 * 128, 512 * 128, 128,
                                  64, 1, hstride, scale, sstride, 0)
    assert fetch(table=0) == -1 and fetch(scale=0) == -1 and fetch(hstride=256 * 1024 + 8) == -1 and fetch(sstride=4) == -1

    def fetch_ip(table=p, scale=p, hstride=256 * 1024, sstride=256 * 8):
        return L.skv_fetch_kv_inplace_fp8(p, p, p, p, p, p, p, table, p, 1, 8, 2048, 128, 160, 32, 8, 128, 8 * 512 * 128, 512 * 128,
                                          128, 64, 1, hstride, scale, sstride, 0)
    assert fetch_ip(table=0) == -1 and fetch_ip(scale=0) == -1 and fetch_ip(hstride=256 * 1024 + 8) == -1 and fetch_ip(sstride=4) == -1
    # shapes the FP8 landing role is not built for: -2 = SKV_ERR_UNSUPPORTED, still before any launch
    assert L.skv_fetch_kv_inplace_fp8(p, p, p, p, p, p, p, p, p, 1, 8, 2048, 128, 128, 32, 8, 128, 8 * 512 * 128, 512 * 128, 128, 64, 1,
                                      256 * 1024, p, 256 * 8, 0) == -2                # rank 128
