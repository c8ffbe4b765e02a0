"""CPU: the FP8 (e4m3) landmark table - the cache built on a CPU device against the reference quantiser
(tests/fp8_v_ref.py: the landmark rows follow the V table's rule) and against its bf16 twin, the refusals, and the argument
checks of the new C entries (no device is touched)."""
import math
import os
import re

import pytest
import torch

import fp8_v_ref as R
import gen_inputs as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("skv_score_landmarks_fp8", "skv_score_landmarks_fused_fp8", "skv_select_chunks_fp8", "skv_select_chunks_inplace_fp8",
               "skv_select_chunks_fused_fp8")


# ---------------------------------------------------------------------------------------------------- the cache, CPU device
def _build(case, landmark_dtype, v_dtype="bf16"):
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    c, inp = G.CASES[case], G.make_inputs(case)
    cache = ShadowKVCache_CPU(G.config_of(case), batch_size=1, max_length=c["L"], device="cpu", dtype=torch.bfloat16,
                              sparse_budget=c["budget"], chunk_size=c["chunk"], rank=c["rank"], v_dtype=v_dtype,
                              landmark_dtype=landmark_dtype)
    cache.get_svd(inp["k_pre"], 0)
    k_roped = G.rope_torch(case, inp["k_pre"], inp["cos_sin"], torch.arange(c["L"]).unsqueeze(0))
    cache.prefill_kv_cache(inp["v"], 0, k_roped, inp["q_last"])
    return cache, [inp["q_last"]]


def _build_subbatched(case, landmark_dtype):
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    c = G.SUBBATCH_CASES[case]
    inputs = G.subbatch_inputs(case)
    cache = ShadowKVCache_CPU(G.config_of(case), batch_size=c["batch"], max_length=c["L"], device="cpu", dtype=torch.bfloat16,
                              sparse_budget=c["budget"], chunk_size=c["chunk"], rank=c["rank"], landmark_dtype=landmark_dtype)
    for i in range(0, c["batch"], c["sub"]):
        idx = list(range(i, i + c["sub"]))
        for l, inp in enumerate(inputs):
            cache.get_svd(inp["k_pre"][idx], l)
            cache.prefill_kv_cache(inp["v"][idx], l, inp["k_roped"][idx], inp["q_last"][idx])
    return cache, [inp["q_last"] for inp in inputs]


def initial_selection_over(lm, lm_idx, q_last, kv, G_, S):
    """The prefill-time selection restated in torch ops over bf16 landmark rows lm [bs, kv, N, D]: einsum / sqrt(128) -> f32
    softmax -> bf16 -> max over the group -> top-k -> chunk ids."""
    attn = torch.einsum("bhgd,bhcd->bhgc", q_last.view(-1, kv, G_, lm.shape[-1]), lm) / math.sqrt(128)
    attn = torch.nn.functional.softmax(attn, dim=-1, dtype=torch.float32).to(torch.bfloat16)
    top = torch.topk(attn.max(dim=-2).values, k=S, dim=-1).indices
    return lm_idx.gather(dim=-1, index=top)


def check_fp8_landmark_cache_against_reference_and_twin(a, b, q_layers, sub=None):
    """a: FP8-landmark cache, b: its bf16 twin (same prompt), q_layers: the last query per layer (CPU); sub: sequences per
    prefill call (the restated selection runs on the cache's device in the same sub-batches).  Shared with the GPU tests."""
    dev = a.k_cache_buffer.device
    kv, G_, S = a.num_key_value_heads, a.num_key_value_groups, a.select_sets
    assert a.k_landmark.dtype == torch.float8_e4m3fn and tuple(a.k_landmark.shape) == tuple(b.k_landmark.shape)
    assert a.k_landmark_scale.dtype == torch.float32 and tuple(a.k_landmark_scale.shape) == tuple(a.k_landmark.shape[:-1])
    assert a.k_landmark_scale.device == a.k_cache_buffer.device and b.k_landmark_scale is None
    assert b.k_landmark.dtype == torch.bfloat16
    for n in ("k_landmark_idx", "U", "SV"):
        assert torch.equal(getattr(a, n).cpu(), getattr(b, n).cpu()), n
    ta, tb = a.v_cache_cpu.cpu(), b.v_cache_cpu.cpu()
    assert torch.equal(ta.view(torch.uint8) if ta.element_size() == 1 else ta.view(torch.int16),
                       tb.view(torch.uint8) if tb.element_size() == 1 else tb.view(torch.int16)), "the V table is untouched"
    assert a.sparse_start == b.sparse_start and a.sparse_end == b.sparse_end
    for l, q_last in enumerate(q_layers):
        want_b, want_s = R.quantize_rows(b.k_landmark[l].cpu())
        table, scale = a.k_landmark[l].cpu().view(torch.uint8), a.k_landmark_scale[l].cpu()
        assert torch.equal(table, want_b), f"layer {l}: landmark bytes"
        assert torch.equal(scale, want_s), f"layer {l}: landmark scales"
        assert not bool(((table & 0x7F) == 0x7F).any())
        for buf in ("k_cache_buffer", "v_cache_buffer"):                 # local rows and outlier chunks: exact, as the twin's
            xa, xb = getattr(a, buf)[l].cpu(), getattr(b, buf)[l].cpu()
            assert torch.equal(xa[:, :, :a.sparse_start].view(torch.int16), xb[:, :, :a.sparse_start].view(torch.int16)), buf
        deq = R.dequantize_rows(table, scale)[0]
        assert torch.equal(a.landmarks_bf16(l).cpu().view(torch.int16), deq.view(torch.int16))
        bs = deq.shape[0]
        step = bs if sub is None else sub
        want = torch.cat([initial_selection_over(deq[i:i + step].to(dev), a.k_landmark_idx[l][i:i + step], q_last[i:i + step].to(dev),
                                                 kv, G_, S) for i in range(0, bs, step)])
        assert torch.equal(a.position_ids[l][..., :S], want), f"layer {l}: initial selection != selection over dequant(table)"


def test_cpu_cache_matches_the_reference_and_its_bf16_twin():
    a, q = _build("llama_small", "fp8_e4m3")
    b, _ = _build("llama_small", "bf16")
    check_fp8_landmark_cache_against_reference_and_twin(a, b, q)


def test_cpu_cache_subbatched_prefill():
    a, q = _build_subbatched("subbatch_llama", "fp8_e4m3")
    b, _ = _build_subbatched("subbatch_llama", "bf16")
    assert a.prefilled_batch == G.SUBBATCH_CASES["subbatch_llama"]["batch"]
    check_fp8_landmark_cache_against_reference_and_twin(a, b, q, sub=G.SUBBATCH_CASES["subbatch_llama"]["sub"])


def test_composes_with_the_fp8_v_table():
    a, q = _build("llama_small", "fp8_e4m3", v_dtype="fp8_e4m3")
    b, _ = _build("llama_small", "bf16", v_dtype="fp8_e4m3")
    assert a.v_scale is not None and torch.equal(a.v_scale, b.v_scale)
    check_fp8_landmark_cache_against_reference_and_twin(a, b, q)


def test_default_changes_nothing_and_clear_drops_the_scale():
    from shadowkv_amd import tensor_op
    assert tensor_op.LANDMARK_DTYPES == ("bf16", "fp8_e4m3")
    b, _ = _build("llama_small", "bf16")
    assert b.landmark_dtype == "bf16" and b.k_landmark_scale is None and b.landmarks_bf16(0).data_ptr() == b.k_landmark[0].data_ptr()
    a, _ = _build("llama_small", "fp8_e4m3")
    assert a._layer(0).lmscale.data_ptr() == a.k_landmark_scale[0].data_ptr() and b._layer(0).lmscale is None
    a.clear()
    assert a.k_landmark is None and a.k_landmark_scale is None and a.landmark_dtype == "fp8_e4m3"


# ---------------------------------------------------------------------------------------------------- refusals
def test_bad_landmark_dtype_is_refused_before_any_allocation():
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    from shadowkv_amd.llama import DecoderLM
    c = G.CASES["llama_small"]
    with pytest.raises(ValueError, match="landmark_dtype"):
        ShadowKVCache_CPU(G.config_of("llama_small"), batch_size=1, max_length=1 << 40, device="cpu", sparse_budget=c["budget"],
                          landmark_dtype="fp8")               # (a table of this size could not be allocated)
    with pytest.raises(ValueError, match="landmark_dtype"):
        DecoderLM(landmark_dtype="e4m3", device="cpu", max_length=1 << 40)


def test_full_attention_mode_ignores_landmark_dtype():
    """attn_mode='full' has no landmarks: landmark_dtype is validated, kept, and changes nothing of the KV_Cache."""
    from shadowkv_amd import llama
    from shadowkv_amd.kv_cache import KV_Cache
    cfg = llama.ModelConfig(name="tiny", hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2,
                            num_key_value_heads=1, vocab_size=100)
    kw = dict(cfg=cfg, batch_size=1, max_length=64, device="cpu", attn_mode="full", max_new_tokens=8)
    a, b = llama.DecoderLM(landmark_dtype="fp8_e4m3", **kw), llama.DecoderLM(**kw)
    assert a.landmark_dtype == "fp8_e4m3" and b.landmark_dtype == "bf16" and type(a.kv_cache) is KV_Cache
    assert not hasattr(a.kv_cache, "k_landmark_scale")
    assert a.kv_cache.k_cache.dtype == b.kv_cache.k_cache.dtype and a.kv_cache.k_cache.shape == b.kv_cache.k_cache.shape
    with pytest.raises(ValueError, match="landmark_dtype"):
        llama.DecoderLM(landmark_dtype="fp8", **kw)


def test_reference_calls_refusal_names_landmark_dtype_and_leaves_the_cache_unchanged():
    a, _ = _build("llama_small", "fp8_e4m3")
    c = G.CASES["llama_small"]
    q = torch.ones(1, c["q_heads"], 1, c["head_dim"], dtype=torch.bfloat16)
    cs = torch.zeros(16, 128, dtype=torch.bfloat16)
    names = ("k_landmark_scale", "k_landmark_idx", "position_ids", "k_cache_buffer", "v_cache_buffer", "offsets", "_cnts_layers")
    before = {n: getattr(a, n).clone() for n in names}
    lm_before = a.k_landmark.view(torch.uint8).clone()
    a.reference_calls = True
    with pytest.raises(RuntimeError, match="landmark_dtype.*bf16 table"):
        a.get_retrieval_position_ids(0, q)
    with pytest.raises(RuntimeError, match="landmark_dtype"):
        a.get_value_cache(0, a.position_ids[0])
    with pytest.raises(RuntimeError, match="landmark_dtype"):
        a.get_key_cache(0, a.position_ids[0], None, cs)
    for n in names:
        assert torch.equal(getattr(a, n), before[n]), n
    assert torch.equal(a.k_landmark.view(torch.uint8), lm_before)
    assert a.gemm_o is None                                   # (not even the reference's scratch was allocated)


# ---------------------------------------------------------------------------------------------------- C ABI
def test_new_symbols_are_exported_and_declared():
    import ctypes
    from shadowkv_amd import _lib
    text = open(os.path.join(ROOT, "include", "shadowkv_hip.h")).read()
    declared = set(re.findall(r"SKV_EXPORT\s+[\w\s\*]+?\b(skv_\w+)\s*\(", text))
    l = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared and hasattr(l, n) and n in _lib.EXPORTS, n
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert l.skv_abi_version() == 1


def test_new_entries_refuse_a_null_table_or_scale_before_any_launch():
    """-1 = SKV_ERR_ARG for a null table and a null scale, on the host (no device needed); a shape the bf16 entry refuses gets
    the bf16 entry's code."""
    from shadowkv_amd import _lib
    L = _lib.lib()
    p = 0x1000                                                 # non-null, 16-byte aligned, never dereferenced on the host

    def score(table=p, scale=p, n=1000):
        return L.skv_score_landmarks_fp8(p, table, scale, p, p, p, 8, 4, n, 1.0, 0)
    assert score(table=0) == -1 and score(scale=0) == -1 and score(n=0) == -1
    assert score(n=0) == L.skv_score_landmarks(p, p, p, p, p, 8, 4, 0, 1.0, 0)

    def score_fused(table=p, scale=p, groups=4):
        return L.skv_score_landmarks_fused_fp8(p, table, scale, p, p, 8, groups, 1000, 1.0, p, 0, 0, 0, 0)
    assert score_fused(table=0) == -1 and score_fused(scale=0) == -1
    assert score_fused(groups=2) == L.skv_score_landmarks_fused(p, p, p, p, 8, 2, 1000, 1.0, p, 0, 0, 0, 0) == -2

    def select(table=p, scale=p, S=32):
        return L.skv_select_chunks_fp8(p, table, scale, p, p, p, p, p, 0, 0, 8, 4, 1000, S, 1.0, 0)
    assert select(table=0) == -1 and select(scale=0) == -1
    assert select(S=2000) == L.skv_select_chunks(p, p, p, p, p, p, p, 0, 0, 8, 4, 1000, 2000, 1.0, 0) == -1

    def inplace(table=p, scale=p, R_=32):
        return L.skv_select_chunks_inplace_fp8(p, table, scale, p, p, p, p, p, p, 0, 0, 8, 4, 1000, 32, R_, p, 1.0, 0)
    assert inplace(table=0) == -1 and inplace(scale=0) == -1
    assert inplace(R_=16) == L.skv_select_chunks_inplace(p, p, p, p, p, p, p, p, 0, 0, 8, 4, 1000, 32, 16, p, 1.0, 0) == -1

    def fused(table=p, scale=p, groups=4, state=p):
        return L.skv_select_chunks_fused_fp8(p, table, scale, p, p, p, p, p, p, 0, 8, groups, 1000, 32, 32, p, 1.0, state, 0, 0, 0, 0,
                                             0, 0.0, None, 0)
    assert fused(table=0) == -1 and fused(scale=0) == -1 and fused(state=0) == -1
    assert fused(groups=2) == L.skv_select_chunks_fused(p, p, p, p, p, p, p, p, 0, 8, 2, 1000, 32, 32, p, 1.0, p, 0, 0, 0, 0, 0, 0.0,
                                                        0) == -2
