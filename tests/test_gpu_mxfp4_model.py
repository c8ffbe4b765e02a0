"""GPU: DecoderLM with weight-only MXFP4 weights (e2m1 nibbles + e8m0 block scales) against a bf16 model that holds the SAME
numbers.

Model A is the seed-s model after quantize_weights(dtype="mxfp4").  Model B is the bf16 model of the same seed whose matrices
are overwritten with dequantize_mxfp4_rows of A's - exact, because a power of two times an e2m1 value is a bf16 number (the
f64 restatement of tests/mxfp4_ref.py is the witness).
The two models hold mathematically identical weights; the same walk table is passed as q_table, so the chunk selection does
not depend on the weights.  What separates their logits is the order of f32 sums: the bound is the 2e-2 relative norm the
project uses for two such paths of one model (tests/test_gpu_graph.py, the in-place against the reference layout)."""
import numpy as np
import pytest
import torch

import mxfp4_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2e-2
MATRICES = ("wqkv", "wo", "gate_up_proj", "down_proj")


def _cfg(name):
    from shadowkv_amd import llama
    if name == "tiny":          # the config of tests/test_gpu_graph.py::_make: hidden 1024 (norm + GEMV as two launches)
        return llama.ModelConfig(name="tiny", hidden_size=1024, intermediate_size=2048, num_hidden_layers=2,
                                 num_attention_heads=8, num_key_value_heads=2, vocab_size=2000)
    # hidden 4096: the one-launch norm paths (QKV with RoPE / cache push, gate/up, lm_head with range keys)
    return llama.ModelConfig(name="h4096", hidden_size=4096, intermediate_size=1024, num_hidden_layers=2,
                             num_attention_heads=32, num_key_value_heads=8, vocab_size=4096)


def _make(cfg="tiny", mx=False, seed=5, layout="inplace", overlap=True, batch=1, context=True, max_length=4608, **kw):
    from shadowkv_amd import llama
    m = llama.DecoderLM(cfg=_cfg(cfg), batch_size=batch, max_length=max_length, device=DEV, sparse_budget=256, rank=160,
                        chunk_size=8, seed=seed, chunk_layout=layout, overlap_attention=overlap, **kw)
    if mx:
        m.quantize_weights(dtype="mxfp4")
    if context:
        llama.build_synthetic_context(m, 4608, seed=77)
    return m, llama


def _pair(**kw):
    """(A, B, llama): the MXFP4 model and the bf16 model holding the same numbers"""
    from shadowkv_amd import tensor_op
    a, llama = _make(mx=True, **kw)
    b, _ = _make(mx=False, **kw)

    def exact(w4, sc):
        deq = tensor_op.dequantize_mxfp4_rows(w4, sc)
        rows = slice(0, 64)                                 # the f64 restatement over the first rows: exact in bf16
        assert np.array_equal(deq[rows].double().cpu().numpy(), mr.decode(w4[rows], sc[rows]))
        assert torch.equal(deq.float(), tensor_op.dequantize_mxfp4_rows(w4, sc, dtype=torch.float32))       # every row
        return deq

    for la, lb in zip(a.layers, b.layers):
        for name in MATRICES:
            getattr(lb, name).copy_(exact(getattr(la, name), getattr(la, name + "_scale")))
    b.lm_head.copy_(exact(a.lm_head, a.lm_head_scale))
    assert a.weight_dtype == "mxfp4" and b.weight_dtype == "bf16"
    return a, b, llama


def _step(m, tok, q_table):
    c = m.kv_cache
    row = c.sparse_end + c.gen_offset
    lg = m.forward_fused(tok, m.get_ctx(tok), torch.tensor([row], device=DEV), kv_len=row + 1, q_table=q_table)
    c.note_kv_appended(1)
    return lg[:, -1]


def _rel(x, y):
    return float((x.float() - y.float()).norm() / y.float().norm())


@pytest.mark.parametrize("cfg", ["tiny", "h4096"])
def test_mxfp4_model_decodes_like_the_bf16_model_with_the_same_numbers(cfg):
    from shadowkv_amd import tensor_op
    steps = 6
    a, b, llama = _pair(cfg=cfg)
    table = llama.make_walk_table(b, steps, seed=3)
    tok = torch.tensor([[17]], device=DEV)
    n0, f0 = tensor_op.mxfp4_native_calls, tensor_op.mxfp4_fallback_calls
    for i in range(steps):
        la, lb = _step(a, tok, table[i]), _step(b, tok, table[i])
        torch.cuda.synchronize()
        assert torch.equal(a.kv_cache.position_ids, b.kv_cache.position_ids), i
        rel = _rel(la, lb)
        print(f"{cfg} step {i}: |logits_A - logits_B| / |logits_B| = {rel:.3e}")
        assert rel < BOUND, (i, rel)
        tok = lb.argmax(dim=-1, keepdim=True)            # both models are fed B's greedy tokens
    # every dense launch of A was a native MXFP4 launch: 4 per layer + the lm_head, per step
    assert tensor_op.mxfp4_native_calls - n0 == steps * (4 * a.num_layers + 1) and tensor_op.mxfp4_fallback_calls == f0
    # MXFP4 models take the one QKV launch (the k/v role of the selection launch reads bf16 rows); both counters keep counting
    assert a.kv_proj_split_launches == 0 and a.kv_proj_fused_launches == steps * a.num_layers
    assert b.kv_proj_split_launches + b.kv_proj_fused_launches == steps * b.num_layers


@pytest.mark.parametrize("cfg", ["tiny", "h4096"])
def test_reference_call_order_takes_the_mxfp4_launches(cfg):
    """decode_step(fused=False) - inference -> layer_compute -> pre_attention_compute / post_attention_compute - on the MXFP4
    model: native launches only, and logits within the bound of the fused step's (same query walk in both)."""
    from shadowkv_amd import tensor_op
    m1, llama = _make(cfg=cfg, mx=True, layout="reference", overlap=False)
    m2, _ = _make(cfg=cfg, mx=True, layout="reference", overlap=False)
    tok = torch.tensor([[23]], device=DEV)
    walk = llama.QueryWalk(m1, step=0.3, seed=3)
    walk.advance()
    m1.query_hook = walk
    pos = m1.get_ctx(tok)
    n0, f0 = tensor_op.mxfp4_native_calls, tensor_op.mxfp4_fallback_calls
    la = m1.inference(tok, pos)
    assert tensor_op.mxfp4_native_calls - n0 == 4 * m1.num_layers + 1 and tensor_op.mxfp4_fallback_calls == f0
    row = m2.kv_cache.sparse_end + m2.kv_cache.gen_offset
    lb = m2.forward_fused(tok, pos, torch.tensor([row], device=DEV), kv_len=row + 1, q_table=walk.qb)
    torch.cuda.synchronize()
    assert torch.equal(m1.kv_cache.position_ids.sort(dim=-1).values, m2.kv_cache.position_ids.sort(dim=-1).values)
    rel = _rel(la[:, -1], lb[:, -1])
    print(f"{cfg}: reference call order against the fused step: {rel:.3e}")
    assert rel < BOUND, rel
    n1 = tensor_op.mxfp4_native_calls
    t = m1.decode_step(tok, temperature=0.0, fused=False)
    assert t.shape == (1, 1) and tensor_op.mxfp4_native_calls - n1 == 4 * m1.num_layers + 1 and tensor_op.mxfp4_fallback_calls == f0


def _tap(m):
    """keeps the logits of the model's last forward_fused call (the captured graph's static output included)"""
    box, orig = {}, m.forward_fused

    def ff(*a, **k):
        box["logits"] = orig(*a, **k)
        return box["logits"]

    m.forward_fused = ff
    return box


@pytest.mark.parametrize("cfg", ["tiny", "h4096"])
def test_graph_decoder_captures_the_mxfp4_step(cfg):
    warm, steps = 2, 6
    m1, llama = _make(cfg=cfg, mx=True)
    m2, _ = _make(cfg=cfg, mx=True)
    table = llama.make_walk_table(m1, warm + steps, seed=3)
    tok0 = torch.tensor([[17]], device=DEV)
    b1, b2 = _tap(m1), _tap(m2)
    t, toks1 = tok0.clone(), []
    for i in range(warm + steps):
        t = m1.decode_step(t, temperature=0.0, q_table=table[i])
        toks1.append(int(t))
    dec = llama.GraphDecoder(m2, temperature=0.0, walk_table=table)
    dec.token.copy_(tok0)
    assert dec.capture(warmup=warm) == warm
    toks2 = [int(dec.step()) for _ in range(steps)]
    torch.cuda.synchronize()
    assert toks2 == toks1[warm:], (toks1, toks2)
    assert torch.equal(b1["logits"].view(torch.int16), b2["logits"].view(torch.int16))
    assert torch.equal(m1.kv_cache.position_ids, m2.kv_cache.position_ids)
    assert torch.equal(m1.kv_cache.k_cache_buffer.view(torch.int16), m2.kv_cache.k_cache_buffer.view(torch.int16))


def test_generate_prefills_through_the_dequantising_path():
    kw = dict(cfg="tiny", layout="reference", overlap=False, context=False, max_length=5120, max_new_tokens=64)
    a, b, _ = _pair(**kw)
    ids = torch.randint(0, 2000, (1, 4700), generator=torch.Generator().manual_seed(3)).to(DEV)
    la, lb = a.prefill(ids), b.prefill(ids)
    torch.cuda.synchronize()
    rel = _rel(la[:, -1], lb[:, -1])
    print(f"prefill logits, MXFP4 model against the bf16 model with the same numbers: {rel:.3e}")
    assert rel < BOUND, rel
    assert a.layers[0].wqkv.dtype == torch.uint8          # the temporaries were temporaries
    gen_len = 4
    out = a.generate(ids, gen_len, temperature=0.0)
    assert out.shape == (1, 1 + gen_len) and out.dtype == torch.long and int(out.min()) >= 0 and int(out.max()) < 2000
    # generate(graph=True): the captured decode against the eager one, same prompt, same greedy tokens
    a2, _ = _make(mx=True, **kw)
    out_g = a2.generate(ids, gen_len, temperature=0.0, graph=True)
    torch.cuda.synchronize()
    assert torch.equal(out_g, out), (out_g.tolist(), out.tolist())
    assert torch.equal(a.kv_cache.position_ids, a2.kv_cache.position_ids)


def test_batch_of_two_falls_back_and_agrees():
    """bs = 2: the MXFP4 kernels take one token row, so every dense op dequantises and calls F.linear - correct, not fast."""
    from shadowkv_amd import tensor_op
    a, b, llama = _pair(cfg="tiny", layout="reference", overlap=False, batch=2)
    table = llama.make_walk_table(b, 1, seed=3)
    tok = torch.tensor([[17], [40]], device=DEV)
    f0 = tensor_op.mxfp4_fallback_calls
    la, lb = _step(a, tok, table[0]), _step(b, tok, table[0])
    torch.cuda.synchronize()
    assert tensor_op.mxfp4_fallback_calls - f0 == 4 * a.num_layers + 1
    assert torch.equal(a.kv_cache.position_ids, b.kv_cache.position_ids)
    rel = _rel(la, lb)
    print(f"bs 2 fallback: {rel:.3e}")
    assert rel < BOUND, rel


def test_mxfp4_weights_with_an_fp8_v_table_and_with_full_attention():
    """weight_dtype="mxfp4" composes with v_dtype="fp8_e4m3" (the V offload table as e4m3 bytes) and with attn_mode="full":
    each against its own twin - the bf16-weight model with the same numbers and the same cache settings."""
    from shadowkv_amd import tensor_op
    steps = 3
    a, b, llama = _pair(cfg="h4096", v_dtype="fp8_e4m3")
    assert a.v_dtype == "fp8_e4m3" and b.v_dtype == "fp8_e4m3"
    table = llama.make_walk_table(b, steps, seed=3)
    tok = torch.tensor([[17]], device=DEV)
    n0, f0 = tensor_op.mxfp4_native_calls, tensor_op.mxfp4_fallback_calls
    for i in range(steps):
        la, lb = _step(a, tok, table[i]), _step(b, tok, table[i])
        torch.cuda.synchronize()
        assert torch.equal(a.kv_cache.position_ids, b.kv_cache.position_ids), i
        rel = _rel(la, lb)
        print(f"fp8 V table, step {i}: {rel:.3e}")
        assert rel < BOUND, (i, rel)
        tok = lb.argmax(dim=-1, keepdim=True)
    assert tensor_op.mxfp4_native_calls - n0 == steps * (4 * a.num_layers + 1) and tensor_op.mxfp4_fallback_calls == f0
    kw = dict(cfg="h4096", context=False, max_length=512, max_new_tokens=16, attn_mode="full")
    a, b, _ = _pair(**kw)
    ids = torch.randint(0, 4096, (1, 300), generator=torch.Generator().manual_seed(5)).to(DEV)
    la, lb = a.prefill(ids), b.prefill(ids)
    rel = _rel(la[:, -1], lb[:, -1])
    print(f"full attention, prefill: {rel:.3e}")
    assert rel < BOUND, rel
    n0 = tensor_op.mxfp4_native_calls
    tok = lb[:, -1].argmax(dim=-1, keepdim=True)
    ta, tb = a.decode_step(tok, temperature=0.0), b.decode_step(tok, temperature=0.0)
    torch.cuda.synchronize()
    assert ta.shape == (1, 1) and tb.shape == (1, 1)
    assert tensor_op.mxfp4_native_calls - n0 == 4 * a.num_layers + 1 and tensor_op.mxfp4_fallback_calls == f0
