"""GPU: DecoderLM with FP8 (e4m3) weights and fp8_rows="native" at 2 and 17 sequences, against a bf16 model that holds the SAME
numbers (the construction of tests/test_gpu_fp8_model.py: power-of-two scales, so the dequantised matrices are exact in bf16).
Every dense op of a batched step is then one skv_linear_rows_fp8 launch - no dequantising call is left - and the logits stay
within the project's 2e-2 relative norm of the bf16 model's.  The default (no option) still takes the fallback."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2e-2
MATRICES = ("wqkv", "wo", "gate_up_proj", "down_proj")
STEPS = 3


def _cfg(name):
    from shadowkv_amd import llama
    if name == "tiny":          # the config of tests/test_gpu_graph.py::_make: hidden 1024 (norm + GEMV as two launches)
        return llama.ModelConfig(name="tiny", hidden_size=1024, intermediate_size=2048, num_hidden_layers=2,
                                 num_attention_heads=8, num_key_value_heads=2, vocab_size=2000)
    # hidden 4096: the one-launch norm paths (QKV with RoPE / cache push, gate/up, lm_head with range keys)
    return llama.ModelConfig(name="h4096", hidden_size=4096, intermediate_size=1024, num_hidden_layers=2,
                             num_attention_heads=32, num_key_value_heads=8, vocab_size=4096)


def _make(cfg="tiny", fp8=False, seed=5, layout="inplace", overlap=True, batch=1, context=True, max_length=4608, **kw):
    from shadowkv_amd import llama
    m = llama.DecoderLM(cfg=_cfg(cfg), batch_size=batch, max_length=max_length, device=DEV, sparse_budget=256, rank=160,
                        chunk_size=8, seed=seed, chunk_layout=layout, overlap_attention=overlap, **kw)
    if fp8:
        m.quantize_weights(pow2_scale=True)
    if context:
        llama.build_synthetic_context(m, 4608, seed=77)
    return m, llama


def _pair(**kw):
    """(A, B, llama): the FP8 model and the bf16 model holding the same numbers"""
    from shadowkv_amd import tensor_op
    a, llama = _make(fp8=True, **kw)
    b, _ = _make(fp8=False, **kw)
    for la, lb in zip(a.layers, b.layers):
        for name in MATRICES:
            deq = tensor_op.dequantize_fp8_rows(getattr(la, name), getattr(la, name + "_scale"))
            assert torch.equal(deq.float(), getattr(la, name).float() * getattr(la, name + "_scale").unsqueeze(1))   # exact in bf16
            getattr(lb, name).copy_(deq)
    b.lm_head.copy_(tensor_op.dequantize_fp8_rows(a.lm_head, a.lm_head_scale))
    assert a.weight_dtype == "fp8_e4m3" and b.weight_dtype == "bf16"
    return a, b, llama


def _step(m, tok, q_table):
    c = m.kv_cache
    row = c.sparse_end + c.gen_offset
    lg = m.forward_fused(tok, m.get_ctx(tok), torch.tensor([row], device=DEV), kv_len=row + 1, q_table=q_table)
    c.note_kv_appended(1)
    return lg[:, -1]


def _rel(x, y):
    return float((x.float() - y.float()).norm() / y.float().norm())


def _tokens(batch):
    return (17 + 23 * torch.arange(batch, device=DEV)).view(batch, 1)


@pytest.mark.parametrize("batch", [2, 17])
@pytest.mark.parametrize("cfg", ["tiny", "h4096"])
def test_native_fp8_rows_model_decodes_like_the_bf16_model_with_the_same_numbers(cfg, batch):
    from shadowkv_amd import tensor_op
    a, b, llama = _pair(cfg=cfg, layout="reference", overlap=False, batch=batch, fp8_rows="native")
    assert a.fp8_rows == "native" and b.fp8_rows == "native"            # (inert on the bf16 model)
    table = llama.make_walk_table(b, STEPS, seed=3)
    tok = _tokens(batch)
    n0, f0 = tensor_op.fp8_native_calls, tensor_op.fp8_fallback_calls
    for i in range(STEPS):
        la, lb = _step(a, tok, table[i]), _step(b, tok, table[i])
        torch.cuda.synchronize()
        assert torch.equal(a.kv_cache.position_ids, b.kv_cache.position_ids), i
        rel = _rel(la, lb)
        print(f"{cfg} bs {batch} step {i}: |logits_A - logits_B| / |logits_B| = {rel:.3e}")
        assert rel < BOUND, (i, rel)
        tok = lb.argmax(dim=-1, keepdim=True)            # both models are fed B's greedy tokens
    # every dense op of A was a native FP8 launch: 4 per layer + the lm_head, per step; nothing was dequantised
    assert tensor_op.fp8_native_calls - n0 == STEPS * (4 * a.num_layers + 1)
    assert tensor_op.fp8_fallback_calls == f0


@pytest.mark.parametrize("batch", [2, 17])
@pytest.mark.parametrize("cfg", ["tiny", "h4096"])
def test_reference_call_order_takes_the_native_fp8_rows_launches(cfg, batch):
    """decode_step(fused=False) - inference -> layer_compute -> pre_attention_compute / post_attention_compute: the same bound,
    selection and counters, the two models on the same query walk."""
    from shadowkv_amd import tensor_op
    a, b, llama = _pair(cfg=cfg, layout="reference", overlap=False, batch=batch, fp8_rows="native")
    for m in (a, b):
        m.query_hook = llama.QueryWalk(m, step=0.3, seed=3)
    tok = _tokens(batch)
    n0, f0 = tensor_op.fp8_native_calls, tensor_op.fp8_fallback_calls
    for i in range(STEPS - 1):
        a.query_hook.advance()
        b.query_hook.advance()
        la, lb = a.inference(tok, a.get_ctx(tok))[:, -1], b.inference(tok, b.get_ctx(tok))[:, -1]
        torch.cuda.synchronize()
        assert torch.equal(a.kv_cache.position_ids, b.kv_cache.position_ids), i
        rel = _rel(la, lb)
        print(f"{cfg} bs {batch} reference call order, step {i}: {rel:.3e}")
        assert rel < BOUND, (i, rel)
        tok = lb.argmax(dim=-1, keepdim=True)
    t = a.decode_step(tok, temperature=0.0, fused=False)
    assert t.shape == (batch, 1)
    assert tensor_op.fp8_native_calls - n0 == STEPS * (4 * a.num_layers + 1)
    assert tensor_op.fp8_fallback_calls == f0


def test_a_model_without_the_option_still_falls_back_at_batch_two():
    from shadowkv_amd import tensor_op
    a, _ = _make(cfg="tiny", fp8=True, layout="reference", overlap=False, batch=2)
    assert a.fp8_rows == "fallback"
    tok = _tokens(2)
    n0, f0 = tensor_op.fp8_native_calls, tensor_op.fp8_fallback_calls
    for i in range(2):
        _step(a, tok, None)
    torch.cuda.synchronize()
    assert tensor_op.fp8_fallback_calls - f0 == 2 * (4 * a.num_layers + 1) and tensor_op.fp8_native_calls == n0
