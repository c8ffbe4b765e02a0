"""GPU: DecoderLM with MXFP4 weights and mxfp4_rows="native" at 2 and 17 sequences, against a bf16 model that holds the SAME
numbers (the construction of tests/test_gpu_mxfp4_model.py: a power of two times an e2m1 value is a bf16 number, so the
dequantised matrices are exact).  Every dense op of a batched step is then one skv_linear_rows_mxfp4 launch - no dequantising
call is left - and the logits stay within the project's 2e-2 relative norm of the bf16 model's.  The default (no option) still
takes the fallback; an FP8 model does not read the option."""
import pytest
import torch

from test_gpu_mxfp4_model import BOUND, DEV, _make, _pair, _rel, _step

pytestmark = pytest.mark.gpu
STEPS = 3


def _tokens(batch):
    return (17 + 23 * torch.arange(batch, device=DEV)).view(batch, 1)


@pytest.mark.parametrize("batch", [2, 17])
@pytest.mark.parametrize("cfg", ["tiny", "h4096"])
def test_native_mxfp4_rows_model_decodes_like_the_bf16_model_with_the_same_numbers(cfg, batch):
    from shadowkv_amd import tensor_op
    a, b, llama = _pair(cfg=cfg, layout="reference", overlap=False, batch=batch, mxfp4_rows="native")
    assert a.mxfp4_rows == "native" and b.mxfp4_rows == "native"        # (inert on the bf16 model)
    table = llama.make_walk_table(b, STEPS, seed=3)
    tok = _tokens(batch)
    n0, f0 = tensor_op.mxfp4_native_calls, tensor_op.mxfp4_fallback_calls
    for i in range(STEPS):
        la, lb = _step(a, tok, table[i]), _step(b, tok, table[i])
        torch.cuda.synchronize()
        assert torch.equal(a.kv_cache.position_ids, b.kv_cache.position_ids), i
        rel = _rel(la, lb)
        print(f"{cfg} bs {batch} step {i}: |logits_A - logits_B| / |logits_B| = {rel:.3e}")
        assert rel < BOUND, (i, rel)
        tok = lb.argmax(dim=-1, keepdim=True)            # both models are fed B's greedy tokens
    # every dense op of A was a native MXFP4 launch: 4 per layer + the lm_head, per step; nothing was dequantised
    assert tensor_op.mxfp4_native_calls - n0 == STEPS * (4 * a.num_layers + 1)
    assert tensor_op.mxfp4_fallback_calls == f0


@pytest.mark.parametrize("batch", [2, 17])
@pytest.mark.parametrize("cfg", ["tiny", "h4096"])
def test_reference_call_order_takes_the_native_mxfp4_rows_launches(cfg, batch):
    """decode_step(fused=False) - inference -> layer_compute -> pre_attention_compute / post_attention_compute: the same bound,
    selection and counters, the two models on the same query walk."""
    from shadowkv_amd import tensor_op
    a, b, llama = _pair(cfg=cfg, layout="reference", overlap=False, batch=batch, mxfp4_rows="native")
    for m in (a, b):
        m.query_hook = llama.QueryWalk(m, step=0.3, seed=3)
    tok = _tokens(batch)
    n0, f0 = tensor_op.mxfp4_native_calls, tensor_op.mxfp4_fallback_calls
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
    assert tensor_op.mxfp4_native_calls - n0 == STEPS * (4 * a.num_layers + 1)
    assert tensor_op.mxfp4_fallback_calls == f0


def test_a_model_without_the_option_still_falls_back_at_batch_two():
    from shadowkv_amd import tensor_op
    a, _ = _make(cfg="tiny", mx=True, layout="reference", overlap=False, batch=2)
    assert a.mxfp4_rows == "fallback"
    tok = _tokens(2)
    n0, f0 = tensor_op.mxfp4_native_calls, tensor_op.mxfp4_fallback_calls
    for i in range(2):
        _step(a, tok, None)
    torch.cuda.synchronize()
    assert tensor_op.mxfp4_fallback_calls - f0 == 2 * (4 * a.num_layers + 1) and tensor_op.mxfp4_native_calls == n0


def test_an_fp8_model_does_not_read_the_option():
    """FP8 weights with mxfp4_rows="native": the same logits, bit for bit, and the same FP8 counters as without it."""
    from shadowkv_amd import llama, tensor_op
    logits, counts = [], []
    for kw in ({}, {"mxfp4_rows": "native"}):
        m, _ = _make(cfg="tiny", layout="reference", overlap=False, batch=2, fp8_rows="native", **kw)
        m.quantize_weights(pow2_scale=True)
        table = llama.make_walk_table(m, 1, seed=3)
        n0, f0 = tensor_op.fp8_native_calls, tensor_op.fp8_fallback_calls
        m0 = tensor_op.mxfp4_native_calls, tensor_op.mxfp4_fallback_calls
        logits.append(_step(m, _tokens(2), table[0]))
        torch.cuda.synchronize()
        counts.append((tensor_op.fp8_native_calls - n0, tensor_op.fp8_fallback_calls - f0))
        assert (tensor_op.mxfp4_native_calls, tensor_op.mxfp4_fallback_calls) == m0
    assert counts[0] == counts[1] == (4 * m.num_layers + 1, 0)
    assert torch.equal(logits[0].view(torch.int16), logits[1].view(torch.int16))
