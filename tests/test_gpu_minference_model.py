"""GPU: DecoderLM(minference=True) on the tiny NeoX and GLM configs of tests/test_gpu_prefill_model.py (~4,700-token prompts):
a full-coverage pattern reproduces the dense prefill, sparse patterns run generate() eagerly and from a captured graph, a
full-mode prefill_cont chunk keeps the dense kernel, and block_sparse is refused before any layer runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROMPT = 4700
LOGIT_BOUND = 0.02     # max |logit difference| relative to max |logit|, as in tests/test_gpu_prefill_model.py
FULL = [{h: ("vertical_and_slash", 30, 1 << 20, 1) for h in range(8)},          # slash = every offset: dense causal
        {h: ("stream_llm", 1, 8192, 1) for h in range(8)}]                    # the local window spans the prompt
SPARSE = [{h: ("stream_llm", 64, 512, 1) if h % 2 else ("vertical_and_slash", 100, 300, 1) for h in range(8)},
          {h: ("vertical_and_slash", 40 + h, 120, 1) for h in range(8)}]


def _make(glm=False, attn_mode="shadowkv_cpu", minference=False, pattern=None):
    from shadowkv_amd import llama
    cfg = llama.ModelConfig(name="tiny", hidden_size=1024, intermediate_size=2048, num_hidden_layers=2,
                            num_attention_heads=8, num_key_value_heads=2, vocab_size=2000,
                            qkv_bias=glm, rope_style="glm" if glm else "neox")
    return llama.DecoderLM(cfg=cfg, batch_size=1, max_length=5120, device=DEV, sparse_budget=256, rank=160, chunk_size=8,
                           seed=5, attn_mode=attn_mode, max_new_tokens=64, minference=minference,
                           minference_pattern=pattern)


def _ids(n, seed=3):
    return torch.randint(0, 2000, (1, n), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize("attn_mode", ["shadowkv_cpu", "full"])
@pytest.mark.parametrize("glm", [False, True])
def test_full_coverage_matches_dense_prefill(glm, attn_mode):
    ids = _ids(PROMPT, seed=20)
    dense = _make(glm, attn_mode).prefill(ids)
    sparse = _make(glm, attn_mode, True, FULL).prefill(ids)
    torch.cuda.synchronize()
    rel = _rel(sparse, dense)
    print(f"\nfull-coverage minference vs dense ({attn_mode}, {'glm' if glm else 'neox'}): {rel:.3e}")
    assert rel < LOGIT_BOUND


def test_minference_runs_the_sparse_path(monkeypatch):
    from shadowkv_amd import tensor_op
    calls = []
    real = tensor_op.minference_prefill_kernel

    def spy(*a, **kw):
        calls.append(a[3])
        return real(*a, **kw)

    monkeypatch.setattr(tensor_op, "minference_prefill_kernel", spy)
    m = _make(minference=True, pattern=SPARSE)
    m.prefill(_ids(PROMPT))
    assert calls == m.minference_parttern
    calls.clear()
    _make().prefill(_ids(PROMPT))
    assert calls == []


@pytest.mark.parametrize("glm", [False, True])
def test_sparse_generate_eager_and_graph(glm):
    ids = _ids(PROMPT, seed=12)
    m1, m2 = _make(glm, minference=True, pattern=SPARSE), _make(glm, minference=True, pattern=SPARSE)
    g1 = m1.generate(ids, 6, temperature=0.0)
    g2 = m2.generate(ids, 6, temperature=0.0, graph=True)
    torch.cuda.synchronize()
    assert g1.shape == (1, 7) and bool(((g1 >= 0) & (g1 < 2000)).all())
    assert torch.equal(g1, g2), (g1, g2)
    assert m1.kv_cache.get_kv_len() == PROMPT + 6
    d = _make(glm, minference=True, pattern=None).generate(ids, 3, temperature=0.0)     # the default pattern
    torch.cuda.synchronize()
    assert d.shape == (1, 4)


@pytest.mark.parametrize("glm", [False, True])
def test_full_mode_continuation_keeps_the_dense_kernel(glm, monkeypatch):
    from shadowkv_amd import tensor_op
    ids = _ids(PROMPT, seed=9)
    ref = _make(glm, "full")
    ref.prefill(ids[:, :3000])
    l_ref = ref.prefill_cont(ids[:, 3000:])
    m = _make(glm, "full", True, FULL)
    m.prefill(ids[:, :3000])
    calls = []
    real = tensor_op.minference_prefill_kernel
    monkeypatch.setattr(tensor_op, "minference_prefill_kernel", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    l_m = m.prefill_cont(ids[:, 3000:])
    torch.cuda.synchronize()
    assert calls == []
    rel = _rel(l_m, l_ref)
    print(f"\nprefill_cont after a minference prefill ({'glm' if glm else 'neox'}): {rel:.3e}")
    assert rel < LOGIT_BOUND


def test_block_sparse_is_refused_before_any_layer_runs():
    with pytest.raises(ValueError, match="block_sparse"):
        _make(minference=True, pattern=[{}, {3: ("block_sparse", 100, 100, 1)}])
    m = _make(minference=True, pattern=SPARSE)
    m.prefill(_ids(PROMPT, seed=1))
    before = m.kv_cache.k_cache_buffer.clone()
    with pytest.raises(ValueError):
        m.generate(_ids(4096), 4)
    assert torch.equal(m.kv_cache.k_cache_buffer, before)
