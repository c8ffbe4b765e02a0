"""GPU: the model-level prefill (DecoderLM.prefill / prefill_cont / batch_prefill / generate) on the tiny two-layer config of
tests/test_gpu_graph.py, NeoX and GLM (qkv bias, GLM RoPE), with real prompts of synthetic token ids.

The PyTorch restatement below recomputes the same weights with torch ops only (RMSNorm, F.linear, RoPE in f32, attention in
f32 through F.scaled_dot_product_attention); the measured max |logit difference| / max |logit| are printed (run with -s)."""
import math

import pytest
import torch
import torch.nn.functional as F

import decode_model_ref as dmr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROMPT = 4700          # > 4096 (the ShadowKV prefill branch), not a multiple of any tile or chunk
LOGIT_BOUND = 0.02     # max |logit difference| relative to max |logit| (measured values are printed)


def _make(glm=False, attn_mode="shadowkv_cpu", batch=1, seed=5, max_length=5120):
    from shadowkv_amd import llama
    cfg = llama.ModelConfig(name="tiny", hidden_size=1024, intermediate_size=2048, num_hidden_layers=2,
                            num_attention_heads=8, num_key_value_heads=2, vocab_size=2000,
                            qkv_bias=glm, rope_style="glm" if glm else "neox")
    return llama.DecoderLM(cfg=cfg, batch_size=batch, max_length=max_length, device=DEV, sparse_budget=256, rank=160,
                           chunk_size=8, seed=seed, attn_mode=attn_mode, max_new_tokens=64)


def _ids(bs, n, seed=3):
    return torch.randint(0, 2000, (bs, n), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _rope(m, x, pos):
    """x [bs, H, S, D] bf16 -> rotated, computed in f32, rounded once."""
    cs = m.cos_sin_cache[pos].float()
    xf = x.float()
    if m.cfg.rope_style == "neox":
        c, s = cs[:, :64], cs[:, 64:]
        x1, x2 = xf[..., :64], xf[..., 64:]
        return torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1).to(x.dtype)
    c, s = cs[:, :32], cs[:, 32:]
    xe, xo = xf[..., 0:64:2], xf[..., 1:64:2]
    rot = torch.stack((xe * c - xo * s, xo * c + xe * s), dim=-1).flatten(-2)
    return torch.cat((rot, xf[..., 64:]), dim=-1).to(x.dtype)


@torch.inference_mode()
def restate(m, ids, positions):
    """Logits [bs, len(positions), V] f32 of a full causal forward over ids, torch ops only, f32 attention."""
    bs, S = ids.shape
    Hq, Hkv, D, hid = m.num_heads, m.num_key_value_heads, m.head_dim, m.hidden_size
    G = Hq // Hkv
    pos = torch.arange(S, device=DEV)
    x = F.embedding(ids, m.embed_tokens)
    for lay in m.layers:
        h = F.rms_norm(x, (hid,), lay.input_layernorm_weight, lay.input_layernorm_variance_epsilon)
        qkv = F.linear(h, lay.wqkv, lay.bqkv)
        q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        q = _rope(m, q.reshape(bs, S, Hq, D).transpose(1, 2), pos)
        k = _rope(m, k.reshape(bs, S, Hkv, D).transpose(1, 2), pos)
        v = v.reshape(bs, S, Hkv, D).transpose(1, 2)
        a = F.scaled_dot_product_attention(q.float(), k.float().repeat_interleave(G, 1), v.float().repeat_interleave(G, 1),
                                           is_causal=True)
        a = a.to(x.dtype).transpose(1, 2).reshape(bs, S, hid)
        x = x + F.linear(a, lay.wo)
        h = F.rms_norm(x, (hid,), lay.post_attention_layernorm_weight, lay.post_attention_layernorm_variance_epsilon)
        g, u = F.linear(h, lay.gate_up_proj).chunk(2, dim=-1)
        x = x + F.linear(F.silu(g) * u, lay.down_proj)
    h = F.rms_norm(x[:, positions], (hid,), m.norm_weight, m.norm_variance_epsilon)
    return F.linear(h, m.lm_head).float()


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize("glm", [False, True])
def test_prefill_logits_match_restatement(glm):
    m = _make(glm=glm)
    ids = _ids(1, PROMPT)
    logits = m.prefill(ids)
    torch.cuda.synchronize()
    assert logits.shape == (1, 1, 2000) and logits.dtype == torch.float32
    assert m.kv_cache.get_kv_len() == PROMPT
    ref = restate(m, ids, [PROMPT - 1])
    rel = _rel(logits, ref)
    print(f"\nprefill logits ({'glm' if glm else 'neox'}): max |d| / max |logit| = {rel:.3e}, "
          f"argmax {int(logits.argmax())} vs {int(ref.argmax())}")
    assert rel < LOGIT_BOUND


@pytest.mark.parametrize("glm", [False, True])
def test_full_and_shadowkv_prefill_agree_bitwise(glm):
    ids = _ids(1, PROMPT, seed=4)
    a = _make(glm=glm).prefill(ids)
    b = _make(glm=glm, attn_mode="full").prefill(ids)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


@pytest.mark.parametrize("glm", [False, True])
def test_layer0_state_equals_direct_builders(glm):
    """Layer 0's inputs do not depend on attention: the state prefill() leaves must be what get_svd + prefill_kv_cache leave
    when called directly on the K / V / q computed from the embedding."""
    ids = _ids(1, PROMPT, seed=6)
    m1 = _make(glm=glm)
    m1.prefill(ids)
    m2 = _make(glm=glm)
    c2 = m2.kv_cache
    with torch.inference_mode():
        c2.clear()
        hs = F.embedding(ids, m2.embed_tokens)
        q, k, v = m2.pre_attention_compute(hs, m2.layers[0])
        c2.get_svd(k, layer_idx=0)
        q, k = m2.apply_rotary_pos_emb(q, k, m2.get_ctx(ids))
        c2.prefill_kv_cache(v, 0, k, q[:, :, -1:])
    torch.cuda.synchronize()
    c1 = m1.kv_cache

    def same(x, y):
        x, y = x.cpu(), y.cpu()
        if x.dtype == torch.bfloat16:
            x, y = x.view(torch.int16), y.view(torch.int16)
        return torch.equal(x, y)

    assert same(c1.U[0], c2.U[0]) and same(c1.SV[0], c2.SV[0])
    assert same(c1.k_landmark[0], c2.k_landmark[0]) and same(c1.k_landmark_idx[0], c2.k_landmark_idx[0])
    assert same(c1.position_ids[0], c2.position_ids[0])
    assert same(c1.k_cache_buffer[0], c2.k_cache_buffer[0]) and same(c1.v_cache_buffer[0], c2.v_cache_buffer[0])
    assert same(c1.v_cache_cpu[0], c2.v_cache_cpu[0])
    assert c1.sparse_start == c2.sparse_start and c1.sparse_end == c2.sparse_end


def test_batch_prefill_sub_batches_are_bit_identical():
    ids = _ids(2, PROMPT, seed=8)
    ma, mb = _make(batch=2), _make(batch=2)
    la = ma.batch_prefill(ids, sub_batch=1)
    lb = mb.batch_prefill(ids, sub_batch=2)
    singles = [_make().prefill(ids[i:i + 1]) for i in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    assert torch.equal(la, torch.cat(singles))
    ca, cb = ma.kv_cache, mb.kv_cache
    assert ca.get_kv_len() == cb.get_kv_len() == PROMPT
    assert torch.equal(ca.position_ids, cb.position_ids)
    assert torch.equal(ca.k_cache_buffer.view(torch.int16), cb.k_cache_buffer.view(torch.int16))
    assert torch.equal(ca.v_cache_buffer.view(torch.int16), cb.v_cache_buffer.view(torch.int16))


@pytest.mark.parametrize("glm", [False, True])
def test_full_mode_continuation(glm):
    ids = _ids(1, PROMPT, seed=9)
    one = _make(glm=glm, attn_mode="full")
    l1 = one.prefill(ids)
    two = _make(glm=glm, attn_mode="full")
    two.prefill(ids[:, :3000])
    l2 = two.prefill_cont(ids[:, 3000:])
    torch.cuda.synchronize()
    assert two.kv_cache.get_kv_len() == PROMPT
    rel = _rel(l2, l1)
    print(f"\nprefill_cont ({'glm' if glm else 'neox'}): two pieces vs one, max |d| / max |logit| = {rel:.3e}")
    assert rel < LOGIT_BOUND
    k1, k2 = one.kv_cache.k_cache[:, :, :, :PROMPT].float(), two.kv_cache.k_cache[:, :, :, :PROMPT].float()
    assert _rel(k2, k1) < LOGIT_BOUND
    with pytest.raises(NotImplementedError):
        _make(glm=glm).prefill_cont(ids[:, :10])


def _tap_decode_steps(m, ids):
    """Wraps m.forward_fused (the pattern of tests/test_gpu_fp8_model.py::_tap): the f64 state of the prefilled prompt is taken
    at the first decode step - after generate()'s prefill and H2D, before anything steps - and every step leaves (its input
    token, its logits, the chunk sets position_ids names afterwards).  -> (box with "state", the list of steps)"""
    box, steps, orig = {}, [], m.forward_fused

    def ff(token, *a, **k):
        if "state" not in box:
            box["state"] = dmr.snapshot_prefilled(m, ids)
        tok = token.clone()
        out = orig(token, *a, **k)
        c = m.kv_cache
        steps.append((tok, out[:, -1].float(), [c.position_ids[l][:, :, :c.select_sets].clone() for l in range(m.num_layers)]))
        return out

    m.forward_fused = ff
    return box, steps


@pytest.mark.parametrize("attn_mode", ["shadowkv_cpu", "full"])
@pytest.mark.parametrize("glm", [False, True])
def test_greedy_generate_follows_restatement(glm, attn_mode):
    """ShadowKV branch, decode steps: the tokens leave the FULL-attention restatement (256 of 4,700 rows are attended), so each
    step's logits are checked against the restatement of the sparse step itself (tests/decode_model_ref.py: the prompt's K / V
    from an f64 dense forward, exact K for the chunks resident since the prefill and RoPE(U . SV) for the misses, the set the
    cache selected, the tokens generate() produced) under LOGIT_BOUND.  Measured on one MI355X, max |d| / max |logit| over the 8
    steps: see profiles/decode_model_ref.txt.  The norm weights are distinct random vectors (1 + 0.25 N(0, 1))."""
    m = _make(glm=glm, attn_mode=attn_mode)
    dmr.randomize_norm_weights(m, 41)
    ids = _ids(1, PROMPT, seed=10)
    if attn_mode != "full":
        box, steps = _tap_decode_steps(m, ids)
    gen = m.generate(ids, 8, temperature=0.0)
    torch.cuda.synchronize()
    assert gen.shape == (1, 9) and gen.dtype == torch.long
    seq = torch.cat([ids, gen[:, :-1]], dim=1)
    ref = restate(m, seq, list(range(PROMPT - 1, PROMPT + 8)))[0]          # [9, V]: the logits each token was chosen from
    chosen = ref.gather(-1, gen[0].unsqueeze(-1)).squeeze(-1)
    gap = (ref.max(dim=-1).values - chosen) / ref.abs().max(dim=-1).values
    print(f"\ngreedy generate ({attn_mode}, {'glm' if glm else 'neox'}): tokens {gen[0].tolist()}, "
          f"(ref max - ref[chosen]) / max |ref| per step = {[round(float(x), 4) for x in gap]}")
    if attn_mode == "full":
        assert float(gap.max()) < LOGIT_BOUND          # exact attention at every step
    else:
        # the first token comes from the dense prefill; the decode steps attend the ShadowKV selection (256 of 4,700 rows
        # here), an approximation of the restatement's full attention that this random-weight model does not follow
        assert float(gap[0]) < LOGIT_BOUND
        assert bool(((gen >= 0) & (gen < 2000)).all())
        assert len(steps) == 8 and [int(t) for t, _, _ in steps] == gen[0, :8].tolist()
        st, dist = box["state"], []
        for tok, logits, sets in steps:
            dist.append(float(dmr.logit_distance(logits, dmr.step(st, tok, sets).logits).max()))
        print(f"prefilled {'glm' if glm else 'neox'}: decode logits against the sparse restatement, max |d| / max |logit| per step = "
              f"{[round(d, 5) for d in dist]}")
        assert max(dist) < LOGIT_BOUND, dist
    assert m.kv_cache.get_kv_len() == PROMPT + 8


@pytest.mark.parametrize("glm", [False, True])
def test_generate_graph_equals_eager(glm):
    ids = _ids(1, PROMPT, seed=12)
    m1, m2 = _make(glm=glm), _make(glm=glm)
    g1 = m1.generate(ids, 6, temperature=0.0)
    g2 = m2.generate(ids, 6, temperature=0.0, graph=True)
    torch.cuda.synchronize()
    assert torch.equal(g1, g2), (g1, g2)
    c1, c2 = m1.kv_cache, m2.kv_cache
    assert c1.kv_offset == c2.kv_offset == PROMPT + 6 and c1.gen_offset == c2.gen_offset
    assert torch.equal(c1.position_ids, c2.position_ids)
    assert torch.equal(c1.k_cache_buffer.view(torch.int16), c2.k_cache_buffer.view(torch.int16))
    assert torch.equal(c1.v_cache_buffer.view(torch.int16), c2.v_cache_buffer.view(torch.int16))


def test_bad_requests_raise_before_any_layer_runs():
    m = _make()
    ids = _ids(1, PROMPT, seed=14)
    m.prefill(ids)
    state = (m.kv_cache.get_kv_len(), m.kv_cache.k_cache_buffer.clone())

    def untouched():
        return m.kv_cache.get_kv_len() == state[0] and torch.equal(m.kv_cache.k_cache_buffer, state[1])

    with pytest.raises(ValueError):
        m.generate(_ids(1, 4096), 4)                                    # too short for the ShadowKV prefill
    assert untouched()
    with pytest.raises(ValueError):
        m.generate(ids, m.kv_cache.generated_row_slack_after_prefill(PROMPT) + 1)   # more tokens than generated rows
    assert untouched()
    with pytest.raises(ValueError):
        m.prefill(_ids(1, 5121))                                        # over max_length
    assert untouched()
    with pytest.raises(ValueError):
        m.generate(ids, 500)                                            # past the RoPE table / the row slack
    assert untouched()
    f = _make(attn_mode="full")
    with pytest.raises(ValueError):
        f.generate(_ids(1, 5121), 1)
    with pytest.raises(ValueError):
        f.generate(ids, 5120 + 64 - PROMPT + 1)                         # past the RoPE table
