"""GPU: the ShadowKV decode step of DecoderLM - forward_fused in its three layouts, three weight formats, two batch paths and
captured - against the f64 restatement of the model in tests/decode_model_ref.py.

Every other model-level decode test compares two paths of this project that share tensor_op and ShadowKVCache_CPU; this one
compares each path with plain f64 torch.  Models: build_synthetic_context(m, 4608), budget 256, rank 160, chunk 8 (there the exact K
is bf16(U . SV), so no kind map is needed), with DISTINCT random norm weights (1 + 0.25 N(0, 1)) copied into every layer's two norm
weights and the final norm weight before the context is built: with the all-ones weights of DecoderLM no test can see a norm weight
used in the wrong place.  Four steps; the kernel's greedy token is fed to both sides, so steps 2 to 4 have hits, misses and
generated rows.  The restatement is handed the set the cache selected (teacher forcing: the top-k is discontinuous at near-ties).

Asserted per step (power of each bound against 19 seeded wiring defects: tests/test_decode_model_ref_cpu.py):
  logits       max |kernel - f64| / max |f64| < 0.02, the LOGIT_BOUND of tests/test_gpu_prefill_model.py for a kernel path against a
               restatement; printed next to the same distance of the round=True restatement (the reference's own rounding noise);
  K / V rows   the new rows of EVERY layer (cache row sparse_end + gen_offset) within rtol 0.02 and atol 0.02 x max |row| of the
               restatement's: layer l's row depends on everything the layers below it produced;
  selection    the cache's set against the exact top-S of the restatement's f64 scores under the reference's rule, per sequence
               and KV head: overlap >= 0.6 at layer 0 (the project's number for this quantity); at deeper layers >= r / 2, r the
               overlap of the f64 and the round=True restatements' top-S (two references; the kernels' roundings are another sample
               of that noise), and r / 2 must exceed 4 S / N - four times what a set from a wrong q or table would reach - else the
               case fails as undecidable.
The printed lines are the record in profiles/decode_model_ref.txt."""
import pytest
import torch

import decode_model_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTX, STEPS = 4608, 4
LOGIT_BOUND, ROW_TOL, OVERLAP0 = 0.02, 0.02, 0.6


def _make(cfg, glm=False, layout="inplace", overlap=True, batch=1, **kw):
    from shadowkv_amd import llama
    if cfg == "tiny":
        size = dict(hidden_size=1024, intermediate_size=2048, num_attention_heads=8, num_key_value_heads=2, vocab_size=2000)
    else:           # hidden 4096: the one-launch norm paths, the split q / kv projection, the lm_head with range keys
        size = dict(hidden_size=4096, intermediate_size=1024, num_attention_heads=32, num_key_value_heads=8, vocab_size=4096)
    mc = llama.ModelConfig(name=cfg, num_hidden_layers=2, qkv_bias=glm, rope_style="glm" if glm else "neox", **size)
    m = llama.DecoderLM(cfg=mc, batch_size=batch, max_length=CTX, device=DEV, sparse_budget=256, rank=160, chunk_size=8, seed=5,
                        chunk_layout=layout, overlap_attention=overlap, **kw)
    ptrs = [w.data_ptr() for w in (m.norm_weight, m.layers[0].input_layernorm_weight, m.layers[1].post_attention_layernorm_weight)]
    ref.randomize_norm_weights(m, 31)
    assert ptrs == [w.data_ptr() for w in (m.norm_weight, m.layers[0].input_layernorm_weight, m.layers[1].post_attention_layernorm_weight)]
    llama.build_synthetic_context(m, CTX, seed=77)
    return m, llama


def _fused_step(m):
    def run(tok):
        c = m.kv_cache
        row = c.sparse_end + c.gen_offset
        lg = m.forward_fused(tok, m.get_ctx(tok), torch.tensor([row], device=DEV), kv_len=row + 1)
        c.note_kv_appended(1)
        return lg[:, -1]
    return run


def _compare(case, m, st, st_r, tok, logits, row, step):
    """One kernel step (already run: its logits, the cache row it wrote) against the two restatements, which are advanced here."""
    c = m.kv_cache
    S, N, L = c.select_sets, c.k_landmark.shape[-2], m.num_layers
    sets = [c.position_ids[l][:, :, :S].clone() for l in range(L)]
    out, out_r = ref.step(st, tok, sets), ref.step(st_r, tok, sets, round=True)
    d, d_r = ref.logit_distance(logits, out.logits), ref.logit_distance(out_r.logits, out.logits)
    line = f"{case} step {step}: logits kernel {float(d.max()):.3e} round=True {float(d_r.max()):.3e} |"
    fails = []
    if not float(d.max()) < LOGIT_BOUND:
        fails.append(f"logits {float(d.max()):.3e}")
    for l in range(L):
        ek = ref.row_excess(c.k_cache_buffer[l][:, :, row], out.k[l], ROW_TOL)
        ev = ref.row_excess(c.v_cache_buffer[l][:, :, row], out.v[l], ROW_TOL)
        ov = ref.set_overlap(sets[l], out.top[l])
        r = ref.set_overlap(out_r.top[l], out.top[l])
        line += f" L{l}: K {ek:.3f} V {ev:.3f} of the row bound, overlap min {float(ov.min()):.3f} mean {float(ov.mean()):.3f} r min {float(r.min()):.3f} |"
        if not (ek < 1 and ev < 1):
            fails.append(f"layer {l} new rows: K {ek:.3f} V {ev:.3f} of the bound")
        if l == 0:
            if not bool((ov >= OVERLAP0).all()):
                fails.append(f"layer 0 overlap {float(ov.min()):.3f}")
        else:
            if not bool((r / 2 > 4 * S / N).all()):
                fails.append(f"layer {l} undecidable: r / 2 = {float(r.min()) / 2:.3f} <= 4 S / N = {4 * S / N:.3f}")
            if not bool((ov >= r / 2).all()):
                fails.append(f"layer {l} overlap {ov.tolist()} below r / 2 = {(r / 2).tolist()}")
    print(line)
    assert not fails, f"{case} step {step}: " + "; ".join(fails)


def _run(case, m, tok, step_fn=None):
    step_fn = step_fn or _fused_step(m)
    st = ref.snapshot(m)
    st_r = st.fork()
    c = m.kv_cache
    for i in range(STEPS):
        row = c.sparse_end + c.gen_offset
        logits = step_fn(tok).float()
        torch.cuda.synchronize()
        _compare(case, m, st, st_r, tok, logits, row, i)
        tok = logits.argmax(dim=-1, keepdim=True)
    assert c.gen_offset == STEPS and st.gen.kv_offset == c.kv_offset == CTX + STEPS


@pytest.mark.parametrize("path", ["reference", "inplace", "overlap"])
@pytest.mark.parametrize("glm", [False, True])
def test_tiny_step_follows_the_restatement(glm, path):
    m, _ = _make("tiny", glm=glm, layout="reference" if path == "reference" else "inplace", overlap=path == "overlap")
    _run(f"tiny {'glm' if glm else 'neox'} {path}", m, torch.tensor([[17]], device=DEV))


@pytest.mark.parametrize("weights,glm", [("bf16", False), ("fp8_e4m3", False), ("mxfp4", False), ("bf16", True)])
def test_h4096_step_follows_the_restatement_and_takes_the_intended_launches(weights, glm):
    from shadowkv_amd import tensor_op
    m, _ = _make("h4096", glm=glm, weight_dtype=weights)
    before = {n: getattr(tensor_op, n) for n in ("fp8_native_calls", "fp8_fallback_calls", "mxfp4_native_calls", "mxfp4_fallback_calls")}
    _run(f"h4096 {weights}{' glm' if glm else ''}", m, torch.tensor([[17]], device=DEV))
    delta = {n: getattr(tensor_op, n) - v for n, v in before.items()}
    dense = STEPS * (4 * m.num_layers + 1)                      # four projections per layer and the lm_head, per step
    if weights == "bf16":                                       # the q rows in front of the scan, the k / v rows in the selection launch
        assert m.kv_proj_split_launches == STEPS * m.num_layers and m.kv_proj_fused_launches == 0
        assert not any(delta.values()), delta
    else:
        fmt = "fp8" if weights == "fp8_e4m3" else "mxfp4"
        want = {n: 0 for n in before}
        want[fmt + "_native_calls"] = dense
        assert delta == want, delta
        assert m.kv_proj_split_launches == 0 and m.kv_proj_fused_launches == STEPS * m.num_layers


@pytest.mark.parametrize("cfg,kw", [("tiny", {}), ("h4096", {"weight_dtype": "fp8_e4m3", "fp8_rows": "native"}),
                                    ("h4096", {"weight_dtype": "mxfp4", "mxfp4_rows": "native"})])
def test_two_sequences_follow_the_restatement(cfg, kw):
    """two sequences with different tokens and contexts (build_synthetic_context draws every sequence's factors and V afresh)"""
    from shadowkv_amd import tensor_op
    m, _ = _make(cfg, layout="reference", overlap=False, batch=2, **kw)
    c = m.kv_cache
    assert not torch.equal(c.U[0][0], c.U[0][1]) and not torch.equal(c.v_cache_cpu[0][0], c.v_cache_cpu[0][1])
    before = {n: getattr(tensor_op, n) for n in ("fp8_native_calls", "fp8_fallback_calls", "mxfp4_native_calls", "mxfp4_fallback_calls")}
    _run(f"bs2 {cfg} {kw.get('weight_dtype', 'bf16')}", m, torch.tensor([[17], [40]], device=DEV))
    delta = {n: getattr(tensor_op, n) - v for n, v in before.items()}
    want = {n: 0 for n in before}
    if kw:                                                      # the rows kernels, not the dequantising fallback
        want[("fp8" if kw["weight_dtype"] == "fp8_e4m3" else "mxfp4") + "_native_calls"] = STEPS * (4 * m.num_layers + 1)
    assert delta == want, delta


def test_captured_step_follows_the_restatement():
    """GraphDecoder on the h4096 bf16 model: two eager warm-up steps on the capture stream, then two replays; the logits are read
    with the tap of tests/test_gpu_fp8_model.py (the captured graph's static output included)."""
    m, llama = _make("h4096")
    box, orig = {}, m.forward_fused

    def ff(*a, **k):
        box["logits"] = orig(*a, **k)
        return box["logits"]

    m.forward_fused = ff
    dec = llama.GraphDecoder(m, temperature=0.0)
    st = ref.snapshot(m)
    st_r = st.fork()
    c = m.kv_cache
    dec.token.copy_(torch.tensor([[17]], device=DEV))
    body = dec._body

    def checked_body():             # (the warm-up steps are steps of the model like any other: compared too)
        if dec._capturing:
            return body()
        tok, row, i = dec.token.clone(), c.sparse_end + c.gen_offset, c.gen_offset
        body()
        torch.cuda.synchronize()
        _compare("captured h4096 bf16" + (" (replay)" if dec.graph is not None else " (warm-up)"), m, st, st_r, tok,
                 box["logits"][:, -1].float(), row, i)

    dec._body = checked_body
    assert dec.capture(warmup=2) == 2 and dec.graph is not None
    for i in range(2, STEPS):
        tok, row = dec.token.clone(), c.sparse_end + c.gen_offset
        dec.step()
        torch.cuda.synchronize()
        _compare("captured h4096 bf16 (replay)", m, st, st_r, tok, box["logits"][:, -1].float(), row, i)
    assert c.gen_offset == STEPS and m.kv_proj_split_launches == 3 * m.num_layers        # two warm-up passes and the captured one
