"""f64 restatement of ONE ShadowKV decode step of DecoderLM, plain torch; not collected (no test_ prefix).
Nothing of shadowkv_amd is imported: snapshot() only reads attributes of the model it is handed.

What is restated is the WIRING of a step - which weight, which norm weight, which position, which rows, which head - on top of
kernels that each have an exact or f64 reference of their own.  Three things are teacher-forced, because they are pinned
elsewhere or are discontinuous:
  the selected set    step() is handed the chunk ids the cache selected in this step (position_ids[l][:, :, :select_sets] after the
                      kernel step): the selection is a top-k over near-ties.  It is judged separately: step() also returns the f64
                      scores under the reference's rule (kv_cache.py::_score_landmarks_torch: q . landmark / sqrt(128), softmax over
                      the landmarks, max over the group, k_landmark_idx) and the exact top-S they give;
  the tokens          the caller feeds the kernel's greedy token to both sides;
  U / SV, landmarks   the factors and the landmark table are read from the cache (their construction has its own tests).

State: make_state() takes plain tensors (the CPU tests build states by hand), snapshot(model) reads a DecoderLM before it steps
and copies whatever a step overwrites, snapshot_prefilled(model, ids) additionally replaces the prompt's K / V by an f64 dense
causal forward of its own and keeps the map chunk -> exact | low-rank (a chunk of the sparse region keeps the prefill's exact K
while it stays resident; a miss is rebuilt from U . SV).  A state is mutable only in its `gen` part (the restatement's own k / v
rows, the two offsets, the kind map): fork() shares the rest.

round=True rounds to bf16 where the kernels' contracts round (norm outputs and h, projection outputs, RoPE outputs, attention
output, SiLU * mul output, logits).  It is the reference's own rounding noise: a yardstick, never an expected value.

defect= seeds one wiring error (DEFECTS) for tests/test_decode_model_ref_cpu.py."""
import math
from types import SimpleNamespace as NS

import torch

import mxfp4_ref as mr

F64 = torch.float64
SCORE_ALPHA = 1.0 / math.sqrt(128)          # the reference scores landmarks at 1 / sqrt(128) whatever the head size

DEFECTS = (
    "attn_residual_dropped",            # x + wo(attn) -> wo(attn)
    "mlp_residual_dropped",             # x + down(act) -> down(act)
    "post_norm_input_weight",           # post-attention norm with the input norm's weight
    "final_norm_layer_weight",          # final norm with layer 0's input norm weight
    "input_norm_weight_ignored",        # a norm weight ignored (ones), one defect per norm
    "post_norm_weight_ignored",
    "final_norm_weight_ignored",
    "rope_pos_plus_one",                # q and k rotated at kv_offset + 1
    "k_pushed_unrotated",               # the new k row stored (and attended) un-rotated
    "self_not_attended",                # kv_len one short: the new token's own row is not attended
    "generated_not_attended",           # the earlier generated rows are not attended
    "v_neighbour_chunk",                # V rows of a selected chunk taken from chunk + 1
    "k_slot_order_rope",                # K of a selected chunk rotated at its slot's row index instead of its token position
    "head_map_mod",                     # query head h reads KV head h % Hkv instead of h // G
    "gate_up_swapped",                  # silu(up) * gate
    "bias_dropped",                     # the QKV bias (GLM) not added
    "usv_prev_layer",                   # layer l rebuilds K from layer l - 1's U / SV
    "select_pre_rope_q",                # selection scored with the un-rotated q
    "select_other_layer_landmarks",     # selection scored against the next layer's landmark table
)


def rb(x, on=True):
    """x rounded to bf16 (as f64) where `on`."""
    return x.to(torch.bfloat16).to(F64) if on else x


def mx_decode(w4, w_scale, rows=1024):
    """The decode rule of tests/mxfp4_ref.py (its E2M1 table and BLOCK; low nibble first, bit 3 the sign, 2^(scale byte - 127) per
    32 elements) in torch, on the tensors' device: f64 [N, K].  Asserted equal to mxfp4_ref.decode by the CPU tests."""
    tab = torch.tensor(mr.E2M1, dtype=F64, device=w4.device)
    out = []
    for r in range(0, w4.shape[0], rows):
        b = w4[r:r + rows].to(torch.int64)
        nib = torch.stack((b & 0xF, b >> 4), dim=-1).reshape(b.shape[0], -1)
        val = tab[nib & 7]
        val = torch.where((nib & 8) != 0, -val, val)
        e = w_scale[r:r + rows].to(torch.int64) - 127
        out.append(val * torch.ldexp(torch.ones_like(e, dtype=F64), e).repeat_interleave(mr.BLOCK, dim=1))
    return torch.cat(out)


def weight64(w, scale):
    """A decode matrix as the kernels are defined to read it, f64: bf16 as it is; float8_e4m3fn times its f32 row scale; MXFP4
    nibbles (uint8) times their e8m0 block scales."""
    if scale is None:
        if w.dtype != torch.bfloat16:
            raise ValueError(f"a matrix without scales must be bf16, got {w.dtype}")
        return w.to(F64)
    if w.dtype == torch.float8_e4m3fn:
        return w.float().to(F64) * scale.to(F64).unsqueeze(1)
    if w.dtype == torch.uint8 and scale.dtype == torch.uint8:
        return mx_decode(w, scale)
    raise ValueError(f"unknown weight format: {w.dtype} with {scale.dtype} scales")


def rope(x, cs, style):
    """x f64 [..., D] rotated by the table rows cs f64 [..., W] (broadcast against x's leading dims).  "neox": W = D, cos | sin
    of D / 2 angles, the halves of x are the pairs.  "glm": W = 64, cos | sin of 32 angles, the pairs are (x[2i], x[2i + 1])
    of the first 64 dims, the rest passes through."""
    half = cs.shape[-1] // 2
    c, s = cs[..., :half], cs[..., half:]
    if style == "neox":
        assert x.shape[-1] == 2 * half
        x1, x2 = x[..., :half], x[..., half:]
        return torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1)
    assert style == "glm"
    xe, xo = x[..., 0:2 * half:2], x[..., 1:2 * half:2]
    rot = torch.stack((xe * c - xo * s, xo * c + xe * s), dim=-1).flatten(-2)
    return torch.cat((rot, x[..., 2 * half:]), dim=-1)


def rmsnorm(x, w, eps):
    return x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps) * w


def silu(x):
    return x / (1.0 + torch.exp(-x))


# ------------------------------------------------------------------------------------------------------------- state
class State:
    """Plain attributes.  Immutable after construction: embed, lm_head, norm_w, norm_eps, layers[l] (wqkv, bqkv, wo, gate_up, down,
    in_w, in_eps, post_w, post_eps), cos_sin, cache[l] (U [bs, n, r], SV [bs, Hkv, D, r], lm [bs, Hkv, N, D], lm_idx [bs, Hkv, N],
    v_table [bs, Hkv, chunks, C * D], k_fixed / v_fixed [bs, Hkv, rows, D]: the local and outlier rows, exact_k [bs, Hkv, n, D] or
    None) and the scalars.  Mutable: gen (k[l] / v[l]: lists of [bs, Hkv, D], kv_offset, gen_offset, kind[l] bool [bs, Hkv, chunks]
    or None)."""

    def fork(self):
        s = State()
        s.__dict__.update(self.__dict__)
        g = self.gen
        s.gen = NS(k=[list(x) for x in g.k], v=[list(x) for x in g.v], kv_offset=g.kv_offset, gen_offset=g.gen_offset,
                   kind=[None if x is None else x.clone() for x in g.kind])
        return s


def make_state(*, embed, lm_head, norm_w, norm_eps, layers, cos_sin, cache, chunk_size, select_sets, sparse_start, sparse_end,
               gen_offset, kv_offset, num_heads, num_kv_heads, rope_style, kind=None):
    s = State()
    s.embed, s.lm_head, s.norm_w, s.norm_eps = embed, lm_head, norm_w, float(norm_eps)
    s.layers, s.cos_sin, s.cache = list(layers), cos_sin, list(cache)
    s.chunk_size, s.select_sets, s.sparse_start, s.sparse_end = int(chunk_size), int(select_sets), int(sparse_start), int(sparse_end)
    s.num_heads, s.num_kv_heads, s.rope_style = int(num_heads), int(num_kv_heads), rope_style
    s.head_dim = embed.shape[1] // s.num_heads
    assert rope_style in ("neox", "glm") and s.num_heads % s.num_kv_heads == 0
    for t in (embed, lm_head, norm_w, cos_sin):
        assert t.dtype == F64
    n = len(s.layers)
    s.gen = NS(k=[[] for _ in range(n)], v=[[] for _ in range(n)], kv_offset=int(kv_offset), gen_offset=int(gen_offset),
               kind=list(kind) if kind is not None else [None] * n)
    return s


def randomize_norm_weights(model, seed):
    """1 + 0.25 N(0, 1), a fresh draw per vector, copied INTO every layer's two norm weights and the final norm weight (the
    pointers stay): DecoderLM starts with all-ones norm weights, under which no test can tell one norm weight from another."""
    g = torch.Generator().manual_seed(seed)
    for w in [t for lay in model.layers for t in (lay.input_layernorm_weight, lay.post_attention_layernorm_weight)] + [model.norm_weight]:
        w.copy_((1 + 0.25 * torch.randn(w.shape, generator=g)).to(w.device))


def _model_layers(model):
    out = []
    for lay in model.layers:
        out.append(NS(wqkv=weight64(lay.wqkv, lay.wqkv_scale), bqkv=None if lay.bqkv is None else lay.bqkv.to(F64),
                      wo=weight64(lay.wo, lay.wo_scale), gate_up=weight64(lay.gate_up_proj, lay.gate_up_proj_scale),
                      down=weight64(lay.down_proj, lay.down_proj_scale),
                      in_w=lay.input_layernorm_weight.to(F64), in_eps=float(lay.input_layernorm_variance_epsilon),
                      post_w=lay.post_attention_layernorm_weight.to(F64),
                      post_eps=float(lay.post_attention_layernorm_variance_epsilon)))
    return out


@torch.inference_mode()
def snapshot(model):
    """The state of a DecoderLM on a filled ShadowKV cache, taken BEFORE it steps.  Everything is copied (a cast to f64 copies)."""
    c = model.kv_cache
    if getattr(model, "attn_mode", None) != "shadowkv_cpu":
        raise ValueError("snapshot restates the ShadowKV decode step: attn_mode must be 'shadowkv_cpu'")
    if model.v_dtype != "bf16" or model.landmark_dtype != "bf16":
        raise ValueError(f"snapshot covers v_dtype='bf16' and landmark_dtype='bf16' only (got {model.v_dtype!r}, "
                         f"{model.landmark_dtype!r}): the FP8 tables have tests against the paths pinned here")
    if c.resident_sets != c.select_sets:
        raise ValueError(f"snapshot covers resident_sets == select_sets only (got {c.resident_sets} != {c.select_sets})")
    if c.U is None or c.k_landmark is None:
        raise ValueError("snapshot needs a filled cache (prefill or build_synthetic_context first)")
    dev = model.device
    cache = []
    for l in range(model.num_layers):
        cache.append(NS(U=c.U[l].to(F64), SV=c.SV[l].to(F64), lm=c.landmarks_bf16(l).to(F64), lm_idx=c.k_landmark_idx[l].clone(),
                        v_table=c.v_cache_cpu[l].to(dev).to(F64),
                        k_fixed=c.k_cache_buffer[l][:, :, :c.sparse_start].to(F64),
                        v_fixed=c.v_cache_buffer[l][:, :, :c.sparse_start].to(F64), exact_k=None))
    return make_state(embed=model.embed_tokens.to(F64), lm_head=weight64(model.lm_head, model.lm_head_scale),
                      norm_w=model.norm_weight.to(F64), norm_eps=model.norm_variance_epsilon, layers=_model_layers(model),
                      cos_sin=model.cos_sin_cache.to(F64), cache=cache, chunk_size=c.chunk_size, select_sets=c.select_sets,
                      sparse_start=c.sparse_start, sparse_end=c.sparse_end, gen_offset=c.gen_offset, kv_offset=c.kv_offset,
                      num_heads=model.num_heads, num_kv_heads=model.num_key_value_heads, rope_style=model.cfg.rope_style)


def dense_prompt_kv(state, ids):
    """f64 dense causal forward of the state's weights over ids [bs, n] at positions 0 .. n - 1, attention one query head at a time:
    ([K_l] rotated, [V_l]) each [bs, Hkv, n, D], and the last position's logits [bs, V]."""
    bs, n = ids.shape
    Hq, Hkv, D = state.num_heads, state.num_kv_heads, state.head_dim
    G = Hq // Hkv
    x = state.embed[ids]
    cs = state.cos_sin[:n]
    causal = torch.ones(n, n, dtype=torch.bool, device=x.device).tril_()
    Ks, Vs = [], []
    for lay in state.layers:
        qkv = rmsnorm(x, lay.in_w, lay.in_eps) @ lay.wqkv.T
        if lay.bqkv is not None:
            qkv = qkv + lay.bqkv
        q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        q = rope(q.view(bs, n, Hq, D).transpose(1, 2), cs, state.rope_style)
        k = rope(k.view(bs, n, Hkv, D).transpose(1, 2), cs, state.rope_style).contiguous()
        v = v.view(bs, n, Hkv, D).transpose(1, 2).contiguous()
        Ks.append(k)
        Vs.append(v)
        a = torch.empty(bs, n, Hq, D, dtype=F64, device=x.device)
        for h in range(Hq):
            s = (q[:, h] @ k[:, h // G].transpose(1, 2)) / math.sqrt(D)
            s.masked_fill_(~causal, float("-inf"))
            a[:, :, h] = torch.softmax(s, dim=-1) @ v[:, h // G]
            del s
        x = x + a.view(bs, n, Hq * D) @ lay.wo.T
        g, u = (rmsnorm(x, lay.post_w, lay.post_eps) @ lay.gate_up.T).chunk(2, dim=-1)
        x = x + (silu(g) * u) @ lay.down.T
    return Ks, Vs, rmsnorm(x[:, -1], state.norm_w, state.norm_eps) @ state.lm_head.T


def prefilled_state(state, ids, prefill_local, chunks, resident_ids):
    """A state whose prompt rows are the exact K / V of dense_prompt_kv(state, ids) placed by the cache's bookkeeping: the last
    `prefill_local` tokens are the local rows, the chunks below `chunks` that k_landmark_idx does not name are the outlier chunks,
    resident_ids[l] int64 [bs, Hkv, S] are the chunks the prefill left in the sparse region with exact K.  U / SV, the landmarks
    and the scalars stay those of `state`."""
    bs, n = ids.shape
    C, D = state.chunk_size, state.head_dim
    Ks, Vs, _ = dense_prompt_kv(state, ids)
    s = state.fork()
    s.cache, kinds = [], []
    for l, (old, K, V) in enumerate(zip(state.cache, Ks, Vs)):
        outl = torch.ones(bs, state.num_kv_heads, chunks, dtype=torch.bool, device=K.device)
        outl.scatter_(-1, old.lm_idx, False)
        n_out = int(outl[0, 0].sum())
        assert bool((outl.sum(-1) == n_out).all())
        oc = outl.nonzero()[:, 2].view(bs, state.num_kv_heads, n_out)                                   # ascending chunk ids
        tok = (oc.unsqueeze(-1) * C + torch.arange(C, device=K.device)).view(bs, state.num_kv_heads, n_out * C, 1).expand(-1, -1, -1, D)
        k_fixed = torch.cat((K[:, :, n - prefill_local:], K.gather(2, tok)), dim=2)
        v_fixed = torch.cat((V[:, :, n - prefill_local:], V.gather(2, tok)), dim=2)
        assert k_fixed.shape[2] == state.sparse_start
        nch = n // C
        s.cache.append(NS(U=old.U, SV=old.SV, lm=old.lm, lm_idx=old.lm_idx, k_fixed=k_fixed, v_fixed=v_fixed, exact_k=K,
                          v_table=V[:, :, :nch * C].reshape(bs, state.num_kv_heads, nch, C * D)))
        kind = torch.zeros(bs, state.num_kv_heads, nch, dtype=torch.bool, device=K.device)
        kind.scatter_(-1, resident_ids[l], True)
        kinds.append(kind)
    s.gen.kind = kinds
    return s


@torch.inference_mode()
def snapshot_prefilled(model, ids):
    """snapshot() of a model after a real prefill of ids [bs, n], with the prompt's K / V restated (prefilled_state)."""
    c = model.kv_cache
    st = snapshot(model)
    if c.gen_offset != 0 or c.kv_offset != ids.shape[1]:
        raise ValueError("snapshot_prefilled is taken right after the prefill of `ids`, before any decode step")
    S = c.select_sets
    return prefilled_state(st, ids, c.prefill_local, c.chunks, [c.position_ids[l][:, :, :S].clone() for l in range(model.num_layers)])


# ------------------------------------------------------------------------------------------------------------- one step
def selection_scores(q, lm, lm_idx, G, S, round=False):
    """The reference's rule in f64: q [bs, Hq, D] (post-RoPE), lm [bs, Hkv, N, D] -> (scores [bs, Hkv, N], the top-S chunk ids
    [bs, Hkv, S]).  round: the softmax weights rounded to bf16 before the maximum over the group, as the reference's are."""
    bs, Hq, D = q.shape
    a = torch.einsum("bhgd,bhnd->bhgn", q.view(bs, Hq // G, G, D), lm) * SCORE_ALPHA
    p = rb(torch.softmax(a, dim=-1), round).max(dim=2).values
    return p, lm_idx.gather(-1, p.topk(S, dim=-1).indices)


@torch.inference_mode()
def step(state, tokens, sets, round=False, defect=None):
    """One decode step of every sequence.  tokens int64 [bs] or [bs, 1]; sets[l] int64 [bs, Hkv, S]: the chunks the cache selected
    in this step.  Appends the step's own k / v rows to state.gen and advances the offsets.  Returns a namespace: logits [bs, V];
    q[l] [bs, Hq, D] (post-RoPE), k[l] / v[l] [bs, Hkv, D] (the new cache rows); scores[l] [bs, Hkv, N], top[l] [bs, Hkv, S]."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")
    R = round
    Hq, Hkv, D, C, S = state.num_heads, state.num_kv_heads, state.head_dim, state.chunk_size, state.select_sets
    G, gen, L = Hq // Hkv, state.gen, len(state.layers)
    tokens = tokens.reshape(-1)
    bs = tokens.shape[0]
    dev = state.embed.device
    pos = gen.kv_offset + (1 if defect == "rope_pos_plus_one" else 0)
    cs_new = state.cos_sin[pos]
    kv_of = torch.arange(Hq, device=dev) % Hkv if defect == "head_map_mod" else torch.arange(Hq, device=dev) // G
    out = NS(q=[], k=[], v=[], scores=[], top=[])
    x = state.embed[tokens]
    for l, (lay, ch) in enumerate(zip(state.layers, state.cache)):
        in_w = torch.ones_like(lay.in_w) if defect == "input_norm_weight_ignored" else lay.in_w
        qkv = rb(rmsnorm(x, in_w, lay.in_eps), R) @ lay.wqkv.T
        if lay.bqkv is not None and defect != "bias_dropped":
            qkv = qkv + lay.bqkv
        q, k, v = rb(qkv, R).split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        q, k, v = q.view(bs, Hq, D), k.view(bs, Hkv, D), v.view(bs, Hkv, D)
        qr, kr = rb(rope(q, cs_new, state.rope_style), R), rb(rope(k, cs_new, state.rope_style), R)
        k_new = k if defect == "k_pushed_unrotated" else kr
        # the selection this q gives under the reference's rule (not what is attended: that is `sets`)
        sel = state.cache[(l + 1) % L] if defect == "select_other_layer_landmarks" else ch
        sc, top = selection_scores(q if defect == "select_pre_rope_q" else qr, sel.lm, sel.lm_idx, G, S, round=R)
        # (ii) the selected chunks: K = RoPE_t(U[t] . SV[h]^T) - or the prefill's exact K while the chunk stayed resident - and V from the table
        ids = sets[l].to(dev)
        assert ids.shape == (bs, Hkv, S), ids.shape
        tok = (ids.unsqueeze(-1) * C + torch.arange(C, device=dev)).view(bs, Hkv, S * C)
        fac = state.cache[l - 1] if defect == "usv_prev_layer" and l > 0 else ch
        b_ix = torch.arange(bs, device=dev).view(bs, 1, 1)
        k_pre = rb(torch.einsum("bhtr,bhdr->bhtd", fac.U[b_ix, tok], fac.SV), R)
        # (the defect: the position a slot-ordered rotation would use, the slot's buffer row)
        at = (state.sparse_start + torch.arange(S * C, device=dev)).expand(bs, Hkv, -1) if defect == "k_slot_order_rope" else tok
        k_sel = rb(rope(k_pre, state.cos_sin[at], state.rope_style), R)
        kind = gen.kind[l]
        if kind is not None:
            exact = kind.gather(-1, ids).repeat_interleave(C, dim=-1).unsqueeze(-1)
            k_sel = torch.where(exact, ch.exact_k.gather(2, tok.unsqueeze(-1).expand(-1, -1, -1, D)), k_sel)
            gen.kind[l] = kind & torch.zeros_like(kind).scatter_(-1, ids, True)       # hits keep their kind, misses are low-rank
        v_ids = (ids + 1).clamp(max=ch.v_table.shape[2] - 1) if defect == "v_neighbour_chunk" else ids
        v_sel = ch.v_table.gather(2, v_ids.unsqueeze(-1).expand(-1, -1, -1, C * D)).view(bs, Hkv, S * C, D)
        ks, vs = [ch.k_fixed, k_sel], [ch.v_fixed, v_sel]                 # (i) local and outlier rows, (ii)
        if defect != "generated_not_attended" and gen.k[l]:               # (iii) the restatement's own earlier rows
            ks.append(torch.stack(gen.k[l], dim=2))
            vs.append(torch.stack(gen.v[l], dim=2))
        if defect != "self_not_attended":                                 # (iv) this token
            ks.append(k_new.unsqueeze(2))
            vs.append(v.unsqueeze(2))
        K, V = torch.cat(ks, dim=2)[:, kv_of], torch.cat(vs, dim=2)[:, kv_of]          # [bs, Hq, rows, D]
        p = torch.softmax(torch.einsum("bhd,bhnd->bhn", qr, K) / math.sqrt(D), dim=-1)
        attn = rb(torch.einsum("bhn,bhnd->bhd", p, V), R).reshape(bs, Hq * D)
        o = rb(attn @ lay.wo.T, R)
        x = o if defect == "attn_residual_dropped" else rb(x + o, R)
        post_w = lay.in_w if defect == "post_norm_input_weight" else lay.post_w
        if defect == "post_norm_weight_ignored":
            post_w = torch.ones_like(post_w)
        g, u = rb(rb(rmsnorm(x, post_w, lay.post_eps), R) @ lay.gate_up.T, R).chunk(2, dim=-1)
        act = rb(silu(u) * g if defect == "gate_up_swapped" else silu(g) * u, R)
        d = rb(act @ lay.down.T, R)
        x = d if defect == "mlp_residual_dropped" else rb(x + d, R)
        gen.k[l].append(k_new)
        gen.v[l].append(v)
        out.q.append(qr)
        out.k.append(k_new)
        out.v.append(v)
        out.scores.append(sc)
        out.top.append(top)
    norm_w = state.norm_w
    if defect == "final_norm_layer_weight":
        norm_w = state.layers[0].in_w
    elif defect == "final_norm_weight_ignored":
        norm_w = torch.ones_like(norm_w)
    out.logits = rb(rb(rmsnorm(x, norm_w, state.norm_eps), R) @ state.lm_head.T, R)
    gen.kv_offset += 1
    gen.gen_offset += 1
    return out


# ------------------------------------------------------------------------------------------------------------- measures
def logit_distance(a, ref):
    """max |a - ref| / max |ref| per sequence: [bs]"""
    return (a.to(F64) - ref).abs().amax(dim=-1) / ref.abs().amax(dim=-1)


def row_excess(a, ref, tol=0.02):
    """The largest |a - ref| / (tol max |ref row| + tol |ref|) over the new K or V rows [bs, Hkv, D]: below 1 iff every element
    lies within rtol = tol and atol = tol x the largest magnitude of its row."""
    a = a.to(F64)
    return float(((a - ref).abs() / (tol * ref.abs().amax(dim=-1, keepdim=True) + tol * ref.abs())).max())


def set_overlap(a, b):
    """The fraction of a's ids found in b, per (sequence, KV head): a, b int64 [bs, Hkv, S] -> f64 [bs, Hkv]"""
    return (a.unsqueeze(-1) == b.to(a.device).unsqueeze(-2)).any(-1).to(F64).mean(-1)
