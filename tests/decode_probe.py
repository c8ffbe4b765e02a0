"""Attended-row read-out for the DECODE attention paths, built on tests/attn_probe.py: one query row per
head (Probe(L, R=1, ...)), so the bf16 output of a decode attention names, for every (sequence, head), which of the L buffer
rows - or, on a ShadowKV cache, which of the L tokens - were attended and how many times.  Plain torch, no library import.

Row-keyed (standalone kernel, slot list): the probe is over the rows of the K / V buffers, a fresh (kdim, vdim) pair per launch.
Token-keyed (cache paths): the probe is over the tokens n < N_tok = L_ctx + gen; the cache keeps its K / V state between the
launches, so the maps do not change with the launch (TokenProbe) and only the query steps through the classes.  What makes a
ShadowKV cache readable:
  identity RoPE table    [cos = 1 | sin = 0] (128 columns NeoX, 64 GLM): the rebuild's RoPE epilogue is exact on one-hot rows;
  token-keyed factors    U[n] = e_(class n), SV[h] = 64 x the head's kdim permutation: U[n] . SV[h]^T = K[h, n] exactly, in
                         any summation order (one product is non-zero);
  planted landmarks      a_c x ones(128), a_c pairwise distinct positive bf16: every probed class scores landmark c at 64 a_c,
                         so the selected chunk set does not change with the launch;
  the expectation        from the cache's own bookkeeping (expected_tokens): the last prefill_local prompt tokens, the outlier
                         chunks ({0 .. chunks - 1} minus k_landmark_idx), the chunks position_ids names for the attended slots
                         and the generated tokens below kv_len.  The selection itself is not predicted here.

The model of the decode contract (records (m, l, acc) per split / miss tile, combine / merge) works on PLANS: a plan is a
list of records, a record a pair (K rows, V rows) of row lists.  clean plans: standalone_plan, listed_plan, overlapped_plan; the
seeded defects of tests/test_decode_probe_cpu.py edit a plan.

What the read-out cannot see, by construction (attn_probe's section, restated for one query row): a reading (head, class) is
one softmax, and a softmax over a row attended twice and nothing else - or over the same rows all attended twice - equals the
plain one; so a doubled row shows only when its class holds a second attended row in that head, and at kv_len = 1 a doubling of
the single row is invisible.  The tests therefore assert that every reading holds an attended probed row, and two from
kv_len = 256 on.  A row whose K is all zero (an empty slot of a fresh cache) weighs exp2(-522) = 0 next to a probed row and is
invisible too: the cache tests fill every resident slot with probe rows.  Arithmetic is not read out: tests/util.check_attention
holds it."""
import math

import torch

import attn_probe as ap

D = ap.D
SCALE = 1.0 / math.sqrt(D)
KINDS = {"missing": "dropped", "extra": "added", "doubled": "multiplicity", "unreadable": "unreadable"}


class TokenProbe(ap.Probe):
    """Probe whose (kdim, vdim) maps do not change with the launch: K / V (and the factors made of them) are one state for all
    C launches, the query alone steps through the classes."""

    def _maps(self, s):
        return super()._maps(0)

    def queries(self, s):
        """q [bs, Hq, 1, 128] of launch s alone."""
        km, _ = self._maps(s)
        q = torch.zeros(self.bs, self.Hq, 1, D, dtype=torch.bfloat16, device=self.device)
        return q.scatter_(3, torch.gather(km.repeat_interleave(self.G, dim=1), 2, self._classes(s)).unsqueeze(-1), 64.0)


# ------------------------------------------------------------------------------------------------ what the cache needs
def identity_rope(style, max_pos, device="cpu"):
    """cos_sin table [max_pos, 128] (neox: cos[:64] | sin[:64]) or [max_pos, 64] (glm: cos[:32] | sin[:32]) of the angle 0."""
    half = {"neox": 64, "glm": 32}[style]
    t = torch.zeros(max_pos, 2 * half, dtype=torch.bfloat16, device=device)
    t[:, :half] = 1.0
    return t


def token_factors(k, C, rank=160):
    """k bf16 [bs, Hkv, N, 128] of a TokenProbe -> (U [bs, N, rank], SV [bs, Hkv, 128, rank]) bf16 with U[b, n] . SV[b, h]^T ==
    k[b, h, n] exactly: U[b, n] = e_(n % C), SV[b, h][:, t] = k row of class t (64 at kdim(t)) for t < C."""
    bs, Hkv, N, _ = k.shape
    assert C <= min(N, D) and C <= rank
    U = torch.zeros(bs, N, rank, dtype=torch.bfloat16, device=k.device)
    U.scatter_(2, (torch.arange(N, device=k.device) % C).view(1, N, 1).expand(bs, -1, -1), 1.0)
    SV = torch.zeros(bs, Hkv, D, rank, dtype=torch.bfloat16, device=k.device)
    SV[..., :C] = k[:, :, :C].transpose(2, 3)                  # token t < C is the first token of class t
    return U, SV


def planted_landmarks(n, seed=0, device="cpu"):
    """bf16 [n, 128]: landmark c = a_c x ones(128), the a_c pairwise distinct bf16 values in [2^-5, 8) in a random order
    (n <= 1,024: eight binades of 128 values; the scores 64 a_c / sqrt(128) then span 45 e-folds, far inside bf16's range)."""
    assert n <= 1024
    g = torch.Generator().manual_seed(seed)
    bits = (0x3D00 + torch.randperm(1024, generator=g)[:n]).to(torch.int16)         # 0x3D00 = 2^-5, 0x4100 = 8.0
    a = bits.view(torch.bfloat16)
    assert a.unique().numel() == n and bool((a > 0).all())
    return a.view(n, 1).expand(n, D).contiguous().to(device)


def expected_tokens(cache, layer, kv_len, L_ctx, n_tok):
    """bool [bs, Hkv, n_tok] from the cache's bookkeeping AFTER a decode launch: the tokens the attention of this step must
    have covered.  Also asserts that the bookkeeping names no token twice."""
    bs, kv, C, S = cache.batch_size, cache.num_key_value_heads, cache.chunk_size, cache.select_sets
    pos = cache.position_ids[layer].cpu()                                           # [bs, kv, resident]
    lm_idx = cache.k_landmark_idx[layer].cpu()
    if cache.resident_sets == S:
        slots = torch.arange(S).expand(bs, kv, S)
    else:
        slots = cache._dst_slots.view(bs, kv, S).cpu().long()
    exp = torch.zeros(bs, kv, n_tok, dtype=torch.int32)
    exp[:, :, L_ctx - cache.prefill_local:L_ctx] += 1
    gen = kv_len - cache.sparse_end
    assert 0 <= gen <= n_tok - L_ctx
    exp[:, :, L_ctx:L_ctx + gen] += 1
    within = torch.arange(C)
    for b in range(bs):
        for h in range(kv):
            outl = torch.ones(cache.chunks, dtype=torch.bool)
            outl[lm_idx[b, h]] = False
            chunks = torch.cat([outl.nonzero().flatten(), pos[b, h][slots[b, h]]])
            assert int(outl.sum()) == cache.outlier_chunk and bool((chunks >= 0).all()) and bool((chunks < cache.chunks).all())
            exp[b, h].index_add_(0, (chunks.view(-1, 1) * C + within).flatten(), torch.ones(chunks.numel() * C, dtype=torch.int32))
    assert int(exp.max()) == 1, "the bookkeeping names a token twice"
    return exp.bool()


# ------------------------------------------------------------------------------------------------ read-out and check
def per_class(expected, C):
    """expected bool [..., L] -> int64 [..., C]: attended probed rows per class."""
    L = expected.shape[-1]
    full = torch.zeros(expected.shape[:-1] + (D * C,), dtype=torch.int64)
    full[..., :L] = expected
    return full.view(expected.shape[:-1] + (D, C)).sum(-2)


def assert_conditions(expected, C, two):
    """Every (head, class) reading holds an attended probed row; `two`: at least two (a doubling is visible)."""
    n = per_class(expected.cpu(), C)
    assert int(n.min()) >= (2 if two else 1), f"a reading holds {int(n.min())} attended probed rows"
    assert int(n.max()) <= 128


def by_launch(probe, expected_of_launch):
    """expected_of_launch: C tensors bool [bs, Hkv, L], what launch s had to attend (a cache whose selection moves between
    the launches) -> bool [bs, Hq, L]: per query head, key g C + t taken from the launch in which that head probed class t."""
    assert len(expected_of_launch) == probe.C and probe.R == 1
    per_s = torch.stack([e.repeat_interleave(probe.G, dim=1) for e in expected_of_launch]).cpu()        # [C, bs, Hq, L]
    t = (torch.arange(probe.L) % probe.C).view(1, 1, -1)
    s_of = (t - probe.shift.cpu().unsqueeze(-1)) % probe.C                                             # [bs, Hq, L]
    return torch.gather(per_s, 0, s_of.unsqueeze(0)).squeeze(0)


def problems(probe, expected, limit=8):
    """[(sequence, head, row or token, kind)] of a filled probe (R = 1) against expected bool [bs, Hkv, L] (or [bs, Hq, L]:
    by_launch); kind in dropped, added, multiplicity, unreadable.  Empty iff every reading is bit for bit what `expected`
    predicts."""
    assert probe.R == 1 and expected.shape[::2] == (probe.bs, probe.L) and bool(probe.seen.all())
    if expected.shape[1] != probe.Hq or probe.G == 1:
        assert expected.shape[1] == probe.Hkv
        expected = expected.repeat_interleave(probe.G, dim=1)
    exp = expected.to(probe.device).reshape(probe.bs * probe.Hq, probe.L)
    vals = probe.grid.view(probe.bs * probe.Hq, D, probe.C)
    mult = ap.decode_readings(vals, exp, probe.L)
    out = []
    for i, j, kind in ap.defects(mult, exp, probe.L, limit=limit):
        out.append((i // probe.Hq, i % probe.Hq, j, KINDS[kind]))
    return out


def check(probe, expected):
    bad = problems(probe, expected)
    assert not bad, "(sequence, head, row or token, kind): " + ", ".join(map(str, bad))
    return int(expected.sum()) * (probe.G if expected.shape[1] == probe.Hkv else 1)


# ------------------------------------------------------------------------------------------------ the decode contract
def split_ranges(n, splits):
    """[(k0, k1)] of skv_attn_partial_*: per = ceil(n / splits), split s covers [s per, min((s + 1) per, n))."""
    per = -(-n // splits)
    return [(min(s * per, n), min((s + 1) * per, n)) for s in range(splits)]


def standalone_plan(kv_len, rows, splits):
    """Standalone pass over the first min(kv_len, rows) rows (the clamp of a kv_len from device memory)."""
    n = min(kv_len, rows)
    return [(list(range(k0, k1)),) * 2 for k0, k1 in split_ranges(n, splits)]


def listed_rows(kv_len, rows, slots, sparse_start, resident_rows):
    """Row order of the LISTED body: [0, sparse_start), the listed chunks, the rows behind the region."""
    n = min(kv_len, rows)
    if n <= sparse_start:
        return list(range(n))
    region = [sparse_start + 8 * int(s) + c for s in slots for c in range(8)]
    return list(range(sparse_start)) + region + list(range(sparse_start + resident_rows, n))


def listed_plan(kv_len, rows, splits, slots, sparse_start, resident_rows):
    order = listed_rows(kv_len, rows, slots, sparse_start, resident_rows)
    return [([order[i] for i in range(k0, k1)],) * 2 for k0, k1 in split_ranges(len(order), splits)]


def overlapped_plan(kv_len, rows, splits, dst_slots, cnt, sparse_start, resident_rows):
    """Attention inside the fetch launch: `splits` records of the LISTED pass over the hit slots dst_slots[:cnt], then one
    record per miss tile t >= t0 = cnt // 8 holding the live virtual slots j >= cnt of [8 t, 8 t + 8).  -> (plan, round_p)."""
    S = len(dst_slots)
    plan = listed_plan(kv_len, rows, splits, dst_slots[:cnt], sparse_start, resident_rows)
    for t in range(cnt // 8, S // 8):
        r = [sparse_start + 8 * int(dst_slots[j]) + c for j in range(max(8 * t, cnt), 8 * t + 8) for c in range(8)]
        plan.append((r, list(r)))
    return plan, [False] * splits + [True] * (S // 8 - cnt // 8)


def record(q, k, v, krows, vrows, round_p=False):
    """(m [G], l [G], acc [G, 128]) f32 of one record: q [G, 128], k / v [rows, 128] bf16.  round_p: the weights go into P.V
    as bf16 (miss tiles, the all-MFMA body), the row sum stays f32."""
    G = q.shape[0]
    if not krows:
        return torch.full((G,), float("-inf")), torch.zeros(G), torch.zeros(G, D)
    s = (q.float() @ k[krows].float().T) * SCALE
    m = s.amax(1)
    p = torch.exp(s - m.view(-1, 1))
    pv = p.to(torch.bfloat16).float() if round_p else p
    return m, p.sum(1), pv @ v[vrows].float()


def combine(recs, rounded=True):
    """skv_attn_combine_kernel / skv_attn_merge_kernel: out = sum w acc / sum w l, w = exp(m - M), 0 for an empty record.
    rounded=False: the f32 quotient before the bf16 store."""
    m = torch.stack([r[0] for r in recs])                                          # [n, G]
    M = m.amax(0)
    w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - M))
    a = (w.unsqueeze(-1) * torch.stack([r[2] for r in recs])).sum(0)
    l = (w * torch.stack([r[1] for r in recs])).sum(0)
    o = a / l.view(-1, 1)
    return o.to(torch.bfloat16) if rounded else o


def run_plan(q, k, v, plan, round_p=None, rounded=True):
    """q [G, 128], k / v [rows, 128] -> bf16 [G, 128]."""
    round_p = round_p or [False] * len(plan)
    return combine([record(q, k, v, kr, vr, rp) for (kr, vr), rp in zip(plan, round_p)], rounded)


def model_read_out(rows, Hq, Hkv, plans, bs=1, seed=0, round_p=None):
    """All C launches of a row-keyed probe over `rows` buffer rows through the model: plans[b][hk] is the plan of KV head hk of
    sequence b.  -> the filled Probe."""
    probe = ap.Probe(rows, 1, bs=bs, Hq=Hq, Hkv=Hkv, seed=seed)
    G = Hq // Hkv
    for s in range(probe.C):
        q, k, v = probe.inputs(s)
        out = torch.empty(bs, 1, Hq, D, dtype=torch.bfloat16)
        for b in range(bs):
            for hk in range(Hkv):
                out[b, 0, hk * G:(hk + 1) * G] = run_plan(q[b, hk * G:(hk + 1) * G, 0], k[b, hk], v[b, hk], plans[b][hk], round_p)
        probe.read(s, out)
    return probe


def plan_mask(plan, rows):
    """bool [rows]: the rows a clean plan attends (K side)."""
    m = torch.zeros(rows, dtype=torch.bool)
    for kr, _ in plan:
        m[kr] = True
    return m
