"""Decode attention on the device at logit ranges past the f32 exp range: a key that dominates by more than
120 (every other weight exactly 0, every earlier accumulation rescaled by exp(-120) = 0, l = 1: the output IS that key's V row),
two equal dominant keys in different splits, the uniform softmax, and - through the project's tolerance gate, unchanged - a
maximum that moves at every step, whole splits whose merged weight is 0, and V rows 1e8 apart.  Every body the launcher picks is
named by the BODIES table of test_gpu_decode_attention_readout.py and asserted to be the one that runs."""
import pytest
import torch

import wide_range_cases as W
from test_gpu_decode_attention_readout import BODIES, body_of
from util import check_attention, standalone_pass_labels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(5, 32), (77, 16), (300, 8), (2497, 32)]           # (kv_len, splits), as test_sparse_attention uses them
SLACK = 50


def _lib():
    from shadowkv_amd import _lib
    return _lib


def _attend(q, k, v, kv_len, splits, slots=None, select_sets=0, sparse_start=0, resident_sets=0):
    """skv_sparse_attention[_slots] through the C ABI with scale 0.125 -> out bf16 [bs][Hq][128] on the CPU."""
    L = _lib()
    bs, Hq = q.shape[0], q.shape[1]
    Hkv, rows = k.shape[1], k.shape[2]
    ws = torch.empty(L.lib().skv_attn_workspace_bytes(bs, Hq, splits), dtype=torch.uint8, device=DEV)
    out = torch.zeros(bs, Hq, 128, dtype=torch.bfloat16, device=DEV)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    if slots is None:
        rc = L.lib().skv_sparse_attention(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), ws.data_ptr(), 0, kv_len, rows,
                                          rows * 128, bs, Hq, Hkv, 128, splits, W.ATTN_SCALE, st)
    else:
        sd = slots.to(DEV)
        rc = L.lib().skv_sparse_attention_slots(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), ws.data_ptr(), 0, kv_len,
                                                rows, rows * 128, bs, Hq, Hkv, 128, splits, W.ATTN_SCALE, sd.data_ptr(), select_sets,
                                                sparse_start, resident_sets, st)
    L.check(rc, "skv_sparse_attention")
    torch.cuda.synchronize()
    return out.cpu()


def _assert_rows(out, want, G, what, any_zero=False):
    """out bf16 [bs][Hq][128] == want bf16 [bs][Hkv][128] for every query head of the group, bit for bit.  any_zero (the means of
    several rows only): an exact zero may carry either sign - x + (-x) is +0 in f64 and the sign of a zero sum of products
    depends on the order of the sum."""
    got = out.view(torch.int16)
    expf = want.repeat_interleave(G, dim=1).contiguous()
    exp = expf.view(torch.int16)
    ne = got != exp
    if any_zero:
        ne &= ~((out == 0) & (expf == 0))
    bad = ne.any(dim=-1).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} (sequence, head) outputs differ from the expected row, first {bad[0].tolist()}: " \
                             f"{out[tuple(bad[0].tolist())][:4].tolist()} != {want.repeat_interleave(G, dim=1)[tuple(bad[0].tolist())][:4].tolist()}"


@pytest.mark.parametrize("kv_len,splits", SHAPES)
@pytest.mark.parametrize("body", list(BODIES))
def test_dominant_key_is_returned_exactly(body, kv_len, splits):
    """One key 120 or more above every other (130 against a runner-up of exactly 10 in ANOTHER split and ordinary logits |a| <= 8);
    the rows behind kv_len hold logits of 400 and must not be read.  Every (sequence, KV head) of a launch has its dominant key
    at another of the rows of W.dominant_positions; expected: that row of V, bit for bit."""
    bs, Hq, Hkv = BODIES[body]
    assert body.startswith(body_of(bs, Hq, Hkv))
    G, rows = Hq // Hkv, kv_len + SLACK
    pos = W.dominant_positions(kv_len, splits)
    per = -(-kv_len // splits)
    heads = bs * Hkv
    for launch in range(-(-len(pos) // heads)):
        a = W.background_logits(bs, Hkv, rows, 1000 * kv_len + launch)
        a[:, :, kv_len:] = 400.0
        where = torch.empty(bs, Hkv, dtype=torch.long)
        for i in range(heads):
            p = pos[(launch * heads + i) % len(pos)]
            r2 = (p + per) % kv_len                              # the runner-up: one split further on (wrapping)
            if r2 != p:
                a[i // Hkv, i % Hkv, r2] = 10.0
            a[i // Hkv, i % Hkv, p] = 130.0
            where[i // Hkv, i % Hkv] = p
        q, k, v = W.attention_inputs(a, Hq, seed=kv_len + launch)
        out = _attend(q, k, v, kv_len, splits)
        want = torch.gather(v, 2, where.view(bs, Hkv, 1, 1).expand(bs, Hkv, 1, 128)).squeeze(2)
        _assert_rows(out, want, G, f"{body} kv_len {kv_len} splits {splits} dominant rows {where.flatten().tolist()}")


@pytest.mark.parametrize("kv_len,splits", [(300, 8), (2497, 32)])
@pytest.mark.parametrize("body", list(BODIES))
def test_two_equal_dominant_keys_in_different_splits(body, kv_len, splits):
    """Two keys at 130 in different splits: the output is (v1 + v2) / 2 (f64, rounded once; V in sixteenths, so it is a bf16
    number and the expectation does not sit on a rounding boundary)."""
    bs, Hq, Hkv = BODIES[body]
    assert body.startswith(body_of(bs, Hq, Hkv))
    G, rows = Hq // Hkv, kv_len + SLACK
    per = -(-kv_len // splits)
    nsp = -(-kv_len // per)
    g = torch.Generator().manual_seed(kv_len)
    a = W.background_logits(bs, Hkv, rows, 7 * kv_len)
    a[:, :, kv_len:] = 400.0
    v = (torch.randint(-64, 65, (bs, Hkv, rows, 128), generator=g).double() / 16.0)
    want = torch.empty(bs, Hkv, 128, dtype=torch.float64)
    for b in range(bs):
        for h in range(Hkv):
            s1, s2 = torch.randperm(nsp, generator=g)[:2].tolist()
            p1 = s1 * per + int(torch.randint(0, min(per, kv_len - s1 * per), (1,), generator=g))
            p2 = s2 * per + int(torch.randint(0, min(per, kv_len - s2 * per), (1,), generator=g))
            a[b, h, p1] = a[b, h, p2] = 130.0
            want[b, h] = (v[b, h, p1] + v[b, h, p2]) / 2.0
    q, k, vb = W.attention_inputs(a, Hq, seed=kv_len, v=W.bf16_exact(v))
    out = _attend(q, k, vb, kv_len, splits)
    _assert_rows(out, W.bf16_exact(want), G, f"{body} kv_len {kv_len} splits {splits}", any_zero=True)


@pytest.mark.parametrize("kv_len,splits", [(256, 8), (2048, 32), (300, 8), (2497, 32)])
@pytest.mark.parametrize("body", list(BODIES))
def test_uniform_softmax(body, kv_len, splits):
    """q = 0, V integer-valued in [-8, 8]: every weight is 1 / kv_len.  kv_len a power of two: the exact mean, rounded once;
    other lengths: the tolerance gate."""
    bs, Hq, Hkv = BODIES[body]
    assert body.startswith(body_of(bs, Hq, Hkv))
    G, rows = Hq // Hkv, kv_len + SLACK
    g = torch.Generator().manual_seed(kv_len + splits)
    v = torch.randint(-8, 9, (bs, Hkv, rows, 128), generator=g).double()
    q, k, vb = W.attention_inputs(W.background_logits(bs, Hkv, rows, kv_len), Hq, seed=kv_len, v=W.bf16_exact(v))
    q.zero_()
    out = _attend(q, k, vb, kv_len, splits)
    if kv_len & (kv_len - 1) == 0:
        mean = v[:, :, :kv_len].sum(dim=2) / kv_len                       # exact in f64
        _assert_rows(out, mean.float().bfloat16(), G, f"{body} kv_len {kv_len} splits {splits}: the exact mean", any_zero=True)
    else:
        check_attention(f"wide_range uniform {body} [{kv_len}-{splits}]", out.float(), q, k, vb, kv_len, W.ATTN_SCALE,
                        standalone_pass_labels(bs, Hq, Hkv, kv_len, splits))


@pytest.mark.parametrize("kv_len,splits", [(300, 8), (2497, 32)])
@pytest.mark.parametrize("kind", ["rising", "plateau", "vmag"])
@pytest.mark.parametrize("body", list(BODIES))
def test_late_maximum_and_dead_splits(body, kind, kv_len, splits):
    """Through util.check_attention, unchanged (its bound, its flipped-weight allowance, the labels of the pass that runs): see
    W.late_maximum_case.  tests/test_wide_range_cpu.py confirms that the two oracles agree inside the allowance on these inputs."""
    bs, Hq, Hkv = BODIES[body]
    assert body.startswith(body_of(bs, Hq, Hkv))
    a, v = W.late_maximum_case(kind, bs, Hkv, kv_len, splits, seed=kv_len + len(kind))
    q, k, v = W.attention_inputs(a, Hq, seed=kv_len, v=v)
    out = _attend(q, k, v, kv_len, splits)
    check_attention(f"wide_range {kind} {body} [{kv_len}-{splits}]", out.float(), q, k, v, kv_len, W.ATTN_SCALE,
                    standalone_pass_labels(bs, Hq, Hkv, kv_len, splits))


@pytest.mark.parametrize("G", [4, 8])
def test_dominant_key_through_the_slot_list(G):
    """skv_sparse_attention_slots (the listed body): R = 32 resident slots behind 24 front rows, 16 listed per head, 5 generated
    rows.  The unlisted slots and the rows behind kv_len hold logits of 400 (reading one changes the result); the dominant key
    sits, per KV head, on the first front row, the first / last row of the first / last listed chunk, a chunk in the middle of
    the list, and the first / last generated row."""
    bs, Hq, R, n, ss, gen = 1, 32, 32, 16, 24, 5
    Hkv = Hq // G
    assert body_of(bs, Hq, Hkv, listed=True) == "listed"
    kv_len = ss + 8 * R + gen
    rows = kv_len + SLACK
    g = torch.Generator().manual_seed(G)
    slots = torch.stack([torch.randperm(R, generator=g)[:n] for _ in range(Hkv)]).to(torch.int32)
    a = W.background_logits(bs, Hkv, rows, 31 * G)
    a[:, :, kv_len:] = 400.0
    where = torch.empty(bs, Hkv, dtype=torch.long)
    for h in range(Hkv):
        listed = slots[h].tolist()
        for s in set(range(R)) - set(listed):
            a[0, h, ss + 8 * s:ss + 8 * s + 8] = 400.0
        choices = [0, ss + 8 * listed[0], ss + 8 * listed[0] + 7, ss + 8 * listed[-1], ss + 8 * listed[-1] + 7, ss + 8 * listed[n // 2] + 3,
                   ss + 8 * R, kv_len - 1]
        where[0, h] = choices[h % len(choices)]
        a[0, h, where[0, h]] = 130.0
    q, k, v = W.attention_inputs(a, Hq, seed=G)
    from shadowkv_amd import tensor_op
    out = _attend(q, k, v, kv_len, tensor_op.default_attention_splits(bs, Hkv, rows), slots=slots, select_sets=n, sparse_start=ss,
                  resident_sets=R)
    want = torch.gather(v, 2, where.view(bs, Hkv, 1, 1).expand(bs, Hkv, 1, 128)).squeeze(2)
    _assert_rows(out, want, G, f"listed G {G} dominant rows {where.flatten().tolist()}")


# ------------------------------------------------------------------------------------------------------------- prefill
VERTICALS = (0, 7, 100, 131, 255)


def _prefill_dominant_case(L=300, G=4, Hkv=2, bs=1, seed=5):
    """Keys are +-1 codes, query row i of head h is 32 x the code of its dominant column j(i, h) <= i: the dominant logit is
    32 x 128 / sqrt(128) = 362, every other one 32 x (code correlation) / sqrt(128) - asserted below to stay 120 under it.
    j(i, h) cycles through the diagonal, column 0, the last vertical column <= i and a random one.  -> (q [bs][Hq][L][128], k, v
    [bs][Hkv][L][128], j [bs][Hq][L])."""
    g = torch.Generator().manual_seed(seed)
    Hq = G * Hkv
    k = (torch.randint(0, 2, (bs, Hkv, L, 128), generator=g) * 2 - 1).double()
    v = torch.randn(bs, Hkv, L, 128, generator=g).bfloat16()
    j = torch.empty(bs, Hq, L, dtype=torch.long)
    for i in range(L):
        below = [c for c in VERTICALS if c <= i]
        for h in range(Hq):
            kind = (i + h) % 4
            j[:, h, i] = (i, 0, below[-1], below[int(torch.randint(0, len(below), (1,), generator=g))])[kind]
    kq = k.repeat_interleave(G, dim=1)                                                  # [bs][Hq][L][128]
    q = 32.0 * torch.gather(kq, 2, j.unsqueeze(-1).expand(bs, Hq, L, 128))
    logit = torch.einsum("bhid,bhjd->bhij", q, kq) / 128.0 ** 0.5
    dom = torch.gather(logit, 3, j.unsqueeze(-1)).squeeze(-1)
    others = logit.scatter(3, j.unsqueeze(-1), -1e9)
    causal = torch.tril(torch.ones(L, L, dtype=torch.bool))
    assert float((dom - others.masked_fill(~causal, -1e9).max(dim=-1).values).min()) >= 120.0
    return W.bf16_exact(q), W.bf16_exact(k), v, j


@pytest.mark.parametrize("kernel", ["skv_prefill_attention", "skv_vs_sparse_attention"])
def test_prefill_dominant_key_is_returned_exactly(kernel):
    """The two prefill kernels (one tile body, skv_flash_tile.h): q_len = kv_len = 300, G = 4, another dominant key per query
    row and head - the diagonal, column 0, vertical columns.  Expected: that key's V row, bit for bit.  The sparse kernel runs
    with the vertical columns 0, 7, 100, 131, 255 and the slash offset 0 (the diagonal blocks), which hold every dominant key."""
    from shadowkv_amd import tensor_op
    q, k, v, j = _prefill_dominant_case()
    bs, Hq, L, _ = q.shape
    G = Hq // k.shape[1]
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    if kernel == "skv_prefill_attention":
        out = tensor_op.causal_attention_prefill(qd, kd, vd)
    else:
        vi = torch.tensor(VERTICALS, dtype=torch.int32, device=DEV).expand(bs, Hq, len(VERTICALS)).contiguous()
        si = torch.zeros(bs, Hq, 1, dtype=torch.int32, device=DEV)
        out = tensor_op.sparse_prefill_attention(qd, kd, vd, vi, si)
    torch.cuda.synchronize()
    out = out.cpu().permute(0, 2, 1, 3)                                                  # [bs][Hq][L][128]
    want = torch.gather(v.repeat_interleave(G, dim=1), 2, j.unsqueeze(-1).expand(bs, Hq, L, 128))
    bad = (out.contiguous().view(torch.int16) != want.contiguous().view(torch.int16)).any(dim=-1).nonzero()
    assert bad.numel() == 0, f"{kernel}: {bad.shape[0]} (sequence, head, row) outputs differ from the dominant key's V row, first " \
                             f"{bad[0].tolist()} (dominant column {int(j[tuple(bad[0].tolist())])})"


# ------------------------------------------------------------------------------------- overlapped path (fetch launch + merge)
def _dominant_cache(kv_heads, glm, ctx=4608, seed=0, profile=None, qval=16.0):
    """test_gpu_decode_attention_readout.ProbedCache with other contents: token n of KV head h has the key a[h][n] x d (d = 1 on
    the first 8 dimensions), exactly rebuilt from U[n][h] = a[h][n], SV[h][:, h] = d under the identity RoPE table; a in
    (0.25, 1], V in sixteenths.  The query 16 d scores token n at 16 x 8 a / sqrt(128) = 11.3 a: a token with a = 16 is 170 above
    every other one.  The planted landmarks fix the selection."""
    from test_gpu_decode_attention_readout import ProbedCache
    import decode_probe as dp
    from shadowkv_amd import llama
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU

    class DominantCache(ProbedCache):
        def __init__(self):
            style = "glm" if glm else "neox"
            mc = llama.ModelConfig(num_hidden_layers=1, num_key_value_heads=kv_heads, rope_style=style,
                                   rope_theta=10000.0 if glm else 500000.0)
            self.cache = c = ShadowKVCache_CPU(mc, batch_size=1, max_length=ctx, device=DEV, dtype=torch.bfloat16, sparse_budget=2048,
                                               chunk_size=8, rank=160)
            self.slack = c.generated_row_slack_after_prefill(ctx)
            self.ctx, self.n_tok, self.bs, self.kv = ctx, ctx + self.slack, 1, kv_heads
            g = torch.Generator().manual_seed(seed)
            self.a = (0.25 + torch.randint(1, 97, (1, kv_heads, self.n_tok), generator=g).double() / 128.0)
            if profile == "rising":             # the logit 8 a / sqrt(128) grows by 2.8 per token (bf16(4 n): in steps further up)
                self.a = (4.0 * torch.arange(self.n_tok, dtype=torch.float64)).float().bfloat16().double().expand(1, kv_heads, -1).clone()
            self.d = torch.zeros(128, dtype=torch.float64)
            self.d[:8] = 1.0
            self.k = W.bf16_exact(self.a.unsqueeze(-1) * self.d).to(DEV)
            self.v = W.bf16_exact(torch.randint(-64, 65, (1, kv_heads, self.n_tok, 128), generator=g).double() / 16.0).to(DEV)
            if profile == "vmag":               # V rows of magnitude 1e4 next to rows of magnitude 1e-4
                mag = torch.where(torch.rand(1, kv_heads, self.n_tok, 1, generator=g) < 0.5, 1e4, 1e-4)
                self.v = (torch.randn(1, kv_heads, self.n_tok, 128, generator=g) * mag).bfloat16().to(DEV)
            U = torch.zeros(1, ctx, 160, dtype=torch.bfloat16, device=DEV)
            U[0, :, :kv_heads] = W.bf16_exact(self.a[0, :, :ctx].T).to(DEV)
            SV = torch.zeros(1, kv_heads, 128, 160, dtype=torch.bfloat16, device=DEV)
            for h in range(kv_heads):
                SV[0, h, :8, h] = 1.0
            c.U, c.SV = U.unsqueeze(0).contiguous(), SV.unsqueeze(0).contiguous()
            self.cs = dp.identity_rope(style, ctx + 256, DEV)
            self.q = torch.zeros(1, 32, 1, 128, dtype=torch.bfloat16, device=DEV)
            self.q[..., :8] = qval
            c.prefill_kv_cache(self.v[:, :, :ctx].contiguous(), 0, self.k[:, :, :ctx].contiguous(), self.q)
            assert c.k_cache_buffer.shape[-2] - c.sparse_end == self.slack
            self.n_lm = c.k_landmark.shape[-2]
            self.plant(seed)
            c.H2D()
            c.k_cache_buffer[0][:, :, c.sparse_end:] = self.k[:, :, ctx:]
            c.v_cache_buffer[0][:, :, c.sparse_end:] = self.v[:, :, ctx:]
            self.gen = torch.Generator().manual_seed(seed)

    return DominantCache()


def _row_of_token(pc, h, tok):
    """The buffer row of KV head h that holds token tok (found by its V row: the V rows are pairwise distinct)."""
    c = pc.cache
    hit = (c.v_cache_buffer[0][0, h] == pc.v[0, h, tok]).all(dim=-1).nonzero().flatten().tolist()
    assert len(hit) == 1, (h, tok, hit)
    return hit[0]


@pytest.mark.parametrize("kv_heads,glm", [(8, False), (4, True)], ids=["g4", "g8-glm"])
def test_overlapped_path_dominant_keys(kv_heads, glm):
    """select_fetch_attend_inplace + the merge (skv_fetch_kv_attn_inplace, skv_attn_finish_inplace), 84 misses per head.  Launch
    1: per KV head one dominant token - in the first / the last miss chunk (attended from the registers the tile lands in), in a
    hit chunk, in the local window, in a generated row; expected: its V row bit for bit.  Launch 2: two equal dominant tokens, one
    in a miss tile and one resident (hit chunk); expected (v1 + v2) / 2.  The bookkeeping the launch leaves behind must name the
    chunks as the miss / hit they were planned to be."""
    pc = _dominant_cache(kv_heads, glm, seed=kv_heads)
    c, S, G = pc.cache, pc.cache.select_sets, 32 // kv_heads
    assert S == 256 and c.can_overlap_attention()
    kv_len = c.sparse_end + 3
    c.select_fetch_attend_inplace(0, pc.q, pc.cs, kv_len=kv_len)              # the region now holds the planted selection
    torch.cuda.synchronize()
    kinds = ["miss_first", "miss_last", "hit", "local", "generated", "miss_mid", "hit", "local"]
    dvec = W.bf16_exact(16.0 * pc.d).to(DEV)
    for launch in ("one", "two"):
        before = c.position_ids[0][0].cpu()                                   # [kv, S]
        pc.evict(84)
        after = c.position_ids[0][0].cpu()
        want = torch.empty(1, kv_heads, 128, dtype=torch.float64)
        undo, planned, rebuilt = [], [], []
        for h in range(kv_heads):
            misses = sorted(set(before[h].tolist()) - set(after[h].tolist()))
            hits = sorted(set(before[h].tolist()) & set(after[h].tolist()))
            assert len(misses) == 84
            kind = kinds[(h + (4 if kv_heads == 4 else 0)) % len(kinds)] if launch == "one" else "miss_mid"     # (4 heads: the second half)
            toks = []
            if kind.startswith("miss"):
                chunk = {"miss_first": misses[0], "miss_last": misses[-1], "miss_mid": misses[41]}[kind]
                toks.append(8 * chunk + (0 if kind == "miss_first" else 7))
                planned.append((h, "miss", chunk))
            if kind == "hit" or launch == "two":
                chunk = hits[(7 * h) % len(hits)]
                toks.append(8 * chunk + 3)
                planned.append((h, "hit", chunk))
            if kind == "local":
                toks.append(pc.ctx - 1 - h)
            if kind == "generated":
                toks.append(pc.ctx + 1)
            for tok in toks:
                if tok < pc.ctx:
                    undo.append((c.U[0][0, tok], c.U[0][0, tok].clone()))
                    c.U[0][0, tok, h] = 16.0
                resident = tok >= pc.ctx or not (kind.startswith("miss") and tok == toks[0])
                if not resident:
                    rebuilt.append((h, tok))
                else:
                    row = _row_of_token(pc, h, tok)
                    assert row < kv_len
                    undo.append((c.k_cache_buffer[0][0, h, row], c.k_cache_buffer[0][0, h, row].clone()))
                    c.k_cache_buffer[0][0, h, row] = dvec
            want[0, h] = sum(pc.v[0, h, t].double().cpu() for t in toks) / len(toks)
        out = c.select_fetch_attend_inplace(0, pc.q, pc.cs, kv_len=kv_len)
        torch.cuda.synchronize()
        cnts, miss = c.cnts.view(-1).cpu(), c.offsets.view(kv_heads, S).cpu()
        assert cnts.tolist() == [S - 84] * kv_heads, cnts
        for h, what, chunk in planned:
            assert (chunk in miss[h, int(cnts[h]):].tolist()) == (what == "miss"), (h, what, chunk)
        _assert_rows(out.view(1, 32, 128).cpu(), W.bf16_exact(want), G, f"overlapped launch {launch}", any_zero=(launch == "two"))
        for ref, old in undo:
            ref.copy_(old)
        for h, tok in rebuilt:              # the launch rebuilt this token's key row from the patched factor: now resident, put it back
            c.k_cache_buffer[0][0, h, _row_of_token(pc, h, tok)] = pc.k[0, h, tok]


@pytest.mark.parametrize("profile,qval", [("rising", 1.0), ("vmag", 16.0)])
@pytest.mark.parametrize("kv_heads,glm", [(8, False), (4, True)], ids=["g4", "g8-glm"])
def test_overlapped_path_late_maximum_and_v_magnitudes(kv_heads, glm, profile, qval):
    """The overlapped path through util.check_attention, unchanged, with the labels of the launch's own bookkeeping
    (overlapped_pass_labels), 84 misses per head.  rising: the logit grows with the token index, so the maximum sits in the
    generated rows the split pass reads last, every earlier accumulation is rescaled by exp(-large) = 0 and every miss-tile
    record enters the merge with a finite m and weight 0.  vmag: V rows 1e8 apart."""
    import math
    from util import overlapped_pass_labels
    pc = _dominant_cache(kv_heads, glm, seed=kv_heads + len(profile), profile=profile, qval=qval)
    c = pc.cache
    kv_len = c.sparse_end + 3
    c.select_fetch_attend_inplace(0, pc.q, pc.cs, kv_len=kv_len)
    torch.cuda.synchronize()
    pc.evict(84)
    out = c.select_fetch_attend_inplace(0, pc.q, pc.cs, kv_len=kv_len)
    torch.cuda.synchronize()
    assert c.cnts.view(-1).cpu().tolist() == [c.select_sets - 84] * kv_heads
    check_attention(f"wide_range overlapped {profile} g{32 // kv_heads}", out.cpu().float().view(1, 32, 128), pc.q.cpu().view(1, 32, 128),
                    c.k_cache_buffer[0].cpu(), c.v_cache_buffer[0].cpu(), kv_len, 1.0 / math.sqrt(128), overlapped_pass_labels(c, kv_len))
