"""GPU: the exact attended-row set of every decode attention path, read out of the bf16 output with the one-query-row probes of
tests/decode_probe.py.  A case passes only if every (sequence, head, class) reading is bit for bit what
the expectation predicts; a failure names (sequence, head, row or token, kind: dropped / added / multiplicity).  No tolerance:
test_gpu_fused_parity.py::test_sparse_attention and test_gpu_kv_cache.py hold the arithmetic, this file the membership.

Standalone (skv_sparse_attention through the C ABI; the probe is over the kv_len + 50 rows of the buffer, so a read past kv_len
shows as an added row): every body the launcher picks - the case id names it - against kv_len around the 16-key group step,
the 64 / 128 / 256-key tiles of the MFMA bodies and the headline length, and splits 1 .. 62 incl. more splits than keys
(`k0` / `k1`, the `key < k1` mask); kv_len from device memory, also past the rows a head owns (the clamp: every row of the
head, none of the buffer behind it).  Slot list (the LISTED body): shuffled lists of 1, R / 2 and R of R = 32 / 512 slots, the
unlisted slots hold probe rows.  Cache paths (token-keyed, ShadowKVCache_CPU with one layer, identity RoPE, planted landmarks):
select_fetch_attend_inplace (fetch launch + merge) at hit counts S, S - 1, S - 84 (a mixed tile), 8, 1, 0, generated rows 1 / 3
/ the full slack, kv_len from host and device, budgets 1024 / 2048 / 4096 (merge MAXREC 64 and 128), G = 4 and G = 8 (GLM RoPE);
select_fetch_inplace + the standalone pass, also at batch 2; 512 resident slots over 256 selected; early + near-miss staging."""
import pytest
import torch

import attn_probe as ap
import decode_probe as dp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLACK = 50                                   # probed rows behind kv_len


def _lib():
    from shadowkv_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


# -------------------------------------------------------------------------------------------------------- standalone
BODIES = {                                   # id -> (bs, Hq, Hkv); the id is the body skv_launch_sparse_attention picks
    "valu-g1": (1, 8, 8), "valu-g2": (1, 8, 4), "mfma-g4": (1, 32, 8), "mfma-g8": (1, 32, 4), "mfma-g8-bs2": (2, 16, 2),
    "qk-mfma-pv-valu-g4-bs9": (9, 32, 8)}
KV_LENS = [1, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 2497, 2499]
SPLITS = [1, 3, 8, 24, 32, 62]


def body_of(bs, Hq, Hkv, listed=False):
    """The launcher's choice (skv_launch_sparse_attention): a slot list -> the VALU body; G = 8, or G = 4 with at most 64
    (batch, head) pairs -> both products on the MFMA; G = 4 beyond -> Q.K^T on the MFMA, P.V on the VALU; else VALU."""
    G = Hq // Hkv
    if listed:
        return "listed"
    if G == 8 or (G == 4 and bs * Hkv <= 64):
        return "mfma"
    return "qk-mfma-pv-valu" if G == 4 else "valu"


def _standalone_cases():
    seen, out = set(), []

    def add(body, kv_len, splits, length="host"):
        if (body, kv_len, splits, length) not in seen:
            seen.add((body, kv_len, splits, length))
            out.append(pytest.param(body, kv_len, splits, length, id=f"{body}-kv{kv_len}-s{splits}-{length}"))

    for bi, body in enumerate(BODIES):
        for ki, kv_len in enumerate(KV_LENS):                      # every kv_len meets every body, the splits rotate
            add(body, kv_len, SPLITS[(ki + bi) % len(SPLITS)])
        for kv_len, splits in ((2499, 1), (2497, 62), (5, 62), (17, 24)):
            add(body, kv_len, splits)                              # splits 1 and 62, more splits than keys
        add(body, 129, 8, "device")                                # kv_len from device memory: the same value ...
        add(body, 2499, 32, "device")
        add(body, 257, 3, "clamped")                               # ... and one past the rows the head owns
    add("mfma-g4", 17, 62, "clamped")
    add("mfma-g8", 1000, 24, "clamped")
    return out


@pytest.mark.parametrize("body,kv_len,splits,length", _standalone_cases())
def test_standalone(body, kv_len, splits, length):
    bs, Hq, Hkv = BODIES[body]
    assert body.startswith(body_of(bs, Hq, Hkv))
    own = kv_len + SLACK                                           # rows the head owns
    L = 2 * own if length == "clamped" else own                    # clamped: the buffer of a second head right behind it
    n_att = own if length == "clamped" else kv_len
    probe = ap.Probe(L, 1, bs=bs, Hq=Hq, Hkv=Hkv, device=DEV, seed=kv_len + splits)
    expected = (torch.arange(L) < n_att).expand(bs, Hkv, L)
    # the model meets the conditions on these inputs (before any launch)
    asked = own + 1000 if length == "clamped" else kv_len
    assert torch.equal(dp.plan_mask(dp.standalone_plan(asked, own, splits), L), expected[0, 0])
    dp.assert_conditions(expected, probe.C, two=kv_len >= 256)
    lib = _lib()
    ws = torch.empty(lib.lib().skv_attn_workspace_bytes(bs, Hq, splits), dtype=torch.uint8, device=DEV)
    out = torch.zeros(bs, 1, Hq, 128, dtype=torch.bfloat16, device=DEV)
    kv_dev = torch.tensor([asked], dtype=torch.int32, device=DEV)
    kvp, host_len = (0, kv_len) if length == "host" else (kv_dev.data_ptr(), 0)
    for s in range(probe.C):
        q, k, v = probe.inputs(s)
        assert k.is_contiguous() and k.shape == (bs, Hkv, L, 128) and own <= L
        rc = lib.lib().skv_sparse_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), ws.data_ptr(), kvp, host_len,
                                            own, L * 128, bs, Hq, Hkv, 128, splits, dp.SCALE, _stream())
        lib.check(rc, "skv_sparse_attention")
        probe.read(s, out)
    torch.cuda.synchronize()
    assert dp.check(probe, expected) == bs * Hq * n_att


# --------------------------------------------------------------------------------------------------------- slot list
@pytest.mark.parametrize("G", [4, 8])
@pytest.mark.parametrize("R,n", [(32, 1), (32, 16), (32, 32), (512, 1), (512, 256), (512, 512)])
def test_slot_list(G, R, n):
    """The LISTED body: of the R slots behind row ss only the n listed ones, in shuffled order, another list per head."""
    from shadowkv_amd import tensor_op
    bs, Hq, Hkv, gen = 1, 32, 32 // G, 5
    ss = 24 if R == 32 else 72               # (72 rows in front of the region: two of each of the 33 classes even at n = 1)
    assert body_of(bs, Hq, Hkv, listed=True) == "listed"
    kv_len = ss + 8 * R + gen
    rows = kv_len + SLACK
    probe = ap.Probe(rows, 1, bs=bs, Hq=Hq, Hkv=Hkv, device=DEV, seed=R + n + G)
    g = torch.Generator().manual_seed(R + n)
    slots = torch.stack([torch.randperm(R, generator=g)[:n] for _ in range(Hkv)]).to(torch.int32)
    splits = tensor_op.default_attention_splits(bs, Hkv, rows)
    expected = torch.stack([dp.plan_mask(dp.listed_plan(kv_len, rows, splits, slots[h].tolist(), ss, 8 * R), rows)
                            for h in range(Hkv)]).view(1, Hkv, rows)
    assert int(expected.sum()) == Hkv * (ss + 8 * n + gen)
    dp.assert_conditions(expected, probe.C, two=True)
    slots_dev = slots.to(DEV)
    for s in range(probe.C):
        q, k, v = probe.inputs(s)
        probe.read(s, tensor_op.sparse_attention_decode(q, k, v, kv_len=kv_len, slots=slots_dev, select_sets=n, sparse_start=ss,
                                                        resident_sets=R))
    torch.cuda.synchronize()
    assert dp.check(probe, expected) == Hq * (ss + 8 * n + gen)


def test_slot_list_of_no_slot_is_refused():
    """n_slots = 0 has no read-out: the API refuses an empty list (select_sets < 1) before any launch."""
    from shadowkv_amd import tensor_op
    from shadowkv_amd._lib import ShadowKVNativeError
    probe = ap.Probe(24 + 256 + 5, 1, bs=1, Hq=32, Hkv=8, device=DEV)
    q, k, v = probe.inputs(0)
    with pytest.raises(ShadowKVNativeError):
        tensor_op.sparse_attention_decode(q, k, v, kv_len=probe.L, slots=torch.zeros(8, 1, dtype=torch.int32, device=DEV),
                                          select_sets=0, sparse_start=24, resident_sets=32)


# ------------------------------------------------------------------------------------------------------- cache paths
class ProbedCache:
    """One-layer ShadowKVCache_CPU over a ctx-token prompt whose U / SV / K / V are the token-keyed probe's, with the identity
    RoPE table and planted landmarks; every generated-row slot behind the sparse region holds the probe's generated tokens."""

    def __init__(self, kv_heads, glm, ctx, budget=2048, resident=None, bs=1, seed=0):
        from shadowkv_amd import llama
        from shadowkv_amd.kv_cache import ShadowKVCache_CPU
        style = "glm" if glm else "neox"
        mc = llama.ModelConfig(num_hidden_layers=1, num_key_value_heads=kv_heads, rope_style=style,
                               rope_theta=10000.0 if glm else 500000.0)
        self.cache = c = ShadowKVCache_CPU(mc, batch_size=bs, max_length=ctx, device=DEV, dtype=torch.bfloat16, sparse_budget=budget,
                                           chunk_size=8, rank=160, resident_sets=resident)
        self.slack = c.generated_row_slack_after_prefill(ctx)                 # rows behind the sparse region (96)
        self.ctx, self.n_tok, self.bs, self.kv = ctx, ctx + self.slack, bs, kv_heads
        self.probe = dp.TokenProbe(self.n_tok, 1, bs=bs, Hq=32, Hkv=kv_heads, device=DEV, seed=seed)
        q, self.k, self.v = self.probe.inputs(0)
        U, SV = dp.token_factors(self.k[:, :, :ctx], self.probe.C)
        c.U, c.SV = U.unsqueeze(0).contiguous(), SV.unsqueeze(0).contiguous()
        self.cs = dp.identity_rope(style, ctx + 256, DEV)
        c.prefill_kv_cache(self.v[:, :, :ctx].contiguous(), 0, self.k[:, :, :ctx].contiguous(), q)
        assert c.k_cache_buffer.shape[-2] - c.sparse_end == self.slack
        self.n_lm = c.k_landmark.shape[-2]
        self.plant(seed)
        c.H2D()
        c.k_cache_buffer[0][:, :, c.sparse_end:] = self.k[:, :, ctx:]
        c.v_cache_buffer[0][:, :, c.sparse_end:] = self.v[:, :, ctx:]
        self.gen = torch.Generator().manual_seed(seed)

    def plant(self, seed, moved=0.0):
        """Planted landmarks, another order per (sequence, head); moved: that share of them trade places (the selection of
        the next launch then differs by a few chunks)."""
        c = self.cache
        for b in range(self.bs):
            for h in range(self.kv):
                lm = dp.planted_landmarks(self.n_lm, seed=1000 * b + h)
                if moved:
                    g = torch.Generator().manual_seed(seed + 7 * h + b)
                    idx = torch.randperm(self.n_lm, generator=g)[:int(moved * self.n_lm)]
                    lm[idx] = lm[idx[torch.randperm(idx.numel(), generator=g)]]
                c.k_landmark[0][b, h].copy_(lm.to(DEV))

    def write_slots(self, b, h, slots, chunks):
        """Makes slot slots[i] of (b, h) hold chunk chunks[i]: the map and the K / V rows."""
        c = self.cache
        within = torch.arange(8)
        rows = (c.sparse_start + slots.view(-1, 1) * 8 + within).flatten().to(DEV)
        tok = (chunks.view(-1, 1) * 8 + within).flatten().to(DEV)
        c.position_ids[0][b, h, slots.to(DEV)] = chunks.to(DEV)
        c.k_cache_buffer[0][b, h, rows] = self.k[b, h, tok]
        c.v_cache_buffer[0][b, h, rows] = self.v[b, h, tok]

    def attended_slots(self):
        c, S = self.cache, self.cache.select_sets
        if c.resident_sets == S:
            return torch.arange(S).expand(self.bs, self.kv, S)
        return c._dst_slots.view(self.bs, self.kv, S).cpu().long()

    def fill_empty_slots(self):
        """Resident set larger than the selection: the slots still empty get chunks outside the selection, so that a
        resident-but-unselected slot holds probe rows."""
        pos, lm_idx = self.cache.position_ids[0].cpu(), self.cache.k_landmark_idx[0].cpu()
        for b in range(self.bs):
            for h in range(self.kv):
                empty = (pos[b, h] < 0).nonzero().flatten()
                pool = torch.tensor(sorted(set(lm_idx[b, h].tolist()) - set(pos[b, h].tolist())))
                assert empty.numel() and pool.numel() >= empty.numel()
                self.write_slots(b, h, empty, pool[torch.randperm(pool.numel(), generator=self.gen)[:empty.numel()]])

    def evict(self, n_miss):
        """Re-creates the miss pattern: n_miss of the attended slots of every head now hold a chunk outside the resident set,
        so the next launch with the same landmarks misses exactly n_miss chunks."""
        if not n_miss:
            return
        pos, lm_idx, att = self.cache.position_ids[0].cpu(), self.cache.k_landmark_idx[0].cpu(), self.attended_slots()
        for b in range(self.bs):
            for h in range(self.kv):
                pool = torch.tensor(sorted(set(lm_idx[b, h].tolist()) - set(pos[b, h].tolist())))
                assert pool.numel() >= n_miss, "the context is too short for this miss count"
                slots = att[b, h][torch.randperm(att.shape[-1], generator=self.gen)[:n_miss]]
                self.write_slots(b, h, slots, pool[torch.randperm(pool.numel(), generator=self.gen)[:n_miss]])

    def read_out(self, overlap, cnt=None, gen=3, kv_from="host", moved=0.0, after_launch=None):
        """C launches; before each, the miss pattern is re-created (cnt hits per head; None: whatever the selection gives).
        Each launch is held to the bookkeeping IT left behind."""
        from shadowkv_amd import tensor_op
        c, probe, S = self.cache, self.probe, self.cache.select_sets
        kv_len = c.sparse_end + gen
        kv_dev = torch.tensor([kv_len], dtype=torch.int32, device=DEV)
        kw = dict(kv_len=kv_len) if kv_from == "host" else dict(kv_len=0, kv_len_dev=kv_dev)
        assert overlap is False or c.can_overlap_attention()

        def launch(q):
            if overlap:
                return c.select_fetch_attend_inplace(0, q, self.cs, **kw)
            c.select_fetch_inplace(0, q, self.cs)
            kw2 = dict(kv_len=kv_len) if kv_from == "host" else dict(kv_len_dev=kv_dev)
            return tensor_op.sparse_attention_decode(q, c.k_cache_buffer[0], c.v_cache_buffer[0], **kw2, **c.attend_slot_args())

        launch(probe.queries(0))                                  # the region now holds the planted selection
        torch.cuda.synchronize()
        if c.resident_sets > S:
            self.fill_empty_slots()
        expected, hits = [], []
        for s in range(probe.C):
            if moved:
                self.plant(s + 1, moved)
            if cnt is not None:
                self.evict(S - cnt)
            out = launch(probe.queries(s))
            torch.cuda.synchronize()
            hits.append(c.cnts.cpu().tolist())
            expected.append(dp.expected_tokens(c, 0, kv_len, self.ctx, self.n_tok))
            probe.read(s, out)
            if after_launch is not None:
                after_launch(c)
        if cnt is not None:
            assert hits == [[cnt] * (self.bs * self.kv)] * probe.C, hits[:2]
        exp = dp.by_launch(probe, expected)
        dp.assert_conditions(exp, probe.C, two=True)
        n_att = c.prefill_local + 8 * c.outlier_chunk + 8 * S + gen
        assert all(int(e.sum()) == self.bs * self.kv * n_att for e in expected)
        assert dp.check(probe, exp) == int(exp.sum())           # (per query head: each class from the launch that read it)
        return hits


CTX = 4608                                   # 520 landmarks: 256 selected + the 264 a launch with no hit replaces them from


def _overlap_cases():
    out = []
    for kv_heads, glm in ((8, False), (4, True)):
        S = 256
        for i, cnt in enumerate((S, S - 1, S - 84, 8, 1, 0)):
            gen = (1, 3, 96)[(i + kv_heads // 4) % 3]
            kv_from = ("host", "device")[(i + kv_heads // 8) % 2]
            out.append(pytest.param(kv_heads, glm, cnt, gen, kv_from, id=f"g{32 // kv_heads}-cnt{cnt}-gen{gen}-{kv_from}"))
        out.append(pytest.param(kv_heads, glm, S - 84, 96 if kv_heads == 8 else 1, "device" if kv_heads == 8 else "host",
                                id=f"g{32 // kv_heads}-cnt{S - 84}-mixed-tile-again"))
    return out


@pytest.mark.parametrize("kv_heads,glm,cnt,gen,kv_from", _overlap_cases())
def test_overlapped(kv_heads, glm, cnt, gen, kv_from):
    """select_fetch_attend_inplace at budget 2048 (24 split records + 32 tile records, MAXREC 64): a chunk is attended by the
    split pass over the hit slots or by the workgroup of its miss tile, never both, never neither; cnt % 8 != 0 puts both kinds
    into tile t0 = cnt / 8."""
    pc = ProbedCache(kv_heads, glm, CTX, seed=cnt + kv_heads)
    assert pc.cache.select_sets == 256 and (pc.cache.sparse_start, pc.cache.sparse_end, pc.slack) == (448, 2496, 96)
    pc.read_out(True, cnt=cnt, gen=gen, kv_from=kv_from)


@pytest.mark.parametrize("budget,ctx,kv_heads,glm,cnt", [(4096, 8192, 8, False, 512 - 84), (1024, 2560, 4, True, 128 - 84)])
def test_overlapped_other_budgets(budget, ctx, kv_heads, glm, cnt):
    """Budget 4096: S = 512, 24 + 64 records, the MAXREC = 128 merge instance; budget 1024: S = 128."""
    pc = ProbedCache(kv_heads, glm, ctx, budget=budget, seed=budget)
    assert pc.cache.select_sets == budget // 8 and cnt % 8 == 4
    pc.read_out(True, cnt=cnt, gen=3)


@pytest.mark.parametrize("kv_heads,glm,bs,cnt,kv_from", [(8, False, 1, 172, "host"), (4, True, 1, 0, "device"), (8, False, 2, 172, "host")])
def test_plain_path(kv_heads, glm, bs, cnt, kv_from):
    """select_fetch_inplace + sparse_attention_decode from the same state; batch 2 is where can_overlap_attention() is false."""
    pc = ProbedCache(kv_heads, glm, CTX, bs=bs, seed=bs)
    assert pc.cache.can_overlap_attention() == (bs == 1)
    pc.read_out(False, cnt=cnt, gen=3, kv_from=kv_from)


@pytest.mark.parametrize("overlap", [True, False], ids=["overlapped", "standalone-listed"])
def test_resident_set_of_512_slots(overlap):
    """resident_sets = 512 > select_sets = 256: the 256 slots outside the selection hold probe rows of other chunks and must
    not be read; the attended slots are _dst_slots."""
    pc = ProbedCache(8, False, 8192, resident=512, seed=3)
    assert pc.cache.resident_sets == 512 and pc.cache.sparse_end == 448 + 4096
    pc.read_out(overlap, cnt=256 - 84, gen=3)


def test_early_and_near_staging():
    """enable_early_fetch(near=True), the staging the benchmark runs with: the landmarks move between the launches, so every
    launch selects a few other chunks - some staged early in the step, some staged ahead by the gate/up and down launches
    of the step before - and must attend exactly what its bookkeeping names."""
    from test_gpu_kv_cache import _check_staging_invariant, _gate_up_with_near_pull
    pc = ProbedCache(8, False, CTX, seed=5)
    pc.cache.near_lists = 2
    pc.cache.enable_early_fetch(near=True)
    gw = torch.Generator(device=DEV).manual_seed(9)

    def after(c):
        _gate_up_with_near_pull(c, 0, gw)
        _check_staging_invariant(c, 0)

    hits = pc.read_out(True, cnt=None, gen=3, moved=0.3, after_launch=after)
    flat = [x for h in hits for x in h]
    assert min(flat) < 256 and max(flat) > 0                        # there were misses to stage for
    pulled, used, _ = pc.cache.early_fetch_stats(0)
    assert pulled > 0
