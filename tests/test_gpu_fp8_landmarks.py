"""GPU: the FP8 (e4m3) landmark table.

scale * e4m3(byte) with a power-of-two scale is a bf16 number, so the FP8 scan has a bf16 TWIN - the same entry, the same cache
or the same model with k_landmark = dequant(FP8 table) - and must equal it bit for bit: logits, keys, partials and everything
the selection, the fetch and the model make of them.  Every comparison here is torch.equal or a bit-pattern compare."""
import functools
import math

import pytest
import torch

import fp8_v_ref as R
import gen_inputs as G
from test_fp8_landmarks_cpu import check_fp8_landmark_cache_against_reference_and_twin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALPHA = 1.0 / math.sqrt(128)


def _lib():
    from shadowkv_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _i16(t):
    return t.contiguous().view(torch.int16)


def _i32(t):
    return t.contiguous().view(torch.int32)


def _scan(fp8, q, lm, scale, blocks, Gq, N, alpha=ALPHA):
    """skv_score_landmarks[_fp8] -> (D bf16 [blocks, G, N], part_max, part_sum f32 [blocks, T, G]) on the CPU."""
    L = _lib()
    T = (N + 255) // 256
    D = torch.full((blocks, Gq, N), -3.0, dtype=torch.bfloat16, device=DEV)
    pm = torch.full((blocks, T, Gq), -5.0, dtype=torch.float32, device=DEV)
    ps = torch.full((blocks, T, Gq), -5.0, dtype=torch.float32, device=DEV)
    if fp8:
        L.check(L.lib().skv_score_landmarks_fp8(q.data_ptr(), lm.data_ptr(), scale.data_ptr(), D.data_ptr(), pm.data_ptr(),
                                                ps.data_ptr(), blocks, Gq, N, alpha, _stream()), "score_landmarks_fp8")
    else:
        L.check(L.lib().skv_score_landmarks(q.data_ptr(), lm.data_ptr(), D.data_ptr(), pm.data_ptr(), ps.data_ptr(), blocks, Gq, N,
                                            alpha, _stream()), "score_landmarks")
    torch.cuda.synchronize()
    return D.cpu(), pm.cpu(), ps.cpu()


# ------------------------------------------------------------------------------------------------ 1. decode of every code
CODES = [c for c in range(256) if (c & 0x7F) != 0x7F]                   # the 254 non-NaN e4m3fn codes


def test_scan_decodes_every_code_at_every_byte_position():
    """One non-zero byte per row, q = ones, alpha = 1: the logit IS bf16(scale * e4m3(code)).  Code c sits in four rows, at byte
    (c + 3 j) % 8 of lane (c + 5 j) % 16, j = 0..3 - all 8 byte positions of a lane's load and all 16 lanes over the set."""
    N, Gq = len(CODES) * 4, 4
    table = torch.zeros(N, 128, dtype=torch.uint8)
    code_of = torch.zeros(N, dtype=torch.int64)
    seen = set()
    for i, c in enumerate(CODES):
        for j in range(4):
            byte, lane = (c + 3 * j) % 8, (c + 5 * j) % 16
            table[4 * i + j, 8 * lane + byte] = c
            code_of[4 * i + j] = c
            seen.add((byte, lane))
    assert {b for b, _ in seen} == set(range(8)) and {l for _, l in seen} == set(range(16))
    scales = [torch.full((N,), 2.0 ** k) for k in (-100, -3, 0, 5, 100)]
    scales.append(torch.ldexp(torch.ones(N), (torch.arange(N) * 7) % 61 - 30))          # a scale of its own per row
    blocks = len(scales)
    scale = torch.stack(scales).float()
    lm = table.unsqueeze(0).expand(blocks, -1, -1).contiguous()
    q = torch.ones(blocks, Gq, 128, dtype=torch.bfloat16)
    D, pm, ps = _scan(True, q.to(DEV), lm.to(DEV), scale.to(DEV), blocks, Gq, N, alpha=1.0)
    val = torch.tensor(CODES, dtype=torch.uint8).view(torch.float8_e4m3fn).double()
    val = dict(zip(CODES, val.tolist()))
    want64 = torch.tensor([val[int(c)] for c in code_of], dtype=torch.float64).unsqueeze(0) * scale.double()      # [blocks, N]
    want = want64.to(torch.bfloat16)
    assert torch.equal(want.double(), want64), "scale * e4m3(code) is a bf16 number"
    for g in range(Gq):
        bad = (D[:, g].float() != want.float()).nonzero()
        assert bad.numel() == 0, f"head {g}: {bad.shape[0]} logits differ, first (block, row) {bad[0].tolist()}: code " \
                                 f"{int(code_of[bad[0][1]])}, got {float(D[bad[0][0], g, bad[0][1]])}, want {float(want[bad[0][0], bad[0][1]])}"
    # and the same bits as the bf16 scan over the dequantised table (the sign of a zero included)
    deq = R.dequantize_rows(lm, scale)[0]
    D2, pm2, ps2 = _scan(False, q.to(DEV), deq.to(DEV), None, blocks, Gq, N, alpha=1.0)
    assert torch.equal(_i16(D), _i16(D2)) and torch.equal(_i32(pm), _i32(pm2)) and torch.equal(_i32(ps), _i32(ps2))


# ------------------------------------------------------------------------------------------------ 2. the scan on the twin
def twin_rows(blocks, N, gen):
    """bf16 landmark rows [blocks, N, 128]: Gaussian times 2^u, u in [-12, 12] per row; an all-zero row; rows whose largest
    magnitude is exactly 448 * 2^k and one bf16 step above it (450 * 2^k: the scale doubles)."""
    u = torch.randint(-12, 13, (blocks, N, 1), generator=gen)
    rows = torch.ldexp(torch.randn(blocks, N, 128, generator=gen), u).to(torch.bfloat16)
    if N >= 7:
        rows[0, 3] = 0
        for r, (top, k) in zip((1, 2, 4, 5), ((448.0, -7), (450.0, -7), (-448.0, 3), (-450.0, 3))):
            base = (torch.randn(128, generator=gen) * 50).clamp(-400, 400) * 2.0 ** k
            base[(11 * r) % 128] = top * 2.0 ** k
            rows[-1, r] = base.to(torch.bfloat16)
    return rows


@functools.lru_cache(maxsize=None)
def _twin_case(blocks, N, seed=0):
    gen = torch.Generator().manual_seed(1000 * blocks + N + seed)
    rows = twin_rows(blocks, N, gen)
    b, s = R.quantize_rows(rows)
    deq = R.dequantize_rows(b, s)[0]
    if N >= 7:
        assert float(s[0, 3]) == 1.0 and not bool(b[0, 3].any())
        assert float(s[-1, 1]) * 2 == float(s[-1, 2]) and float(s[-1, 4]) * 2 == float(s[-1, 5])     # 448: fits; 450: the next scale
    return rows, b, s, deq


@pytest.mark.parametrize("Gq", [1, 2, 4, 8, 16])
def test_fp8_scan_equals_the_bf16_scan_of_the_dequantised_table(Gq):
    """D, part_max, part_sum bit for bit at the tile edge (255 / 256 / 257), with clamped last rows (1, 7, 1000) and masked last
    tiles, for one and three blocks."""
    for blocks in (1, 3):
        for N in (1, 7, 255, 256, 257, 1000):
            _, b, s, deq = _twin_case(blocks, N)
            gen = torch.Generator().manual_seed(17 * N + Gq)
            q = (torch.randn(blocks, Gq, 128, generator=gen) * 2).to(torch.bfloat16).to(DEV)
            Da, pa, sa = _scan(True, q, b.to(DEV), s.to(DEV), blocks, Gq, N)
            Db, pb, sb = _scan(False, q, deq.to(DEV), None, blocks, Gq, N)
            what = f"G {Gq}, blocks {blocks}, N {N}"
            assert torch.equal(_i16(Da), _i16(Db)), f"{what}: logits"
            assert torch.equal(_i32(pa), _i32(pb)), f"{what}: part_max"
            assert torch.equal(_i32(sa), _i32(sb)), f"{what}: part_sum"
            assert bool(torch.isfinite(Da.float()).all())


# ------------------------------------------------------------------------------------------------ 3. the selection chain
class _Chain:
    """One selection entry over consecutive steps from one resident set; holds every buffer the entry writes."""

    def __init__(self, entry, fp8, lm, scale, lm_idx, cached0, blocks, Gq, N, S, Rs, inplace):
        L = _lib().lib()
        self.entry, self.fp8, self.inplace = entry, fp8, inplace
        self.lm, self.scale, self.lid = lm.to(DEV), None if scale is None else scale.to(DEV), lm_idx.to(DEV)
        self.dims = (blocks, Gq, N, S, Rs)
        self.ws = torch.zeros(L.skv_select_workspace_bytes(blocks, Gq, N), dtype=torch.uint8, device=DEV)
        self.state = torch.zeros(L.skv_select_state_bytes(blocks, Gq), dtype=torch.uint8, device=DEV)
        self.cached = torch.full((blocks, Rs), -1, dtype=torch.int64, device=DEV)
        self.cached[:, :S] = cached0.to(DEV)
        self.age = torch.zeros(blocks, Rs, dtype=torch.int32, device=DEV)
        self.offsets = torch.full((blocks, S), -7, dtype=torch.int32, device=DEV)
        self.dst = torch.full((blocks, S), -7, dtype=torch.int32, device=DEV)
        self.cnts = torch.zeros(blocks, dtype=torch.int32, device=DEV)
        self.sel = torch.zeros(blocks, S, dtype=torch.int64, device=DEV)

    def step(self, q):
        Lm = _lib()
        L = Lm.lib()
        blocks, Gq, N, S, Rs = self.dims
        lm = (self.lm.data_ptr(), self.scale.data_ptr()) if self.fp8 else (self.lm.data_ptr(),)
        sfx = "_fp8" if self.fp8 else ""
        if self.entry == "select_chunks":
            rc = getattr(L, "skv_select_chunks" + sfx)(q.data_ptr(), *lm, self.lid.data_ptr(), self.cached.data_ptr(),
                                                       self.offsets.data_ptr(), self.cnts.data_ptr(), self.ws.data_ptr(), 0,
                                                       self.sel.data_ptr(), blocks, Gq, N, S, ALPHA, _stream())
        elif self.entry == "select_chunks_inplace":
            rc = getattr(L, "skv_select_chunks_inplace" + sfx)(q.data_ptr(), *lm, self.lid.data_ptr(), self.cached.data_ptr(),
                                                               self.offsets.data_ptr(), self.dst.data_ptr(), self.cnts.data_ptr(),
                                                               self.ws.data_ptr(), 0, self.sel.data_ptr(), blocks, Gq, N, S, Rs,
                                                               self.age.data_ptr(), ALPHA, _stream())
        else:
            args = (q.data_ptr(), *lm, self.lid.data_ptr(), self.cached.data_ptr(), self.offsets.data_ptr(),
                    self.dst.data_ptr() if self.inplace else 0, self.cnts.data_ptr(), self.ws.data_ptr(), self.sel.data_ptr(),
                    blocks, Gq, N, S, Rs, self.age.data_ptr() if self.inplace else 0, ALPHA, self.state.data_ptr(), 0, 0, 0, 0, 0, 0.0)
            rc = L.skv_select_chunks_fused_fp8(*args, None, _stream()) if self.fp8 else L.skv_select_chunks_fused(*args, _stream())
        Lm.check(rc, self.entry + sfx)
        torch.cuda.synchronize()

    def buffers(self):
        return dict(cached_pos_ids=self.cached, offsets=self.offsets, dst_slots=self.dst, cnts=self.cnts, slot_age=self.age,
                    selected=self.sel, workspace=self.ws, select_state=self.state)


@functools.lru_cache(maxsize=None)
def _chain_inputs(blocks, Gq, N, S):
    gen = torch.Generator().manual_seed(31 * N + Gq)
    rows, b, s, deq = _twin_case(blocks, N, seed=5)
    lm_idx = torch.stack([torch.sort(torch.randperm(N + 48, generator=gen)[:N]).values for _ in range(blocks)]).to(torch.int64)
    cached0 = torch.stack([lm_idx[i][torch.randperm(N, generator=gen)[:S]] for i in range(blocks)])
    q = torch.randn(blocks, Gq, 128, generator=gen) * 2.0
    qs = [q.to(torch.bfloat16)]
    for t in range(2):                                         # a drifting query, then a jump
        q = q + 0.3 * torch.randn(blocks, Gq, 128, generator=gen) if t == 0 else torch.randn(blocks, Gq, 128, generator=gen) * 3.0
        qs.append(q.to(torch.bfloat16))
    return b, s, deq, lm_idx, cached0, qs


@pytest.mark.parametrize("entry,inplace,resident2x", [
    ("select_chunks", False, False),
    ("select_chunks_inplace", True, False),
    ("select_chunks_inplace", True, True),                     # resident_sets > select_sets
    ("select_chunks_fused", False, False),
    ("select_chunks_fused", True, False),
    ("select_chunks_fused", True, True),
])
@pytest.mark.parametrize("Gq", [4, 8])
def test_fp8_selection_equals_its_bf16_namesake_on_the_twin(Gq, entry, inplace, resident2x):
    """Three consecutive steps (the fused form carries its select state): resident ids, offsets / miss ids, destination slots,
    hit counts, slot ages, the selected ids, the whole workspace and the whole select state (diagnostics included)."""
    blocks, N, S = 3, 4100, 32
    Rs = 2 * S if resident2x else S
    b, s, deq, lm_idx, cached0, qs = _chain_inputs(blocks, Gq, N, S)
    A = _Chain(entry, True, b, s, lm_idx, cached0, blocks, Gq, N, S, Rs, inplace)
    B = _Chain(entry, False, deq, None, lm_idx, cached0, blocks, Gq, N, S, Rs, inplace)
    for t, q in enumerate(qs):
        A.step(q.to(DEV)); B.step(q.to(DEV))
        for (name, x), y in zip(A.buffers().items(), B.buffers().values()):
            assert torch.equal(x, y), f"{entry} step {t}: {name}"
        cn = A.cnts.cpu()
        assert bool(((cn >= 0) & (cn <= S)).all())
    if entry == "select_chunks" and Gq == 4:                   # ... and against the oracle run on the dequantised table
        import oracle
        T = (N + 255) // 256
        D = torch.zeros(blocks, Gq, N, dtype=torch.bfloat16); P = torch.zeros_like(D)
        C = _Chain(entry, True, b, s, lm_idx, cached0, blocks, Gq, N, S, Rs, inplace)
        C.step(qs[0].to(DEV))
        oracle.batch_gemm_softmax(qs[0], deq, D, torch.zeros(blocks, T, Gq), torch.zeros(blocks, T, Gq), P, blocks, Gq, N, 128, ALPHA)
        sel = oracle.group_max_topk(P, lm_idx, blocks, Gq, N, S)
        c0 = cached0.clone(); off0 = torch.zeros(blocks, S, dtype=torch.int32); cnt0 = torch.zeros(blocks, dtype=torch.int32)
        oracle.reorder_keys_and_compute_offsets(c0, sel, off0, cnt0, 1, blocks, S)
        assert torch.equal(c0, C.cached.cpu()) and torch.equal(off0, C.offsets.cpu()) and torch.equal(cnt0, C.cnts.cpu())


# ------------------------------------------------------------------------------------------------ 4. GPU prefill
def _build_cache(case, landmark_dtype, **kw):
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    c, inp = G.CASES[case], G.make_inputs(case)
    cache = ShadowKVCache_CPU(G.config_of(case), batch_size=1, max_length=c["L"], device=DEV, dtype=torch.bfloat16,
                              sparse_budget=c["budget"], chunk_size=c["chunk"], rank=c["rank"], landmark_dtype=landmark_dtype, **kw)
    cache.get_svd(inp["k_pre"].to(DEV), 0)
    k_roped = G.rope_torch(case, inp["k_pre"], inp["cos_sin"], torch.arange(c["L"]).unsqueeze(0))
    cache.prefill_kv_cache(inp["v"].to(DEV), 0, k_roped.to(DEV), inp["q_last"].to(DEV))
    cache.H2D()
    torch.cuda.synchronize()
    return cache, inp


@pytest.mark.parametrize("batched", [False, True], ids=["bs1", "bs2x2"])
def test_gpu_prefill_fills_the_table_like_the_reference(batched):
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    if not batched:
        a, inp = _build_cache("llama_small", "fp8_e4m3")
        b, _ = _build_cache("llama_small", "bf16")
        check_fp8_landmark_cache_against_reference_and_twin(a, b, [inp["q_last"]])
        return
    case = "subbatch_llama"                                    # four sequences, prefilled two at a time
    c, inputs = G.SUBBATCH_CASES[case], G.subbatch_inputs(case)
    caches = []
    for dt in ("fp8_e4m3", "bf16"):
        cache = ShadowKVCache_CPU(G.config_of(case), batch_size=c["batch"], max_length=c["L"], device=DEV, dtype=torch.bfloat16,
                                  sparse_budget=c["budget"], chunk_size=c["chunk"], rank=c["rank"], landmark_dtype=dt)
        for i in range(0, c["batch"], c["sub"]):
            idx = list(range(i, i + c["sub"]))
            for l, inp in enumerate(inputs):
                cache.get_svd(inp["k_pre"][idx].to(DEV), l)
                cache.prefill_kv_cache(inp["v"][idx].to(DEV), l, inp["k_roped"][idx].to(DEV), inp["q_last"][idx].to(DEV))
        caches.append(cache)
    torch.cuda.synchronize()
    check_fp8_landmark_cache_against_reference_and_twin(caches[0], caches[1], [inp["q_last"] for inp in inputs], sub=c["sub"])


# ------------------------------------------------------------------------------------------------ 5. the model
PROMPT = 4700


@torch.inference_mode()         # (a model's prefill leaves inference tensors)
def make_twin(a, b):
    """b (bf16-landmark cache, same inputs as the FP8-landmark cache a) <- dequant(a's table) as its landmarks, and a's initial
    resident set (ids and the K / V rows they stand for: every other row of the two buffers is equal already)."""
    assert a.k_landmark.dtype == torch.float8_e4m3fn and b.k_landmark.dtype == torch.bfloat16
    assert torch.equal(a.k_landmark_idx, b.k_landmark_idx)
    s0 = a.sparse_start
    for n in ("k_cache_buffer", "v_cache_buffer"):
        xa, xb = getattr(a, n), getattr(b, n)
        assert torch.equal(_i16(xa[:, :, :, :s0]), _i16(xb[:, :, :, :s0])) and torch.equal(_i16(xa[:, :, :, a.sparse_end:]), _i16(xb[:, :, :, a.sparse_end:]))
        xb.copy_(xa)
    deq = R.dequantize_rows(a.k_landmark.cpu().view(torch.uint8), a.k_landmark_scale.cpu())[0]
    b.k_landmark.copy_(deq)
    b.position_ids.copy_(a.position_ids)
    a.H2D(); b.H2D()
    torch.cuda.synchronize()


def _model(glm, batch, landmark_dtype, v_dtype="bf16"):
    from shadowkv_amd import llama
    cfg = llama.ModelConfig(name="tiny", hidden_size=1024, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=8,
                            num_key_value_heads=2, vocab_size=2000, qkv_bias=glm, rope_style="glm" if glm else "neox")
    return llama.DecoderLM(cfg=cfg, batch_size=batch, max_length=5120, device=DEV, sparse_budget=256, rank=160, chunk_size=8,
                           seed=5, max_new_tokens=64, v_dtype=v_dtype, landmark_dtype=landmark_dtype)


def _tap(m):
    """keeps the bf16 logits of the model's last forward_fused / inference call (a captured graph's static output included)"""
    box = {}
    for name in ("forward_fused", "inference"):
        def wrap(orig):
            def f(*args, **kw):
                box["logits"] = orig(*args, **kw)
                return box["logits"]
            return f
        setattr(m, name, wrap(getattr(m, name)))
    return box


def _same_state(a, b, what):
    ca, cb = a.kv_cache, b.kv_cache
    assert torch.equal(ca.position_ids, cb.position_ids), what
    assert torch.equal(ca._cnts_layers, cb._cnts_layers), f"{what}: hit counts"
    assert torch.equal(_i16(ca.k_cache_buffer), _i16(cb.k_cache_buffer)), f"{what}: K buffer"
    assert torch.equal(_i16(ca.v_cache_buffer), _i16(cb.v_cache_buffer)), f"{what}: V buffer"


def _decode_all_paths(a, b, tok, steps=6):
    from shadowkv_amd import llama
    ba, bb = _tap(a), _tap(b)
    ta, tb = tok.clone(), tok.clone()
    for fused in (True, False):
        for i in range(steps):
            ta, tb = a.decode_step(ta, temperature=0.0, fused=fused), b.decode_step(tb, temperature=0.0, fused=fused)
            torch.cuda.synchronize()
            what = f"fused={fused} step {i}"
            assert ba["logits"].dtype == torch.bfloat16 and torch.equal(_i16(ba["logits"]), _i16(bb["logits"])), what
            assert torch.equal(ta, tb), what
            _same_state(a, b, what)
    da, db = llama.GraphDecoder(a, temperature=0.0), llama.GraphDecoder(b, temperature=0.0)
    da.token.copy_(ta); db.token.copy_(tb)
    assert da.capture(warmup=2) == 2 and db.capture(warmup=2) == 2
    for i in range(steps):
        ta, tb = da.step().clone(), db.step().clone()
        torch.cuda.synchronize()
        assert torch.equal(ta, tb) and torch.equal(_i16(ba["logits"]), _i16(bb["logits"])), f"graph step {i}"
    _same_state(a, b, "after the graph steps")


@pytest.mark.parametrize("glm,batch,v_dtype", [(False, 1, "bf16"), (False, 2, "bf16"), (True, 1, "bf16"), (True, 2, "bf16"),
                                               (False, 2, "fp8_e4m3")])
def test_model_decodes_bit_equal_to_its_bf16_twin(glm, batch, v_dtype):
    """6 greedy steps each through decode_step(fused=True), decode_step(fused=False) and a captured GraphDecoder from the same
    prompt: tokens, bf16 logits, hit counts and cache buffers of the FP8-landmark model and its twin stay bit-equal."""
    a, b = _model(glm, batch, "fp8_e4m3", v_dtype), _model(glm, batch, "bf16", v_dtype)
    ids = torch.randint(0, 2000, (batch, PROMPT), generator=torch.Generator().manual_seed(3)).to(DEV)
    prefill = "prefill" if batch == 1 else "batch_prefill"
    la, lb = getattr(a, prefill)(ids), getattr(b, prefill)(ids)
    torch.cuda.synchronize()
    assert torch.equal(la, lb)                                 # the prompt's own attention reads no landmark
    assert a.kv_cache.k_landmark.element_size() * 2 == b.kv_cache.k_landmark.element_size()
    make_twin(a.kv_cache, b.kv_cache)
    _decode_all_paths(a, b, la[:, -1].argmax(dim=-1, keepdim=True))
    assert a.kv_cache.get_kv_len() == b.kv_cache.get_kv_len() == PROMPT + 12 + 2 + 6


def test_generate_graph_equals_eager_with_fp8_landmarks():
    ids = torch.randint(0, 2000, (1, PROMPT), generator=torch.Generator().manual_seed(12)).to(DEV)
    m1, m2 = _model(False, 1, "fp8_e4m3"), _model(False, 1, "fp8_e4m3")
    g1 = m1.generate(ids, 6, temperature=0.0)
    g2 = m2.generate(ids, 6, temperature=0.0, graph=True)
    torch.cuda.synchronize()
    assert torch.equal(g1, g2), (g1, g2)
    _same_state(m1, m2, "generate")


@functools.lru_cache(maxsize=None)
def _headline_pair():
    """Two layers of Llama-3.1-8B shapes (the k/v projection role is built for K = 4096) over a 4,104-token synthetic context, in
    the in-place layout with the attention inside the fetch launch: the FP8-landmark model and its twin."""
    from shadowkv_amd import llama
    out = []
    for dt in ("fp8_e4m3", "bf16"):
        m = llama.DecoderLM(cfg=llama.LLAMA_3_1_8B, batch_size=1, max_length=4104, device=DEV, sparse_budget=256, rank=160,
                            chunk_size=8, num_layers=2, seed=1234, chunk_layout="inplace", overlap_attention=True, landmark_dtype=dt)
        llama.build_synthetic_context(m, 4104, seed=4321)
        out.append(m)
    make_twin(out[0].kv_cache, out[1].kv_cache)
    return out[0], out[1], llama


def test_bs1_with_early_fetch_near_staging_and_the_split_qkv_launch():
    """The captured bs-1 headline path: early fetch + near-miss staging + the k/v projection as a role of a selection launch.
    Eager steps, then a captured graph, along a query walk (so that the early fetch has something to predict)."""
    a, b, llama = _headline_pair()
    for m in (a, b):
        assert m.kv_cache.early_fetch_supported() and m.kv_cache.kv_proj_role_supported() and m.split_kv_proj
        m.kv_cache.enable_early_fetch(early_max=8, near=True)
    steps = 8
    table = llama.make_walk_table(a, steps, seed=3)
    ba, bb = _tap(a), _tap(b)
    ta = tb = torch.tensor([[17]], device=DEV)
    for i in range(3):
        ta, tb = a.decode_step(ta, temperature=0.0, q_table=table[i]), b.decode_step(tb, temperature=0.0, q_table=table[i])
        torch.cuda.synchronize()
        assert torch.equal(ta, tb) and torch.equal(_i16(ba["logits"]), _i16(bb["logits"])), f"eager step {i}"
        _same_state(a, b, f"eager step {i}")
    assert a.kv_proj_split_launches == 3 * a.num_layers and a.kv_proj_fused_launches == 0
    da, db = llama.GraphDecoder(a, temperature=0.0, walk_table=table[3:]), llama.GraphDecoder(b, temperature=0.0, walk_table=table[3:])
    da.token.copy_(ta); db.token.copy_(tb)
    wa, wb = da.capture(warmup=1), db.capture(warmup=1)
    assert wa == wb
    pulled = 0
    for i in range(steps - 3 - wa):
        ta, tb = da.step().clone(), db.step().clone()
        torch.cuda.synchronize()
        assert torch.equal(ta, tb) and torch.equal(_i16(ba["logits"]), _i16(bb["logits"])), f"graph step {i}"
        _same_state(a, b, f"graph step {i}")
        for l in range(a.num_layers):
            ea, eb = a.kv_cache.early_fetch_counts(l), b.kv_cache.early_fetch_counts(l)
            assert torch.equal(ea, eb), f"graph step {i}: early-fetch counts of layer {l}"
            pulled += int(ea.sum())
    assert pulled > 0, "nothing was pulled early"
    assert a.kv_proj_split_launches > 3 * a.num_layers and a.kv_proj_fused_launches == 0 and a.kv_cache.near_fetch


# ------------------------------------------------------------------------------------------------ 6. refusals on the device
def test_refusals_leave_every_buffer_unchanged():
    a, inp = _build_cache("llama_small", "fp8_e4m3")
    q, cs = inp["q_steps"][0].to(DEV), inp["cos_sin"].to(DEV)
    names = ("position_ids", "offsets", "_cnts_layers", "k_cache_buffer", "v_cache_buffer", "k_landmark_scale", "k_landmark_idx",
             "_slot_age", "_sel_state", "_select_ws")
    before = {n: getattr(a, n).clone() for n in names}
    table = a.k_landmark.view(torch.uint8).clone()
    a.reference_calls = True
    with pytest.raises(RuntimeError, match="landmark_dtype"):
        a.get_retrieval_position_ids(0, q)
    with pytest.raises(RuntimeError, match="landmark_dtype"):
        a.get_value_cache(0, a.position_ids[0])
    with pytest.raises(RuntimeError, match="landmark_dtype"):
        a.get_key_cache(0, a.position_ids[0], None, cs)
    a.reference_calls = False
    # the early fetch of an FP8-landmark cache rides in the fused selection only: without it the state is refused, then the launch
    assert a.early_fetch_supported()
    a.fused_select = False
    assert not a.early_fetch_supported()
    with pytest.raises(RuntimeError, match="early fetch"):
        a.enable_early_fetch(early_max=8)
    a.fused_select = True
    a.enable_early_fetch(early_max=8)
    a.fused_select = False
    with pytest.raises(RuntimeError, match="landmark_dtype"):
        a.select_fetch_inplace(0, q, cs)
    a.fused_select = True
    L = _lib().lib()
    assert L.skv_score_landmarks_fp8(q.data_ptr(), a.k_landmark[0].data_ptr(), 0, a._select_ws.data_ptr(), a._select_ws.data_ptr(),
                                     a._select_ws.data_ptr(), a.block_num, 4, a.k_landmark.shape[-2], ALPHA, _stream()) == -1
    torch.cuda.synchronize()
    for n in names:
        assert torch.equal(getattr(a, n), before[n]), n
    assert torch.equal(a.k_landmark.view(torch.uint8), table)
