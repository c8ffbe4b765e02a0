"""GPU: the FP8 (e4m3) V offload table.

The quantise kernel is pinned byte for byte to the reference quantiser (tests/fp8_v_ref.py).  Everything behind it is pinned
through a TWIN: cache A keeps its V table in FP8; cache B is a bf16 cache built from the same inputs whose table is overwritten
with dequant(A's table) and whose sparse-region V rows hold the dequantised rows of B.position_ids.  Selection reads no V, so A
and B must stay identical, step after step and on every path that moves V."""
import functools

import pytest
import torch

import fp8_v_ref as R
import gen_inputs as G
from test_fp8_v_cpu import check_fp8_cache_against_reference_and_twin, check_sparse_rows_are_dequantised_table_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _i16(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ 1. the quantise kernel
@functools.lru_cache(maxsize=None)
def _quant_rows():
    g = torch.Generator().manual_seed(11)
    rows = torch.cat((R.pattern_rows(), R.sweep_rows(), torch.randn(62, 128, generator=g).to(torch.bfloat16)))
    return rows, R.quantize_rows(rows)


@pytest.mark.parametrize("strided", [False, True])
def test_quantise_kernel_equals_the_reference(strided):
    from shadowkv_amd import tensor_op
    rows, (want_b, want_s) = _quant_rows()
    n_rows, D, kv = rows.shape[0], 128, 8
    assert n_rows % 16 != 0                                    # the last workgroup is a partial one
    if strided:      # the [1, kv, n, 128] transpose view of a fused [1, n, (32 + 2 kv) * 128] QKV output (test_gpu_kv_cache.py:46-48)
        n = -(-n_rows // kv)
        idx = torch.arange(kv * n) % n_rows                    # head h, token t <- row (h * n + t) % n_rows
        fused = torch.randn(1, n, (32 + 2 * kv) * D).to(torch.bfloat16)
        fused[0, :, (32 + kv) * D:] = rows[idx].view(kv, n, D).transpose(0, 1).reshape(n, kv * D)
        fused = fused.to(DEV)
        v = fused[..., (32 + kv) * D:].view(1, n, kv, D).transpose(1, 2)
        assert not v.is_contiguous() and torch.equal(v.cpu().reshape(-1, D).view(torch.int16), rows[idx].view(torch.int16))
    else:
        n, idx = n_rows, torch.arange(n_rows)
        v = rows.to(DEV).view(1, 1, n, D)
    heads = v.shape[1]
    # one spare token row per block behind the rows: the kernel must not write there
    table = torch.full((1, heads, (n + 1) * D), 0xAB, dtype=torch.uint8, device=DEV)
    scale = torch.full((1, heads, n + 1), -7.0, dtype=torch.float32, device=DEV)
    tensor_op.quantize_v_rows(v, table, scale)
    torch.cuda.synchronize()
    got_b, got_s = table.cpu()[:, :, :n * D].reshape(-1, D), scale.cpu()[:, :, :n].reshape(-1)
    bad = (got_b != want_b[idx]).any(dim=-1).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} rows differ, first: row {int(idx[bad[0]])}: {got_b[bad[0]].tolist()} != {want_b[idx[bad[0]]].tolist()}"
    assert torch.equal(got_b, want_b[idx]) and torch.equal(got_s, want_s[idx])
    assert bool((table.cpu()[:, :, n * D:] == 0xAB).all()) and bool((scale.cpu()[:, :, n:] == -7.0).all())


# ------------------------------------------------------------------------------------------------ 2. / 3. landing
CASES = {
    # name: (generator case, extra max_length, v_offload)
    "llama_small": ("llama_small", 0, True),
    "glm_small": ("glm_small", 0, True),
    "llama_cpu_b1024": ("llama_cpu_b1024", 0, True),
    "llama_small_long_table": ("llama_small", 512, True),      # host stride != the prompt's chunk count
    "trace_llama_bs2": ("trace_llama_bs2", 0, True),           # two sequences, 16 (batch, head) blocks, two layers
    "llama_small_hbm_table": ("llama_small", 0, False),        # v_offload=False
}
PATHS = ("get_value_cache", "lazy_value_fetch", "fetch_kv", "select_fetch_inplace", "select_fetch_inplace_resident2x")


@functools.lru_cache(maxsize=None)
def _inputs(gcase):
    """Per layer: dict(k_pre [bs, ...], k_roped, v, q_last, q_steps [steps, bs, Hq, 1, D]) on the CPU + cos_sin."""
    c = G.case_of(gcase)
    bs, layers = c.get("batch", 1), c["layers"]
    pos = torch.arange(c["L"]).unsqueeze(0)
    out = []
    for l in range(layers):
        per = [G.make_inputs(gcase, layer=8 * l + b) for b in range(bs)]
        out.append(dict(k_pre=torch.cat([p["k_pre"] for p in per]),
                        k_roped=torch.cat([G.rope_torch(gcase, p["k_pre"], p["cos_sin"], pos) for p in per]),
                        v=torch.cat([p["v"] for p in per]), q_last=torch.cat([p["q_last"] for p in per]),
                        q_steps=torch.cat([p["q_steps"] for p in per], dim=1), cos_sin=per[0]["cos_sin"]))
    return out


def _build(case, v_dtype, resident_sets=None):
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    gcase, extra, offload = CASES[case]
    c, inputs = G.case_of(gcase), _inputs(gcase)
    cache = ShadowKVCache_CPU(G.config_of(gcase), batch_size=c.get("batch", 1), max_length=c["L"] + extra, device=DEV,
                              dtype=torch.bfloat16, sparse_budget=c["budget"], chunk_size=c["chunk"], rank=c["rank"],
                              v_offload=offload, resident_sets=resident_sets, v_dtype=v_dtype)
    for l, inp in enumerate(inputs):
        cache.get_svd(inp["k_pre"].to(DEV), l)
        cache.prefill_kv_cache(inp["v"].to(DEV), l, inp["k_roped"].to(DEV), inp["q_last"].to(DEV))
    cache.H2D()
    torch.cuda.synchronize()
    return cache, c, inputs


def make_twin(a, b):
    """b (bf16 cache, same inputs as the FP8-V cache a) <- dequant(a's table) in its table, the dequantised rows of its own
    position_ids in its sparse region; by the reference dequantiser, on the CPU."""
    C, D = a.chunk_size, a.head_dim
    assert torch.equal(a.position_ids, b.position_ids)
    table = a.v_cache_cpu.cpu().view(torch.uint8)
    L, bs, kv, n, _ = table.shape
    scale = a.v_scale.cpu()
    deq = R.dequantize_rows(table.view(L, bs, kv, n, C, D), scale)[0].view(L, bs, kv, n, C * D)
    b.v_cache_cpu.copy_(deq)
    pos = b.position_ids.cpu().clamp_min(0)                                         # [L, bs, kv, R]; empty slots: any row
    rows = deq.gather(3, pos.unsqueeze(-1).expand(-1, -1, -1, -1, C * D)).view(L, bs, kv, -1, D)
    live = (b.position_ids.cpu() >= 0).repeat_interleave(C, dim=-1).unsqueeze(-1)
    region = b.v_cache_buffer[:, :, :, b.sparse_start:b.sparse_start + rows.shape[3]]
    region.copy_(torch.where(live, rows, region.cpu()).to(DEV))
    torch.cuda.synchronize()


def _pair(case, path):
    rs = None
    if path == "select_fetch_inplace_resident2x":
        rs = 2 * (G.case_of(CASES[case][0])["budget"] // 8)
    a, c, inputs = _build(case, "fp8_e4m3", rs)
    b, _, _ = _build(case, "bf16", rs)
    assert a.v_cache_cpu.dtype == torch.float8_e4m3fn and a.v_cache_cpu.is_cuda == (not CASES[case][2])
    assert a.v_cache_cpu.element_size() * 2 == b.v_cache_cpu.element_size()
    if CASES[case][2]:
        assert a.v_cache_cpu.is_pinned()
    for cch in (a, b):
        cch.lazy_value_fetch = path == "lazy_value_fetch"
    make_twin(a, b)
    return a, b, c, inputs


def _step(cache, path, l, q, cs):
    """One decode step of layer l on `path`; returns the attention output."""
    from shadowkv_amd import tensor_op
    if path.startswith("select_fetch_inplace"):
        cache.select_fetch_inplace(l, q, cs)
        return tensor_op.sparse_attention_decode(q, cache.k_cache_buffer[l], cache.v_cache_buffer[l], kv_len=cache.sparse_end + 1,
                                                 **cache.attend_slot_args())
    ids = cache.get_retrieval_position_ids(layer_idx=l, query_states=q)
    if path == "fetch_kv":
        cache.fetch_kv(l, ids, cs)
        k_view, v_view = cache.k_cache_buffer[l][:, :, :cache.sparse_end + 1], cache.v_cache_buffer[l][:, :, :cache.sparse_end + 1]
    else:
        cur = torch.cuda.current_stream()
        with torch.cuda.stream(cache.copy_stream):
            cache.copy_stream.wait_stream(cur)
            v_view = cache.get_value_cache(l, ids)
        k_view = cache.get_key_cache(layer_idx=l, position_ids=ids, rope_func=None, cos_sin_cache=cs)
        cur.wait_stream(cache.copy_stream)
    return tensor_op.sparse_attention_decode(q, k_view, v_view)


def _edge_query(cache, l, gen):
    """A query that selects the FIRST and the LAST chunk a head can select (its lowest / highest landmark id): query head 0 of
    every group points along the first landmark, head 1 along the last one."""
    lm = cache.k_landmark[l].float()                                                # [bs, kv, N, D]
    bs, kv, _, D = lm.shape
    Gq = cache.num_key_value_groups
    q = torch.randn(bs, kv, Gq, D, generator=gen).to(DEV) * 0.1
    q[:, :, 0] = lm[:, :, 0] * 8
    q[:, :, 1] = lm[:, :, -1] * 8
    return q.view(bs, kv * Gq, 1, D).to(torch.bfloat16)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("path", PATHS)
def test_landing_is_exact_and_the_invariant_holds(path, case):
    """After every decode step A (FP8 table) and its twin B are equal in position_ids / offsets / cnts, the K and the V
    buffer and the attention output (test 2), and every slot of A's sparse region holds dequant(table[position_ids[slot]])
    (test 3).  The run holds a repeated query (cnts == S: nothing is fetched), a step with cnts < S / 2 for some head (the golden
    q_steps are joined by seeded queries that make sure of it), and the first and the last selectable chunk of the table
    arrive as misses at least once."""
    a, b, c, inputs = _pair(case, path)
    S, layers, B = a.select_sets, len(inputs), a.block_num
    cs = inputs[0]["cos_sin"].to(DEV)
    gen = torch.Generator().manual_seed(99)
    # "opposite": the prompt's last query negated, as the FIRST step - its selection is nearly disjoint from the resident set the
    # prefill left (with 128 of 240 landmarks selected, as in llama_cpu_b1024, a random query alone would hit about half)
    steps = [("opposite", 0)] + [("golden", t) for t in range(inputs[0]["q_steps"].shape[0])] + \
            [("repeat", 0), ("random", 0), ("edge", 0)]
    min_cnt, saw_all_hits = S, False
    fetched = [set() for _ in range(layers)]
    q_prev = [None] * layers
    for kind, t in steps:
        for l, inp in enumerate(inputs):
            if kind == "golden":
                q = inp["q_steps"][t].to(DEV)
            elif kind == "opposite":
                q = (-inp["q_last"]).to(DEV)
            elif kind == "repeat":
                q = q_prev[l]
            elif kind == "random":
                q = (torch.randn(inp["q_last"].shape, generator=gen) * 2).to(torch.bfloat16).to(DEV)
            else:
                q = _edge_query(a, l, gen)
            q_prev[l] = q
            oa, ob = _step(a, path, l, q, cs), _step(b, path, l, q, cs)
            torch.cuda.synchronize()
            what = f"{kind} {t}, layer {l}"
            assert torch.equal(a.position_ids, b.position_ids), what
            assert torch.equal(a.offsets, b.offsets) and torch.equal(a.cnts, b.cnts), what
            assert torch.equal(_i16(a.k_cache_buffer), _i16(b.k_cache_buffer)), f"{what}: K buffer"
            assert torch.equal(_i16(a.v_cache_buffer), _i16(b.v_cache_buffer)), f"{what}: V buffer"
            assert torch.equal(_i16(oa), _i16(ob)), f"{what}: attention output"
            check_sparse_rows_are_dequantised_table_rows(a, l)
            cnts = a.cnts.cpu().view(B)
            if kind == "repeat":
                assert bool((cnts == S).all()), f"{what}: the same query again must hit everywhere, cnts {cnts.tolist()}"
                saw_all_hits = True
            min_cnt = min(min_cnt, int(cnts.min()))
            miss = a.offsets.cpu().view(B, S)
            for bh in range(B):
                fetched[l].update(miss[bh, int(cnts[bh]):].tolist())
    assert saw_all_hits and min_cnt < S / 2, f"coverage: fewest hits of a head in any step {min_cnt} of {S}"
    for l in range(layers):
        first, last = int(a.k_landmark_idx[l][..., 0].min()), int(a.k_landmark_idx[l][..., -1].max())
        assert first == 0 and last == a.chunks - 1
        assert first in fetched[l] and last in fetched[l], f"layer {l}: chunks {first} / {last} were never fetched"


def test_gpu_prefill_fills_the_table_like_the_reference():
    """The native pass over the strided prompt V (sub-batch offset included) against the reference quantiser, and everything
    but the sparse-region V rows against the bf16 cache."""
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    case = "subbatch_llama"
    c, inputs = G.SUBBATCH_CASES[case], G.subbatch_inputs(case)
    kv, D, Hq = c["kv_heads"], c["head_dim"], c["q_heads"]
    caches = []
    for v_dtype in ("fp8_e4m3", "bf16"):
        cache = ShadowKVCache_CPU(G.config_of(case), batch_size=c["batch"], max_length=c["L"] + 64, device=DEV, dtype=torch.bfloat16,
                                  sparse_budget=c["budget"], chunk_size=c["chunk"], rank=c["rank"], v_dtype=v_dtype)
        for i in range(0, c["batch"], c["sub"]):
            idx = list(range(i, i + c["sub"]))
            for l, inp in enumerate(inputs):
                cache.get_svd(inp["k_pre"][idx].to(DEV), l)
                # V as the model hands it over: the transposed view of the fused QKV output
                fused = torch.zeros(len(idx), c["L"], (Hq + 2 * kv) * D, dtype=torch.bfloat16)
                fused[..., (Hq + kv) * D:] = inp["v"][idx].transpose(1, 2).reshape(len(idx), c["L"], kv * D)
                v = fused.to(DEV)[..., (Hq + kv) * D:].view(len(idx), c["L"], kv, D).transpose(1, 2)
                assert not v.is_contiguous()
                cache.prefill_kv_cache(v, l, inp["k_roped"][idx].to(DEV), inp["q_last"][idx].to(DEV))
        caches.append(cache)
    torch.cuda.synchronize()
    check_fp8_cache_against_reference_and_twin(caches[0], caches[1], [inp["v"] for inp in inputs])


# ------------------------------------------------------------------------------------------------ 4. the model
PROMPT = 4700


def _model(glm, batch, v_dtype, layout="reference", overlap=False):
    from shadowkv_amd import llama
    cfg = llama.ModelConfig(name="tiny", hidden_size=1024, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=8,
                            num_key_value_heads=2, vocab_size=2000, qkv_bias=glm, rope_style="glm" if glm else "neox")
    return llama.DecoderLM(cfg=cfg, batch_size=batch, max_length=5120, device=DEV, sparse_budget=256, rank=160, chunk_size=8,
                           seed=5, max_new_tokens=64, chunk_layout=layout, overlap_attention=overlap, v_dtype=v_dtype)


def _ids(batch, seed=3):
    return torch.randint(0, 2000, (batch, PROMPT), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _model_pair(glm, batch, layout="reference", overlap=False, prefill="prefill"):
    """(A with FP8 V, its bf16 twin B, first greedy token) after the prompt."""
    a, b = _model(glm, batch, "fp8_e4m3", layout, overlap), _model(glm, batch, "bf16", layout, False)
    ids = _ids(batch)
    la = getattr(a, prefill)(ids)
    lb = getattr(b, prefill)(ids)
    torch.cuda.synchronize()
    assert torch.equal(la, lb)                                 # the prompt's own attention reads the exact V in both
    make_twin(a.kv_cache, b.kv_cache)
    a.kv_cache.H2D(); b.kv_cache.H2D()
    return a, b, la[:, -1].argmax(dim=-1, keepdim=True)


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
    assert torch.equal(_i16(ca.k_cache_buffer), _i16(cb.k_cache_buffer)), f"{what}: K buffer"
    assert torch.equal(_i16(ca.v_cache_buffer), _i16(cb.v_cache_buffer)), f"{what}: V buffer"


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("glm", [False, True])
def test_model_decodes_bit_equal_to_its_bf16_twin(glm, batch):
    """6 greedy steps each through decode_step(fused=True), decode_step(fused=False) and a captured GraphDecoder, one after
    the other from the same prompt: tokens, bf16 logits and cache buffers of A and B stay bit-equal."""
    from shadowkv_amd import llama
    a, b, tok = _model_pair(glm, batch, prefill="prefill" if batch == 1 else "batch_prefill")
    ba, bb = _tap(a), _tap(b)
    ta, tb = tok.clone(), tok.clone()
    for fused in (True, False):
        for i in range(6):
            ta, tb = a.decode_step(ta, temperature=0.0, fused=fused), b.decode_step(tb, temperature=0.0, fused=fused)
            torch.cuda.synchronize()
            what = f"fused={fused} step {i}"
            assert ba["logits"].dtype == torch.bfloat16 and torch.equal(_i16(ba["logits"]), _i16(bb["logits"])), what
            assert torch.equal(ta, tb), what
            _same_state(a, b, what)
    da, db = llama.GraphDecoder(a, temperature=0.0), llama.GraphDecoder(b, temperature=0.0)
    da.token.copy_(ta); db.token.copy_(tb)
    assert da.capture(warmup=2) == 2 and db.capture(warmup=2) == 2
    for i in range(6):
        ta, tb = da.step().clone(), db.step().clone()
        torch.cuda.synchronize()
        assert torch.equal(ta, tb) and torch.equal(_i16(ba["logits"]), _i16(bb["logits"])), f"graph step {i}"
    _same_state(a, b, "after the graph steps")
    assert a.kv_cache.get_kv_len() == b.kv_cache.get_kv_len() == PROMPT + 12 + 2 + 6


@pytest.mark.parametrize("glm", [False, True])
def test_generate_graph_equals_eager_with_fp8_v(glm):
    ids = _ids(1, seed=12)
    m1, m2 = _model(glm, 1, "fp8_e4m3"), _model(glm, 1, "fp8_e4m3")
    g1 = m1.generate(ids, 6, temperature=0.0)
    g2 = m2.generate(ids, 6, temperature=0.0, graph=True)
    torch.cuda.synchronize()
    assert torch.equal(g1, g2), (g1, g2)
    _same_state(m1, m2, "generate")
    for l in range(m1.num_layers):
        check_sparse_rows_are_dequantised_table_rows(m1.kv_cache, l)
        check_sparse_rows_are_dequantised_table_rows(m2.kv_cache, l)


def test_inplace_overlap_request_takes_the_plain_launch():
    """chunk_layout='inplace', overlap_attention=True on an FP8-V model: can_overlap_attention() says no, the plain fetch
    launch + the standalone attention run, and the step matches the bf16 twin that takes the plain launch by request."""
    a, b, tok = _model_pair(False, 1, layout="inplace", overlap=True)
    assert a.overlap_attention and not a.kv_cache.can_overlap_attention() and b.kv_cache.can_overlap_attention()
    called = []
    orig = a.kv_cache.select_fetch_inplace
    a.kv_cache.select_fetch_inplace = lambda *args, **kw: (called.append(1), orig(*args, **kw))[1]
    ba, bb = _tap(a), _tap(b)
    ta, tb = tok.clone(), tok.clone()
    for i in range(6):
        ta, tb = a.decode_step(ta, temperature=0.0), b.decode_step(tb, temperature=0.0)
        torch.cuda.synchronize()
        assert torch.equal(ta, tb) and torch.equal(_i16(ba["logits"]), _i16(bb["logits"])), i
        _same_state(a, b, f"step {i}")
    assert len(called) == 6 * a.num_layers


# ------------------------------------------------------------------------------------------------ 5. refusals on the device
def test_refusals_leave_the_cache_untouched():
    a, c, inputs = _build("llama_small", "fp8_e4m3")
    q, cs = inputs[0]["q_steps"][0].to(DEV), inputs[0]["cos_sin"].to(DEV)
    names = ("position_ids", "offsets", "_cnts_layers", "k_cache_buffer", "v_cache_buffer", "v_scale")
    before = {n: getattr(a, n).clone() for n in names}
    table = a.v_cache_cpu.view(torch.uint8).clone()
    a.reference_calls = True
    with pytest.raises(RuntimeError, match="v_dtype"):
        a.get_retrieval_position_ids(0, q)
    with pytest.raises(RuntimeError, match="v_dtype"):
        a.get_value_cache(0, a.position_ids[0])
    with pytest.raises(RuntimeError, match="v_dtype"):
        a.get_key_cache(0, a.position_ids[0], None, cs)
    a.reference_calls = False
    assert not a.early_fetch_supported() and not a.can_overlap_attention()
    with pytest.raises(RuntimeError, match="v_dtype"):
        a.enable_early_fetch(early_max=16)
    with pytest.raises(RuntimeError, match="v_dtype"):
        a.enable_early_fetch()
    with pytest.raises(RuntimeError, match="v_dtype"):
        a.select_fetch_attend_inplace(0, q, cs, kv_len=a.sparse_end + 1)
    torch.cuda.synchronize()
    assert a._early is None
    for n in names:
        assert torch.equal(getattr(a, n), before[n]), n
    assert torch.equal(a.v_cache_cpu.view(torch.uint8), table)
