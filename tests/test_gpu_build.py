"""GPU: the prefill-side state builder kernel skv_chunk_stats (chunk means + per-chunk minimum cosine similarity,
/root/reference/models/kv_cache.py:854-868) through the C ABI against oracle_chunk_stats (bit-exact), and
ShadowKVCache_CPU.prefill_kv_cache built on the GPU (native pass) against the same cache built on the CPU with the
reference-pinned torch ops."""
import os

import numpy as np
import pytest
import torch

import gen_inputs as G
import oracle
from util import assert_bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _case(blocks, chunks, seed, extra_rows=0):
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(blocks, chunks * 8 + extra_rows, 128, generator=g)
    k *= torch.exp(torch.randn(blocks, chunks * 8 + extra_rows, 1, generator=g))       # row norms spread
    k = k.bfloat16()
    if chunks >= 3:
        k[0, 0:8] = 0                                   # an all-zero chunk (norm clamp)
        k[-1, 8:16] = k[-1, 8:9]                        # identical rows: cos == 1 up to rounding
        k[0, 16:24] *= 1e-3
    return k


@pytest.mark.parametrize("blocks,chunks,extra", [(1, 1, 0), (3, 5, 0), (8, 1021, 0), (2, 4100, 40), (16, 257, 8),
                                                 # the grid is capped at 4,096 workgroups x 4 chunks: past 16,384 chunks the
                                                 # grid-stride loop repeats (bench.py's 200 K / 244 K contexts: 25,600 / 31,232)
                                                 (2, 16389, 8)])
def test_chunk_stats_bit_exact_against_oracle(blocks, chunks, extra):
    from shadowkv_amd import tensor_op
    k = _case(blocks, chunks, 11 * blocks + chunks, extra)                            # [blocks, rows, 128]
    want_m, want_c = oracle.chunk_stats(k[:, :chunks * 8].contiguous())
    kd = k.to(DEV).view(1, blocks, -1, 128)
    got_m, got_c = tensor_op.chunk_stats(kd[:, :, :chunks * 8], 8)                     # a view: block stride > used rows
    assert_bits_equal(got_m.cpu().view(blocks, chunks, 128), want_m)
    assert_bits_equal(got_c.cpu().view(blocks, chunks), want_c)


def test_chunk_stats_full_size_properties():
    """Headline shape (8 kv heads x 15,608 chunks of a 124,928-token context): size-independent properties.
    Chunks of 8 identical rows: mean == the row bit for bit and the score is cos(x, x) ~ 1; permuting the rows of a
    chunk changes neither its mean nor its minimum (the 8-row sum is exact in f32 for same-scale bf16 rows)."""
    from shadowkv_amd import tensor_op
    g = torch.Generator(device=DEV).manual_seed(9)
    chunks = 15608
    k = torch.randn(1, 8, chunks * 8, 128, device=DEV, generator=g).bfloat16()
    k[:, :, : 8 * 100] = k[:, :, : 8 * 100].view(1, 8, 100, 8, 128)[:, :, :, :1].expand(-1, -1, -1, 8, -1).reshape(1, 8, 800, 128)
    m, c = tensor_op.chunk_stats(k, 8)
    assert torch.equal(m[:, :, :100].view(torch.int16), k[:, :, 0:800:8].view(torch.int16))
    assert (c[:, :, :100].float() - 1).abs().max() <= 2 ** -6
    perm = torch.tensor([3, 7, 0, 5, 1, 6, 2, 4], device=DEV)
    kp = k.view(1, 8, chunks, 8, 128)[:, :, :, perm].reshape(1, 8, chunks * 8, 128).contiguous()
    m2, c2 = tensor_op.chunk_stats(kp, 8)
    assert torch.equal(m.view(torch.int16), m2.view(torch.int16))
    assert torch.equal(c.view(torch.int16), c2.view(torch.int16))
    # against torch's own ops on the GPU on a slice (torch's f32 summation order differs: one-ulp flips allowed)
    ks = k[:, :, : 8 * 2048].view(1, 8, 2048, 8, 128)
    tm = ks.mean(dim=-2)
    tc = torch.nn.functional.cosine_similarity(tm.unsqueeze(3).expand(-1, -1, -1, 8, -1), ks, dim=-1).min(-1).values
    assert torch.equal(tm.view(torch.int16), m[:, :, :2048].view(torch.int16))
    d = (tc.float() - c[:, :, :2048].float()).abs()
    assert (d == 0).float().mean() > 0.995 and d.max() <= 2 ** -8


def test_chunk_stats_rejects_unsupported_shapes():
    from shadowkv_amd import _lib
    k = torch.zeros(1, 64, 128, device=DEV, dtype=torch.bfloat16)
    m = torch.zeros(1, 8, 128, device=DEV, dtype=torch.bfloat16)
    c = torch.zeros(1, 8, device=DEV, dtype=torch.bfloat16)
    L = _lib.lib()
    assert L.skv_chunk_stats(_lib.ptr(k), 64 * 128, 1, 4, 16, 128, _lib.ptr(m), _lib.ptr(c), 0) != 0
    assert L.skv_chunk_stats(_lib.ptr(k), 64 * 128, 1, 8, 8, 64, _lib.ptr(m), _lib.ptr(c), 0) != 0
    assert L.skv_chunk_stats(0, 64 * 128, 1, 8, 8, 128, _lib.ptr(m), _lib.ptr(c), 0) != 0
    assert L.skv_chunk_stats(_lib.ptr(k), 64 * 128, 1, 0, 8, 128, _lib.ptr(m), _lib.ptr(c), 0) == 0    # empty: no-op


@pytest.mark.parametrize("case", list(G.CASES))
def test_prefill_state_built_on_gpu_equals_cpu_build(case):
    """prefill_kv_cache with the native pass (GPU) against the torch-op host mirror (CPU), which the golden fixtures pin
    to the reference bit for bit: landmarks, landmark ids, initial selection, buffers."""
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    c, inp = G.CASES[case], G.make_inputs(case)
    k_roped = G.rope_torch(case, inp["k_pre"], inp["cos_sin"], torch.arange(c["L"]).unsqueeze(0))
    caches = {}
    for dev in ("cpu", DEV):
        cache = ShadowKVCache_CPU(G.config_of(case), batch_size=1, max_length=c["L"], device=dev, dtype=torch.bfloat16,
                                  sparse_budget=c["budget"], chunk_size=c["chunk"], rank=c["rank"])
        cache.U = torch.zeros(1, 1, c["L"], c["rank"], dtype=torch.bfloat16, device=dev)   # factorisation not under test
        cache.SV = torch.zeros(1, 1, c["kv_heads"], 128, c["rank"], dtype=torch.bfloat16, device=dev)
        cache.prefill_kv_cache(inp["v"].to(dev), 0, k_roped.to(dev), inp["q_last"].to(dev))
        caches[dev] = cache
    if DEV.startswith("cuda"):
        torch.cuda.synchronize()
    a, b = caches["cpu"], caches[DEV]
    kv, C, D = c["kv_heads"], c["chunk"], 128
    # outlier pick = topk(smallest) of the scores: identical unless the boundary value is tied (torch.topk's tie
    # order is unspecified and differs between its CPU and GPU kernels)
    _, mc = oracle.chunk_stats(k_roped[0, :, : a.chunks * C].contiguous())
    for h in range(kv):
        srt = mc[h].float().sort().values
        tied = a.outlier_chunk > 0 and srt[a.outlier_chunk - 1] == srt[a.outlier_chunk]
        if not tied:
            assert torch.equal(a.k_landmark_idx[0][0, h], b.k_landmark_idx[0][0, h].cpu()), h
            assert_bits_equal(b.k_landmark[0][0, h].cpu(), a.k_landmark[0][0, h])
    # local rows and outlier region: exact copies of the source rows, whichever chunks were picked
    pl, ss, se = b.prefill_local, b.sparse_start, b.sparse_end
    assert (pl, ss, se) == (a.prefill_local, a.sparse_start, a.sparse_end)
    assert_bits_equal(b.k_cache_buffer[0][:, :, :pl].cpu(), a.k_cache_buffer[0][:, :, :pl])
    assert_bits_equal(b.v_cache_buffer[0][:, :, :pl].cpu(), a.v_cache_buffer[0][:, :, :pl])
    # sparse region: slot i holds chunk position_ids[i] (the invariant decode relies on), K and V
    for h in range(kv):
        ids = b.position_ids[0][0, h].cpu()
        assert ids.min() >= 0 and ids.max() < b.chunks and ids.unique().numel() == ids.numel()
        want_v = inp["v"][0, h].view(-1, C, D)[ids].reshape(-1, D)
        want_k = k_roped[0, h].view(-1, C, D)[ids].reshape(-1, D)
        assert_bits_equal(b.v_cache_buffer[0][0, h, ss:se].cpu(), want_v)
        assert_bits_equal(b.k_cache_buffer[0][0, h, ss:se].cpu(), want_k)


def _recon(U, SV):
    return torch.einsum("blr,bhdr->bhld", U.float(), SV.float())


@pytest.mark.parametrize("case", ["llama_small", "glm_small"])
def test_gram_factorisation_on_gpu_against_reference_pinned_factors(case):
    """svd_mode='gram' on the GPU (K^T K -> eigh -> K V_r / s_r: SURVEY.md section 8f rank 2, replaces torch.svd at
    /root/reference/models/kv_cache.py:700-733).  Column signs / algorithm differ from an SVD, so what decode consumes is
    compared: the rank-160 reconstruction U.SV from the stored bf16 factors against the reconstruction from the factors the
    REFERENCE produced (fixture svd_U / svd_SV, made by tests/golden/make_golden.py), rtol 1e-2 of the RMS key value."""
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{case}.npz"))
    c, inp = G.CASES[case], G.make_inputs(case)
    cache = ShadowKVCache_CPU(G.config_of(case), batch_size=1, max_length=c["L"], device=DEV, dtype=torch.bfloat16,
                              sparse_budget=c["budget"], chunk_size=c["chunk"], rank=c["rank"], svd_mode="gram")
    cache.get_svd(inp["k_pre"].to(DEV), 0)
    torch.cuda.synchronize()
    bf = lambda a: torch.from_numpy(a.astype(np.int16)).view(torch.bfloat16)
    ref = torch.einsum("blr,bhrd->bhld", bf(z["svd_U"]).float(), bf(z["svd_SV"]).float())     # fixture SV is [1, kv, r, D]
    got = _recon(cache.U[0], cache.SV[0]).cpu()
    k = inp["k_pre"].float()
    scale = k.pow(2).mean().sqrt()
    assert float((got - ref).pow(2).mean().sqrt() / scale) < 1e-2
    assert float((got - k).pow(2).mean().sqrt()) <= float((ref - k).pow(2).mean().sqrt()) * 1.02 + 1e-3 * float(scale)


def test_gram_factorisation_at_headline_length_and_rank_deficient_keys():
    """One layer at the headline length (L = 124,928 tokens, 8 KV heads x 128): Gram factorisation against torch.svd on
    the same keys - the reconstructions agree to 1e-2 of the RMS key value and approximate K equally well; keys of rank
    100 < 160 (48+ singular values at rounding-noise level) must give finite factors and the same reconstruction."""
    from shadowkv_amd.kv_cache import gram_factorize
    g = torch.Generator(device=DEV).manual_seed(3)
    L, H, r = 122 * 1024, 1024, 160
    a = torch.randn(1, L, r, device=DEV, generator=g)
    b = torch.randn(1, r, H, device=DEV, generator=g) * (torch.arange(r, device=DEV).float().mul(-0.02).exp().view(1, r, 1))
    k = (a @ b + 0.02 * torch.randn(1, L, H, device=DEV, generator=g)).bfloat16().float()
    u_g, sv_g = gram_factorize(k, r)
    u, s, v = torch.svd(k)
    rec_svd = (u[:, :, :r].bfloat16().float() * 1) @ (torch.diag_embed(s[:, :r]) @ v.transpose(1, 2)[:, :r]).bfloat16().float()
    rec_gram = u_g.bfloat16().float() @ sv_g.bfloat16().float()
    scale = k.pow(2).mean().sqrt()
    assert float((rec_gram - rec_svd).pow(2).mean().sqrt() / scale) < 1e-2
    e_s, e_g = (rec_svd - k).pow(2).mean().sqrt(), (rec_gram - k).pow(2).mean().sqrt()
    assert float(e_g) <= float(e_s) * 1.02 + 1e-3 * float(scale)
    del u, s, v, rec_svd, rec_gram
    k2 = (a[:, :20000, :100] @ b[:, :100]).bfloat16().float()          # rank 100 (+ bf16 rounding noise)
    u2, sv2 = gram_factorize(k2, r)
    assert bool(torch.isfinite(u2).all()) and bool(torch.isfinite(sv2).all())
    assert float(u2.abs().max()) < 1e3                                   # no noise / ~0 columns
    rec2 = u2.bfloat16().float() @ sv2.bfloat16().float()
    assert float((rec2 - k2).pow(2).mean().sqrt() / k2.pow(2).mean().sqrt()) < 2e-2
    k3 = torch.zeros(1, 4096, H, device=DEV)                             # all-zero keys: zero factors, not NaN
    u3, sv3 = gram_factorize(k3, r)
    assert float(u3.abs().max()) == 0.0 and float(sv3.abs().max()) == 0.0


def test_default_factorisation_on_a_gpu_is_the_gram_path():
    """Round 4: get_svd's default (svd_mode='auto') takes the Gram factorisation for keys on a GPU and torch.svd on the CPU;
    'svd' stays selectable.  The default's factors are the Gram path's bit for bit, and its rank-160 reconstruction meets
    SURVEY.md 8c's criterion (rtol 1e-2 of the RMS key value) against the reference's own call on the same keys
    (/root/reference/models/kv_cache.py:700-733)."""
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    case = "llama_small"
    c, inp = G.CASES[case], G.make_inputs(case)
    caches = {}
    for mode in ("auto", "gram", "svd"):
        cache = ShadowKVCache_CPU(G.config_of(case), batch_size=1, max_length=c["L"], device=DEV, dtype=torch.bfloat16,
                                  sparse_budget=c["budget"], chunk_size=c["chunk"], rank=c["rank"], svd_mode=mode)
        cache.get_svd(inp["k_pre"].to(DEV), 0)
        caches[mode] = cache
    torch.cuda.synchronize()
    assert ShadowKVCache_CPU(G.config_of(case), batch_size=1, max_length=c["L"], device=DEV).svd_mode == "auto"
    assert_bits_equal(caches["auto"].U.cpu(), caches["gram"].U.cpu())
    assert_bits_equal(caches["auto"].SV.cpu(), caches["gram"].SV.cpu())
    k = inp["k_pre"].float()
    scale = k.pow(2).mean().sqrt()
    rec_d, rec_s = _recon(caches["auto"].U[0], caches["auto"].SV[0]).cpu(), _recon(caches["svd"].U[0], caches["svd"].SV[0]).cpu()
    assert float((rec_d - rec_s).pow(2).mean().sqrt() / scale) < 1e-2
    # the CPU default is still the reference's torch.svd (the fixtures pin it bit for bit: tests/test_kv_cache_cpu.py)
    cpu = ShadowKVCache_CPU(G.config_of(case), batch_size=1, max_length=c["L"], device="cpu", sparse_budget=c["budget"],
                            chunk_size=c["chunk"], rank=c["rank"])
    ref = ShadowKVCache_CPU(G.config_of(case), batch_size=1, max_length=c["L"], device="cpu", sparse_budget=c["budget"],
                            chunk_size=c["chunk"], rank=c["rank"], svd_mode="svd")
    cpu.get_svd(inp["k_pre"], 0); ref.get_svd(inp["k_pre"], 0)
    assert_bits_equal(cpu.U, ref.U)
    assert_bits_equal(cpu.SV, ref.SV)


# ---------------------------------------------------------------------------------------------------------------------
# Sub-batched prefill on the device (VERDICT r4 missing #4 / SURVEY 8f3): LLM.batch_prefill's pattern
# (/root/reference/models/base.py:533-543; kv_cache.py:683-737, 788-980) - the CPU counterpart
# (tests/test_kv_cache_cpu.py::test_subbatched_prefill_equals_the_reference_and_the_one_shot_build) pins it to the reference.
# ---------------------------------------------------------------------------------------------------------------------
def _device_prefill(case, sub, only=None, factor_on="cpu"):
    from shadowkv_amd.kv_cache import ShadowKVCache_CPU
    c = G.SUBBATCH_CASES[case]
    inputs = G.subbatch_inputs(case)
    seqs = list(range(c["batch"])) if only is None else [only]
    cache = ShadowKVCache_CPU(G.config_of(case), batch_size=len(seqs), max_length=c["L"], device=DEV, dtype=torch.bfloat16,
                              sparse_budget=c["budget"], chunk_size=c["chunk"], rank=c["rank"])
    for i in range(0, len(seqs), sub):
        idx = seqs[i:i + sub]
        for l, inp in enumerate(inputs):
            # factor_on="cpu": torch.svd through LAPACK, one matrix at a time whatever the batch - the factors do not depend on
            # how the batch was cut (a batched rocSOLVER / hipBLASLt call may pick another algorithm per batch count)
            k_pre = inp["k_pre"][idx]
            cache.get_svd(k_pre if factor_on == "cpu" else k_pre.to(DEV), l)
            cache.prefill_kv_cache(inp["v"][idx].to(DEV), l, inp["k_roped"][idx].to(DEV), inp["q_last"][idx].to(DEV))
        assert cache.prefilled_batch == min(i + sub, len(seqs))
        assert cache.kv_offset == (c["L"] if cache.prefilled_batch == len(seqs) else 0)
    cache.H2D()
    torch.cuda.synchronize()
    return cache, inputs


def _decode3(case, cache, inputs, seqs):
    """3 decode steps x layers in the reference's method order; returns the per-step observable state."""
    c = G.SUBBATCH_CASES[case]
    cs = inputs[0]["cos_sin"].to(DEV)
    out = []
    q_prev = [inp["q_last"][seqs] for inp in inputs]
    for t in range(3):
        for l in range(c["layers"]):
            g = torch.Generator().manual_seed(1000 * t + l)
            noise = torch.randn(c["batch"], c["q_heads"], 1, c["head_dim"], generator=g)[seqs]
            q = (q_prev[l].float() + 0.5 * noise).bfloat16()
            q_prev[l] = q
            kn = torch.randn(c["batch"], c["kv_heads"], 1, c["head_dim"], generator=g)[seqs].bfloat16()
            vn = torch.randn(c["batch"], c["kv_heads"], 1, c["head_dim"], generator=g)[seqs].bfloat16()
            cache.update_kv_cache(kn.to(DEV), vn.to(DEV), l)
            pos = cache.get_retrieval_position_ids(layer_idx=l, query_states=q.to(DEV))
            cur = torch.cuda.current_stream()
            with torch.cuda.stream(cache.copy_stream):
                cache.copy_stream.wait_stream(cur)
                v = cache.get_value_cache(l, pos)
            k = cache.get_key_cache(layer_idx=l, position_ids=pos, rope_func=None, cos_sin_cache=cs)
            cur.wait_stream(cache.copy_stream)
            torch.cuda.synchronize()
            out.append(dict(pos=pos.cpu().clone(), cnts=cache.cnts.cpu().clone().view(len(seqs), -1), k=k.cpu().clone(),
                            v=v.cpu().clone()))
    return out


def test_subbatched_prefill_on_the_device_then_decode():
    case = "subbatch_llama"
    c = G.SUBBATCH_CASES[case]
    B = c["batch"]
    sub, inputs = _device_prefill(case, c["sub"])
    one, _ = _device_prefill(case, B)
    names = ("U", "SV", "k_landmark", "k_landmark_idx", "position_ids", "k_cache_buffer", "v_cache_buffer", "v_cache_cpu")
    for n in names:
        a, b = getattr(sub, n).cpu(), getattr(one, n).cpu()
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                           b.view(torch.int16) if b.dtype == torch.bfloat16 else b), f"sub-batched vs one-shot: {n}"
    d_sub = _decode3(case, sub, inputs, list(range(B)))
    d_one = _decode3(case, one, inputs, list(range(B)))
    for i, (x, y) in enumerate(zip(d_sub, d_one)):
        assert torch.equal(x["pos"], y["pos"]) and torch.equal(x["cnts"], y["cnts"]), f"call {i}: ids / counts"
        assert_bits_equal(x["v"], y["v"], f"call {i}: V view")
        assert_bits_equal(x["k"], y["k"], f"call {i}: K view")
    assert sub.kv_offset == c["L"] + 3 and sub.gen_offset == 3
    misses = sum(int((sub.select_sets - x["cnts"]).sum()) for x in d_sub)
    assert misses > 0
    # four single-sequence caches: sequence b of the batch behaves exactly like a batch of one
    for b in range(B):
        single, _ = _device_prefill(case, 1, only=b)
        for n in names:
            a, s1 = getattr(sub, n)[:, b:b + 1].cpu(), getattr(single, n).cpu()
            # (the batched cache has decoded 3 steps by now: compare what decoding does not touch, then the decode itself)
            if n in ("U", "SV", "k_landmark", "k_landmark_idx", "v_cache_cpu"):
                assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                                   s1.view(torch.int16) if s1.dtype == torch.bfloat16 else s1), f"sequence {b}: {n}"
        d1 = _decode3(case, single, inputs, [b])
        for i, (x, y) in enumerate(zip(d_sub, d1)):
            assert torch.equal(x["pos"][b:b + 1], y["pos"]) and torch.equal(x["cnts"][b:b + 1], y["cnts"]), f"sequence {b} call {i}"
            assert_bits_equal(x["v"][b:b + 1], y["v"], f"sequence {b} call {i}: V view")
            assert_bits_equal(x["k"][b:b + 1], y["k"], f"sequence {b} call {i}: K view")
        del single
