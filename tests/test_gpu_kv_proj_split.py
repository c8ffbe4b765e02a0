"""GPU: the QKV projection split by rows - q rows as a launch of their own (skv_q_gemv_rope), k / v rows as a role of a
selection launch (skv_select_chunks_fused_kv_proj) - against the one launch (skv_qkv_gemv_rope_update).  The arithmetic of
every row is the same, so every comparison is torch.equal on raw bits."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HID, HQ, D = 4096, 32, 128
ROWS, FIRST_GEN = 40, 8          # cache rows per head; rows [FIRST_GEN, ROWS) play the generated-row slack
PLACEMENTS = {"scan": 0, "topk": 1}
CASES = {"neox_kv8": (8, False), "glm_kv4": (4, True)}


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t


@pytest.fixture(scope="module")
def proj():
    """Per case: weights and inputs of one token, built once."""
    out = {}
    for name, (kv, glm) in CASES.items():
        g = torch.Generator(device=DEV).manual_seed(11 + kv)
        r = lambda *s, scale=1.0: (torch.randn(*s, device=DEV, generator=g) * scale).bfloat16()   # noqa: E731
        width = 64 if glm else 128
        out[name] = dict(kv=kv, glm=glm, w=r((HQ + 2 * kv) * D, HID, scale=HID ** -0.5), x=r(1, 1, HID), res=r(1, 1, HID),
                         nw=r(HID, scale=0.2) + 1, bias=r((HQ + 2 * kv) * D, scale=0.1) if glm else None,
                         cs=r(64, width), pos=torch.tensor([[37]], device=DEV))
    return out


def select_inputs(kv, N, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    S = 32
    lm = torch.randn(kv, N, D, device=DEV, generator=g).bfloat16()
    idx = torch.arange(N, device=DEV).repeat(kv, 1)
    cached = torch.stack([torch.randperm(N, device=DEV, generator=g)[:S] for _ in range(kv)])
    return lm, idx, cached, S


def run_selection(L, q, lm, idx, cached, S, kv_desc):
    """One fused selection (in-place layout) from a fresh state; returns everything its two launches leave behind."""
    from shadowkv_amd import _lib
    kv, N = lm.shape[0], lm.shape[1]
    G = HQ // kv
    ws = torch.zeros(L.skv_select_workspace_bytes(kv, G, N), dtype=torch.uint8, device=DEV)
    state = torch.zeros(L.skv_select_state_bytes(kv, G), dtype=torch.uint8, device=DEV)
    pos_ids = cached.clone()
    miss = torch.zeros(kv, S, dtype=torch.int32, device=DEV)
    dst = torch.zeros_like(miss)
    cnts = torch.zeros(kv, dtype=torch.int32, device=DEV)
    args = (q.data_ptr(), lm.data_ptr(), idx.data_ptr(), pos_ids.data_ptr(), miss.data_ptr(), dst.data_ptr(), cnts.data_ptr(),
            ws.data_ptr(), 0, kv, G, N, S, S, 0, 1.0 / math.sqrt(D), state.data_ptr(), 0, 0, 0, 0, 0, 0.0)
    st = torch.cuda.current_stream().cuda_stream
    if kv_desc is None:
        _lib.check(L.skv_select_chunks_fused(*args, st), "select_chunks_fused")
    else:
        _lib.check(L.skv_select_chunks_fused_kv_proj(*args, ctypes.byref(kv_desc), st), "select_chunks_fused_kv_proj")
    torch.cuda.synchronize()
    return dict(ws=ws, state=state, pos_ids=pos_ids, miss=miss, dst=dst, cnts=cnts)


def nan_caches(kv):
    k = torch.full((1, kv, ROWS, D), float("nan"), device=DEV).bfloat16()
    return k, k.clone()


@pytest.fixture(scope="module")
def fused_ref(proj):
    """The one launch, once per (case, append row): q, h and the caches it leaves (NaN everywhere but the appended row)."""
    from shadowkv_amd import tensor_op
    out = {}
    for name, p in proj.items():
        for row in (FIRST_GEN, 20, ROWS - 1):
            k, v = nan_caches(p["kv"])
            h, q = tensor_op.norm_qkv_rope_update(p["x"], p["res"], p["nw"], 1e-5, p["w"], p["bias"], p["cs"], p["pos"],
                                                  torch.tensor([row], device=DEV), k, v, HQ, p["kv"])
            torch.cuda.synchronize()
            assert not torch.isnan(k[0, :, row].float()).any() and not torch.isnan(v[0, :, row].float()).any()
            out[name, row] = (h, q, k, v)
    return out


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("row", [FIRST_GEN, 20, ROWS - 1])
@pytest.mark.parametrize("case", list(CASES))
def test_q_launch_plus_kv_role_reproduce_the_one_launch(proj, fused_ref, case, row, placement):
    from shadowkv_amd import _lib, tensor_op
    p = proj[case]
    h0, q0, k0, v0 = fused_ref[case, row]
    k, v = nan_caches(p["kv"])
    row_idx = torch.tensor([row], device=DEV)          # (the descriptor points at it: alive until the selection call)
    h, q, desc = tensor_op.norm_q_rope(p["x"], p["res"], p["nw"], 1e-5, p["w"], p["bias"], p["cs"], p["pos"],
                                       row_idx, k, v, HQ, p["kv"], placement=PLACEMENTS[placement])
    torch.cuda.synchronize()
    assert torch.equal(bits(q), bits(q0)) and torch.equal(bits(h), bits(h0))
    assert torch.isnan(k.float()).all() and torch.isnan(v.float()).all()          # the q launch appends nothing
    lm, idx, cached, S = select_inputs(p["kv"], 520, seed=3)
    run_selection(_lib.lib(), q, lm, idx, cached, S, desc)
    # the appended rows carry the one launch's bits, and every other row still holds its NaN sentinel
    assert torch.equal(bits(k), bits(k0)) and torch.equal(bits(v), bits(v0))
    assert torch.isnan(k[0, :, :row].float()).all() and torch.isnan(k[0, :, row + 1:].float()).all()
    assert torch.isnan(v[0, :, :row].float()).all() and torch.isnan(v[0, :, row + 1:].float()).all()


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("N", [520, 200])
@pytest.mark.parametrize("case", list(CASES))
def test_selection_launches_unchanged_by_the_role(proj, fused_ref, case, N, placement):
    """Keys, slot-major logits and per-tile partials (the workspace), the select state, ids / miss lists / slots / counts:
    the same bytes with and without the role's workgroups in the grid."""
    from shadowkv_amd import _lib, tensor_op
    p = proj[case]
    _, q0, _, _ = fused_ref[case, 20]
    lm, idx, cached, S = select_inputs(p["kv"], N, seed=5 + N)
    plain = run_selection(_lib.lib(), q0, lm, idx, cached, S, None)
    k, v = nan_caches(p["kv"])
    row_idx = torch.tensor([20], device=DEV)
    h, q, desc = tensor_op.norm_q_rope(p["x"], p["res"], p["nw"], 1e-5, p["w"], p["bias"], p["cs"], p["pos"],
                                       row_idx, k, v, HQ, p["kv"], placement=PLACEMENTS[placement])
    with_role = run_selection(_lib.lib(), q, lm, idx, cached, S, desc)
    for name in plain:
        assert torch.equal(plain[name], with_role[name]), name
    assert int(plain["cnts"].min()) >= 0 and int(plain["cnts"].max()) <= S


def test_role_refuses_unsupported_shapes(proj):
    from shadowkv_amd import _lib
    L = _lib.lib()
    p = 0x1000
    d = _lib.KvProjDesc(p, p, p, None, p, p, p, p, p, 128, 40 * 128, 1e-5, 4096, 32, 8, 128, 64, 40, 1, 1)
    args = (p, p, p, p, p, p, p, p, 0, 8, 4, 520, 32, 32, 0, 0.088, p, 0, 0, 0, 0, 0, 0.0)
    for field, value, rc in (("K", 2048, -2), ("head_dim", 64, -2), ("rope_mode", 3, -2), ("placement", 2, -1), ("h", None, -1)):
        bad = _lib.KvProjDesc.from_buffer_copy(d)
        setattr(bad, field, value)
        assert L.skv_select_chunks_fused_kv_proj(*args, ctypes.byref(bad), 0) == rc, field
    assert L.skv_q_gemv_rope(p, p, 0, p, 1e-5, 0, 0, p, p, 0, p, 2048, 32, 8, 128, 128, 64, 1, 0) == -2


# ---------------------------------------------------------------------------------------------------------- captured step
def _model(glm, batch=1):
    from shadowkv_amd import llama
    cfg = llama.GLM_4_9B_1M if glm else llama.LLAMA_3_1_8B
    m = llama.DecoderLM(cfg=cfg, batch_size=batch, max_length=4104, device=DEV, sparse_budget=256, rank=160, chunk_size=8,
                        num_layers=2, seed=1234, chunk_layout="inplace", overlap_attention=True)
    llama.build_synthetic_context(m, 4104, seed=4321)
    m.kv_cache.fused_select = True
    return m, llama


def _captured_run(glm, split, placement="topk"):
    """Two captures, each an eager warm-up step + 3 replays (4 steps); after each replay: logits, token, caches, slot -> chunk map."""
    m, llama = _model(glm)
    m.split_kv_proj = split
    m.kv_proj_placement = PLACEMENTS[placement]
    held = {}
    fwd = m.forward_fused

    def rec(*a, **k):
        held["logits"] = fwd(*a, **k)
        return held["logits"]
    m.forward_fused = rec
    out = []
    tok = torch.tensor([[17]], device=DEV)
    for _ in range(2):
        dec = llama.GraphDecoder(m, temperature=0.6, seed=7)
        dec.token.copy_(tok)
        dec.capture(warmup=1)
        for _ in range(3):
            tok = dec.step().clone()
            torch.cuda.synchronize()
            c = m.kv_cache
            out.append((held["logits"].clone(), tok.clone(), c.k_cache_buffer.clone(), c.v_cache_buffer.clone(),
                        c.position_ids.clone()))
    return m, out


@pytest.mark.parametrize("glm", [False, True], ids=["llama31_4k", "glm_4k"])
def test_captured_step_split_on_equals_off(glm):
    m_off, off = _captured_run(glm, split=False)
    assert m_off.kv_proj_split_launches == 0 and m_off.kv_proj_fused_launches > 0
    for placement in PLACEMENTS:
        m_on, on = _captured_run(glm, split=True, placement=placement)
        assert m_on.kv_proj_fused_launches == 0 and m_on.kv_proj_split_launches > 0
        assert len(on) == len(off) == 6
        for a, b in zip(on, off):
            for x, y in zip(a, b):
                assert torch.equal(bits(x), bits(y))


def test_fallbacks_keep_the_one_launch():
    """A batch of 2 and the call-order path (fused=False) never take the split path; the switch off neither."""
    m, _ = _model(False, batch=2)
    assert m.split_kv_proj
    tok = torch.tensor([[5], [9]], device=DEV)
    m.decode_step(tok, temperature=0.0)
    assert m.kv_proj_split_launches == 0 and m.kv_proj_fused_launches == m.num_layers
    del m
    m, _ = _model(False)
    tok = torch.tensor([[5]], device=DEV)
    c = m.kv_cache
    c.lazy_value_fetch, c.inplace_methods = True, True        # (the call order over the in-place layout)
    m.decode_step(tok, temperature=0.0, fused=False)
    c.lazy_value_fetch, c.inplace_methods = False, False
    assert m.kv_proj_split_launches == 0 and m.kv_proj_fused_launches == 0       # (the call order has its own projection)
    m.decode_step(tok, temperature=0.0)
    assert m.kv_proj_split_launches == m.num_layers and m.kv_proj_fused_launches == 0
    m.split_kv_proj = False
    m.decode_step(tok, temperature=0.0)
    assert m.kv_proj_split_launches == m.num_layers and m.kv_proj_fused_launches == m.num_layers
