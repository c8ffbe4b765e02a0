"""The selection chain on the device at logit ranges past every cut-off of the softmax contract: the
designed cases of tests/wide_range_cases.py (validated on the CPU by tests/test_wide_range_cpu.py) through every selection
entry of the C ABI, bit for bit against the oracle and, where the case has one, against its closed-form selection."""
import functools

import pytest
import torch

import oracle
import wide_range_cases as W
from util import assert_bits_equal, open_parity_record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = W.selection_cases()
SEQS = W.sequences()


def _lib():
    from shadowkv_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _record(line):
    try:
        with open_parity_record("wide_range_tests.txt") as f:
            f.write(line + "\n")
    except OSError:
        pass


def _oracle_softmax(q, lm, blocks, G, N, alpha):
    T = (N + 255) // 256
    D = torch.zeros(blocks, G, N, dtype=torch.bfloat16); P = torch.zeros_like(D)
    nm = torch.zeros(blocks, T, G); sm = torch.zeros(blocks, T, G)
    oracle.batch_gemm_softmax(q, lm, D, nm, sm, P, blocks, G, N, 128, alpha)
    return D, P, nm, sm


@functools.lru_cache(maxsize=None)
def _reference(i):
    """The oracle's results of case i, computed once: logits, P, Norm / Sum (tile partials, the finals in the tile-0 slots), the
    partials of tile 0 itself, the group-max scores, the selected ids and the reference-order diff."""
    c = CASES[i]
    D, P, nm, sm = _oracle_softmax(c.q, c.lm, c.blocks, c.G, c.N, c.alpha)
    # tile 0's own partials: the oracle overwrites them with the finals, so score tile 0 again as tile 1 of a two-tile row
    n0 = min(256, c.N)
    two = torch.cat((c.lm[:, :256], c.lm[:, :n0]), dim=1).contiguous()
    if two.shape[1] > 256:
        _, _, nm2, sm2 = _oracle_softmax(c.q, two, c.blocks, c.G, two.shape[1], c.alpha)
        pm0, ps0 = nm2[:, 1], sm2[:, 1]
    else:
        pm0 = ps0 = None
    score = P.float().max(dim=1).values.bfloat16()                      # the max of bf16 numbers is one of them: exact
    sel = oracle.group_max_topk(P, c.lm_idx, c.blocks, c.G, c.N, c.S)
    cached = c.cached.clone(); off = torch.zeros(c.blocks, c.S, dtype=torch.int32); cnt = torch.zeros(c.blocks, dtype=torch.int32)
    oracle.reorder_keys_and_compute_offsets(cached, sel, off, cnt, 1, c.blocks, c.S)
    return dict(D=D, P=P, nm=nm, sm=sm, pm0=pm0, ps0=ps0, score=score, sel=sel, cached=cached, off=off, cnt=cnt)


def _inplace_expected(cached, sel):
    """The in-place layout in integers: ids selected again keep their slot; the misses (ascending id) take the slots of the
    evicted ids (ascending slot)."""
    blocks, S = cached.shape
    exp = cached.clone(); cnts = []; miss_ids = []; dst = []
    for b in range(blocks):
        chosen = set(sel[b].tolist())
        resident = cached[b].tolist()
        keep = [i for i, cid in enumerate(resident) if cid in chosen and cid >= 0 and resident.index(cid) == i]
        kept_ids = {resident[i] for i in keep}
        free = [i for i in range(S) if i not in set(keep)]
        misses = sorted(chosen - kept_ids)
        assert len(free) == len(misses)
        for slot, cid in zip(free, misses):
            exp[b, slot] = cid
        cnts.append(len(keep)); miss_ids.append(misses); dst.append(free)
    return exp, cnts, miss_ids, dst


def _check_closed_form(c, sel, what):
    want = c.expected_ids()
    if want is not None:
        assert torch.equal(sel.cpu(), want), f"{c.name}: {what}: the closed-form selection"


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.name for c in CASES])
def test_batch_gemm_softmax_and_scan(i):
    """skv_batch_gemm_softmax (D, Norm, Sum, Softmax: every P value is an ABI output) and skv_score_landmarks (logits, tile
    partials) against the oracle and the designed profile."""
    c, r = CASES[i], _reference(i)
    L = _lib()
    B, G, N = c.blocks, c.G, c.N
    T = (N + 255) // 256
    qd, lmd = c.q.to(DEV), c.lm.to(DEV)
    D1 = torch.zeros(B, G, N, dtype=torch.bfloat16, device=DEV); P1 = torch.zeros_like(D1)
    N1 = torch.zeros(B, T, G, device=DEV); S1 = torch.zeros(B, T, G, device=DEV)
    L.check(L.lib().skv_batch_gemm_softmax(qd.data_ptr(), lmd.data_ptr(), D1.data_ptr(), N1.data_ptr(), S1.data_ptr(), P1.data_ptr(),
                                           B, G, N, 128, c.alpha, 0.0, _stream()), "batch_gemm_softmax")
    D2 = torch.zeros(B, G, N, dtype=torch.bfloat16, device=DEV)
    pm = torch.zeros(B, T, G, device=DEV); ps = torch.zeros(B, T, G, device=DEV)
    L.check(L.lib().skv_score_landmarks(qd.data_ptr(), lmd.data_ptr(), D2.data_ptr(), pm.data_ptr(), ps.data_ptr(), B, G, N, c.alpha,
                                        _stream()), "score_landmarks")
    torch.cuda.synchronize()
    assert_bits_equal(c.logits, D1, f"{c.name}: logits against the designed profile")
    assert_bits_equal(r["D"], D1, f"{c.name}: logits D")
    assert torch.equal(r["nm"].view(torch.int32), N1.cpu().view(torch.int32)), f"{c.name}: Norm (tile maxima + final maximum)"
    assert torch.equal(r["sm"].view(torch.int32), S1.cpu().view(torch.int32)), f"{c.name}: Sum (tile sums + final 1 / sum)"
    assert_bits_equal(r["P"], P1, f"{c.name}: softmax P")
    assert_bits_equal(r["D"], D2, f"{c.name}: scan logits")
    pm, ps = pm.cpu(), ps.cpu()
    assert torch.equal(r["nm"][:, 1:].view(torch.int32), pm[:, 1:].view(torch.int32)), f"{c.name}: scan tile maxima"
    assert torch.equal(r["sm"][:, 1:].view(torch.int32), ps[:, 1:].view(torch.int32)), f"{c.name}: scan tile sums"
    if r["pm0"] is not None:
        assert torch.equal(r["pm0"].contiguous().view(torch.int32), pm[:, 0].contiguous().view(torch.int32)), f"{c.name}: tile 0 maximum"
        assert torch.equal(r["ps0"].contiguous().view(torch.int32), ps[:, 0].contiguous().view(torch.int32)), f"{c.name}: tile 0 sum"


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.name for c in CASES])
def test_three_launch_selection(i):
    """skv_select_chunks (P through softmax_out, selected ids, reordered resident ids, offsets, hit counts),
    skv_select_chunks_inplace (selected ids, in-place resident ids, miss ids, destination slots, hit counts) and
    skv_select_from_scores in both layouts, against the oracle; the closed-form selection where the case states one."""
    c, r = CASES[i], _reference(i)
    L = _lib()
    B, G, N, S = c.blocks, c.G, c.N, c.S
    qd, lmd, lid = c.q.to(DEV), c.lm.to(DEV), c.lm_idx.to(DEV)
    ws = torch.empty(L.lib().skv_select_workspace_bytes(B, G, N), dtype=torch.uint8, device=DEV)
    # reference slot order
    P = torch.zeros(B, G, N, dtype=torch.bfloat16, device=DEV); sel = torch.zeros(B, S, dtype=torch.int64, device=DEV)
    ca = c.cached.to(DEV); off = torch.zeros(B, S, dtype=torch.int32, device=DEV); cnt = torch.zeros(B, dtype=torch.int32, device=DEV)
    L.check(L.lib().skv_select_chunks(qd.data_ptr(), lmd.data_ptr(), lid.data_ptr(), ca.data_ptr(), off.data_ptr(), cnt.data_ptr(),
                                      ws.data_ptr(), P.data_ptr(), sel.data_ptr(), B, G, N, S, c.alpha, _stream()), "select_chunks")
    torch.cuda.synchronize()
    assert_bits_equal(r["P"], P, f"{c.name}: softmax_out")
    assert torch.equal(r["sel"], sel.cpu()), f"{c.name}: selected ids"
    assert torch.equal(r["cnt"], cnt.cpu()) and torch.equal(r["cached"], ca.cpu()) and torch.equal(r["off"], off.cpu()), \
        f"{c.name}: hit counts / reordered ids / offsets"
    _check_closed_form(c, sel, "skv_select_chunks")
    # in-place layout
    exp, cnts, miss_ids, dst = _inplace_expected(c.cached, r["sel"])
    cb = c.cached.to(DEV)
    mids = torch.full((B, S), -7, dtype=torch.int32, device=DEV); slots = torch.full((B, S), -7, dtype=torch.int32, device=DEV)
    cnt2 = torch.zeros(B, dtype=torch.int32, device=DEV); sel2 = torch.zeros(B, S, dtype=torch.int64, device=DEV)
    P2 = torch.zeros(B, G, N, dtype=torch.bfloat16, device=DEV)
    L.check(L.lib().skv_select_chunks_inplace(qd.data_ptr(), lmd.data_ptr(), lid.data_ptr(), cb.data_ptr(), mids.data_ptr(),
                                              slots.data_ptr(), cnt2.data_ptr(), ws.data_ptr(), P2.data_ptr(), sel2.data_ptr(), B, G, N, S,
                                              S, 0, c.alpha, _stream()), "select_chunks_inplace")
    torch.cuda.synchronize()
    assert_bits_equal(r["P"], P2, f"{c.name}: in-place softmax_out")
    assert torch.equal(sel2.cpu(), r["sel"]) and cnt2.cpu().tolist() == cnts and torch.equal(cb.cpu(), exp), f"{c.name}: in-place"
    for b in range(B):
        k = cnts[b]
        assert mids[b, k:].cpu().tolist() == miss_ids[b] and slots[b, k:].cpu().tolist() == dst[b], (c.name, b)
        assert slots[b, :k].cpu().tolist() == sorted(set(range(S)) - set(dst[b])), (c.name, b)
    # the top-k stage alone on the oracle's scores, both layouts
    stride = (N + 7) // 8 * 8
    sc = torch.full((B, stride), 0x7f7f, dtype=torch.int16).view(torch.bfloat16)
    sc[:, :N] = r["score"]
    scd = sc.to(DEV)
    for inplace in (False, True):
        cc = c.cached.to(DEV); o3 = torch.full((B, S), -7, dtype=torch.int32, device=DEV); d3 = torch.full((B, S), -7, dtype=torch.int32, device=DEV)
        n3 = torch.zeros(B, dtype=torch.int32, device=DEV); s3 = torch.zeros(B, S, dtype=torch.int64, device=DEV)
        L.check(L.lib().skv_select_from_scores(scd.data_ptr(), stride, lid.data_ptr(), cc.data_ptr(), o3.data_ptr(),
                                               d3.data_ptr() if inplace else 0, n3.data_ptr(), s3.data_ptr(), B, N, S, S, 0, _stream()),
                "select_from_scores")
        torch.cuda.synchronize()
        assert torch.equal(s3.cpu(), r["sel"]), f"{c.name}: select_from_scores ids (in-place {inplace})"
        _check_closed_form(c, s3, "skv_select_from_scores")
        if inplace:
            assert n3.cpu().tolist() == cnts and torch.equal(cc.cpu(), exp)
            for b in range(B):
                assert o3[b, cnts[b]:].cpu().tolist() == miss_ids[b] and d3[b, cnts[b]:].cpu().tolist() == dst[b]
        else:
            assert torch.equal(n3.cpu(), r["cnt"]) and torch.equal(cc.cpu(), r["cached"]) and torch.equal(o3.cpu(), r["off"])


class _Fused:
    """skv_select_chunks_fused with its state, next to the three-launch entry fed the same queries from the same resident set."""

    def __init__(self, blocks, G, N, S, lm, lm_idx, cached, alpha, inplace):
        L = self.L = _lib()
        assert L.lib().skv_select_fused_supported(G, N, S) == 1
        self.B, self.G, self.N, self.S, self.alpha, self.inplace = blocks, G, N, S, alpha, inplace
        self.lmd, self.lid = lm.to(DEV), lm_idx.to(DEV)
        self.ws_a = torch.empty(L.lib().skv_select_workspace_bytes(blocks, G, N), dtype=torch.uint8, device=DEV)
        self.ws_b = torch.empty_like(self.ws_a)
        self.state = torch.zeros(L.lib().skv_select_state_bytes(blocks, G), dtype=torch.uint8, device=DEV)
        L.check(L.lib().skv_select_state_init(self.state.data_ptr(), blocks, G, _stream()), "select_state_init")
        self.ca, self.cb = cached.to(DEV), cached.to(DEV)
        self.soff = L.lib().skv_select_state_stats_offset(blocks, G)

    def _bufs(self):
        B, S = self.B, self.S
        return (torch.full((B, S), -7, dtype=torch.int32, device=DEV), torch.full((B, S), -7, dtype=torch.int32, device=DEV),
                torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, S, dtype=torch.int64, device=DEV))

    def step(self, q, what):
        """One step on both paths; asserts they agree bit for bit and the stats word; -> (selected ids, paths per block)."""
        L, B, G, N, S = self.L, self.B, self.G, self.N, self.S
        qd = q.to(DEV)
        ma, sa, na, oa = self._bufs()
        mb, sb, nb, ob = self._bufs()
        if self.inplace:
            L.check(L.lib().skv_select_chunks_inplace(qd.data_ptr(), self.lmd.data_ptr(), self.lid.data_ptr(), self.ca.data_ptr(),
                                                      ma.data_ptr(), sa.data_ptr(), na.data_ptr(), self.ws_a.data_ptr(), 0, oa.data_ptr(),
                                                      B, G, N, S, S, 0, self.alpha, _stream()), "select_chunks_inplace")
        else:
            L.check(L.lib().skv_select_chunks(qd.data_ptr(), self.lmd.data_ptr(), self.lid.data_ptr(), self.ca.data_ptr(), ma.data_ptr(),
                                              na.data_ptr(), self.ws_a.data_ptr(), 0, oa.data_ptr(), B, G, N, S, self.alpha, _stream()),
                    "select_chunks")
        L.check(L.lib().skv_select_chunks_fused(qd.data_ptr(), self.lmd.data_ptr(), self.lid.data_ptr(), self.cb.data_ptr(), mb.data_ptr(),
                                                sb.data_ptr() if self.inplace else 0, nb.data_ptr(), self.ws_b.data_ptr(), ob.data_ptr(),
                                                B, G, N, S, S, 0, self.alpha, self.state.data_ptr(), 0, 0, 0, 0, 0, 0.0, _stream()),
                "select_chunks_fused")
        torch.cuda.synchronize()
        assert torch.equal(oa, ob), f"{what}: selected ids"
        assert torch.equal(na, nb), f"{what}: hit counts"
        assert torch.equal(self.ca, self.cb), f"{what}: resident ids"
        assert torch.equal(ma, mb), f"{what}: offsets / miss ids"
        if self.inplace:
            assert torch.equal(sa, sb), f"{what}: destination slots"
        st = self.state.view(torch.float32)[:B * G].cpu()
        assert not bool(torch.isnan(st).any()), f"{what}: NaN in the log-normalisers the launch leaves behind"
        stats = self.state[self.soff:self.soff + 8 * B].view(torch.int32).view(B, 2).cpu()
        for path, ncand in stats.tolist():
            assert path in (0, 1, 2, 3), (what, path)
            assert (path & 2) or S <= ncand <= 2048, f"{what}: the candidates contain the selection, or every slot was evaluated"
        return ob.cpu(), stats.tolist(), st


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.name for c in CASES])
def test_fused_selection_single_cases(i, inplace):
    """skv_select_chunks_fused on every case, twice with the same query (first step: no normalisers, every slot or a searched
    level; second step: this row's exact normalisers in the state): identical to the three-launch entry, to the oracle and to
    the closed form."""
    c, r = CASES[i], _reference(i)
    f = _Fused(c.blocks, c.G, c.N, c.S, c.lm, c.lm_idx, c.cached, c.alpha, inplace)
    for step in range(2):
        sel, stats, _ = f.step(c.q, f"{c.name} step {step}")
        assert torch.equal(sel, r["sel"]), f"{c.name} step {step}: selected ids against the oracle"
        _check_closed_form(c, sel, f"fused step {step}")
        _record(f"selection {c.name:34s} fused {'in-place ' if inplace else 'reference'} step {step}: (path, candidates) per block {stats}")
    assert sorted(f.cb[0].cpu().tolist()) == sorted(r["sel"][0].tolist())


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("k", range(len(SEQS)), ids=[s.name for s in SEQS])
def test_fused_selection_scale_jump_sequences(k, inplace):
    """Eight steps whose query scale jumps by 100x (and by 2^118), flips its sign and ends on a cliff: under the previous step's
    log-normalisers every key of a row saturates at 32767, at 0, or the row splits between the two (test_wide_range_cpu.py
    counts them).  Step by step: the fused entry == the three-launch entry == the oracle; step 6 == the cliff's closed form."""
    s = SEQS[k]
    f = _Fused(s.blocks, s.G, s.N, s.S, s.lm, s.lm_idx, s.cached, s.alpha, inplace)
    for t in range(8):
        sel, stats, st = f.step(s.q[t], f"{s.name} step {t}")
        D, P, nm, sm = _oracle_softmax(s.q[t], s.lm, s.blocks, s.G, s.N, s.alpha)
        assert_bits_equal(s.logits[t], D, "designed logits")
        want = oracle.group_max_topk(P, s.lm_idx, s.blocks, s.G, s.N, s.S)
        assert torch.equal(sel, want), f"{s.name} step {t}: selected ids against the oracle"
        assert bool(torch.isfinite(st).all()), f"{s.name} step {t}: the state is this step's log-normalisers: finite"
        if t == 6:
            for b in range(s.blocks):
                assert sel[b].tolist() == s.lm_idx[b][torch.tensor(s.cliff_expected[b])].tolist(), "the cliff's closed form"
        _record(f"selection {s.name:34s} fused {'in-place ' if inplace else 'reference'} step {t} (scale {s.scales[t]:.3g}): "
                f"(path, candidates) per block {stats}")


def test_cache_steps_on_cliff_queries_with_and_without_early_fetch():
    """ShadowKVCache_CPU (in-place layout, 8 KV heads, fused selection) over a landmark table of cliff profiles: three steps
    whose k-th score is exactly 0, so the early fetch's threshold max_g + ln(k-th value / inv_g) + margin is -inf and the
    near-miss list is cut from all-zero scores.  With the early fetch and the near-miss staging on, against the plain steps:
    selection, hit counts, miss lists, attention output and both caches bit for bit; the selection is the closed form; the
    thresholds and log-normalisers left behind hold no NaN."""
    from test_gpu_kv_cache import _headline_cache, _gate_up_with_near_pull, _check_staging_invariant
    ca, cs, g = _headline_cache(8, False, L=16384, seed=53)
    cb, _, _ = _headline_cache(8, False, L=16384, seed=53)
    B, G, S = ca.block_num, ca.num_key_value_groups, ca.select_sets
    N = ca.k_landmark.shape[-2]
    lm, qs, expected = W.cliff_steps(B, G, N, S, entry=16.0)
    for c in (ca, cb):
        c.k_landmark[0][0].copy_(lm.to(DEV))
    ca.near_lists = 2
    ca.enable_early_fetch(near=True)
    assert ca.fused_select and cb.fused_select
    lm_idx = ca.k_landmark_idx[0][0].cpu()
    kv_len = ca.sparse_end + 2
    gw = torch.Generator(device=DEV).manual_seed(3)
    o = ca._early["offsets"]
    for step in range(3):
        q = qs[step].view(1, B * G, 1, 128).to(DEV)
        oa = ca.select_fetch_attend_inplace(0, q, cs, kv_len=kv_len)
        ob = cb.select_fetch_attend_inplace(0, q, cs, kv_len=kv_len)
        torch.cuda.synchronize()
        _check_staging_invariant(ca, 0)
        assert torch.equal(ca.cnts, cb.cnts) and torch.equal(ca.offsets, cb.offsets), step
        assert torch.equal(ca.position_ids, cb.position_ids), step
        assert torch.equal(oa.view(torch.int16), ob.view(torch.int16)), step
        assert torch.equal(ca.v_cache_buffer.view(torch.int16), cb.v_cache_buffer.view(torch.int16)), step
        assert torch.equal(ca.k_cache_buffer.view(torch.int16), cb.k_cache_buffer.view(torch.int16)), step
        ids = ca.position_ids[0][0].cpu()
        for b in range(B):
            assert sorted(ids[b].tolist()) == lm_idx[b][torch.tensor(expected[step][b])].tolist(), (step, b)
        dthr = ca._early["states"][0][o[0]:o[0] + 4 * B * G].view(torch.float32).cpu()
        norm = ca._sel_state[0][:4 * B * G].view(torch.float32).cpu()
        assert not bool(torch.isnan(dthr).any()) and not bool(torch.isnan(norm).any()), (step, dthr, norm)
        assert not bool(torch.isnan(oa.float()).any())
        _record(f"cache cliff step {step}: early thresholds -inf {int(torch.isinf(dthr).sum())} of {dthr.numel()}, fused stats "
                f"{ca.fused_select_stats(0).tolist()}")
        _gate_up_with_near_pull(ca, 0, gw)
        _check_staging_invariant(ca, 0)
