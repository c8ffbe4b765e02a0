"""The designed wide-range selection cases (tests/wide_range_cases.py) on the CPU oracle alone: the logits are the designed
bf16 profile bit for bit, the closed-form selections hold, and every case really takes the branch it was built for - the counts
are printed (pytest -s) and must be non-zero.  tests/test_gpu_wide_range_selection.py runs the same cases on the device."""
import math

import numpy as np
import pytest
import torch

import oracle
import wide_range_cases as W
from util import assert_bits_equal, attention_tolerance, standalone_pass_labels

CASES = W.selection_cases()
SEQS = W.sequences()


def oracle_softmax(q, lm, blocks, G, N, alpha):
    T = (N + 255) // 256
    D = torch.zeros(blocks, G, N, dtype=torch.bfloat16); P = torch.zeros_like(D)
    nm = torch.zeros(blocks, T, G); sm = torch.zeros(blocks, T, G)
    oracle.batch_gemm_softmax(q, lm, D, nm, sm, P, blocks, G, N, 128, alpha)
    return D, P, nm, sm


def edge_counts(D, P, fm, finv):
    """Which cut-offs of the contract a row set reaches.  D, P bf16 [blocks][G][N]; fm, finv f32 [blocks][G] (the finals).
    x = D - m in f32, as the kernels form it; the exp_to_fixed classes are counted on x_t = D - m_t (tile maximum) from the
    exponent the contract's exp has there: e = 0 for x_t < -80 (`ex == 0`), e < 2^-36 for x_t < -36 ln 2 (`sh <= -24`), a
    right shift (-24 < sh < 0) down to e < 2^-13.  (The designed logits keep 0.005 clear of both boundaries, 1e4 times the error of the exp.)"""
    blocks, G, N = D.shape
    d = D.float()
    x = d - fm.unsqueeze(-1)
    T = (N + 255) // 256
    pad = torch.full((blocks, G, T * 256 - N), -math.inf)
    dt = torch.cat((d, pad), -1).view(blocks, G, T, 256)
    mt = dt.max(dim=-1, keepdim=True).values
    xt = (dt - mt)[torch.isfinite(dt)]
    assert not bool(((xt + 36 * math.log(2)).abs() < 0.005).any()) and not bool(((xt + 13 * math.log(2)).abs() < 0.005).any())
    pb = P.view(torch.int16).to(torch.int32) & 0xFFFF
    prod = torch.exp(x.double()) * finv.double().unsqueeze(-1)
    score = P.float().max(dim=1).values
    return {
        "x < -80": int((x < -80.0).sum()),
        "x == -80": int((x == -80.0).sum()),
        "fixed: e == 0": int((xt < -80.0).sum()),
        "fixed: sh <= -24": int(((xt >= -80.0) & (xt < -36 * math.log(2))).sum()),
        "fixed: shifted": int(((xt >= -36 * math.log(2)) & (xt < -13 * math.log(2))).sum()),
        "tiles: exp(m_t - m) == 0": int(((mt.squeeze(-1) - fm.unsqueeze(-1)) < -80.0).sum()),
        "tiles: m_t < m": int((mt.squeeze(-1) < fm.unsqueeze(-1)).sum()),
        "P bf16-subnormal": int((((pb & 0x7F80) == 0) & ((pb & 0x7F) != 0)).sum()),
        "P product f32-denormal": int(((x >= -80.0) & (prod < 2.0 ** -126)).sum()),
        "rows with < S positive scores": None,            # filled by the caller (needs S)
        "min positive scores per row": int((score > 0).sum(dim=-1).min()),
    }


REQUIRED = {
    "cliff": ("x < -80", "fixed: e == 0", "rows with < S positive scores"),
    "straddle": ("x < -80", "x == -80", "fixed: e == 0", "fixed: sh <= -24", "fixed: shifted", "tiles: exp(m_t - m) == 0",
                 "tiles: m_t < m", "rows with < S positive scores"),
    "subnormal_p": ("P bf16-subnormal", "P product f32-denormal", "fixed: sh <= -24", "x == -80"),
    "huge_flat": ("x < -80", "rows with < S positive scores"),
}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_reaches_its_edge(case):
    c = case
    D, P, nm, sm = oracle_softmax(c.q, c.lm, c.blocks, c.G, c.N, c.alpha)
    assert_bits_equal(c.logits, D, f"{c.name}: designed logits")
    fm, finv = nm[:, 0], sm[:, 0]
    cnt = edge_counts(D, P, fm, finv)
    score = P.float().max(dim=1).values
    cnt["rows with < S positive scores"] = int(((score > 0).sum(dim=-1) < c.S).sum())
    print(f"\n{c.name}: " + ", ".join(f"{k} {v}" for k, v in cnt.items()))
    assert bool(torch.isfinite(P.float()).all()) and bool(torch.isfinite(finv).all())
    for key in REQUIRED[c.name.split("[")[0].split("/")[0]]:
        assert cnt[key] > 0, f"{c.name} does not reach its edge: {key} == 0"
    sel = oracle.group_max_topk(P, None, c.blocks, c.G, c.N, c.S)
    if c.expected is not None:
        for b in range(c.blocks):
            assert sel[b].tolist() == c.expected[b], f"{c.name} block {b}: the closed-form selection"
    if c.name.startswith("straddle"):
        live = c.extra["n_live"]
        assert all(live[b] == (c.S - 5 if b % 2 == 0 else c.S + 5) for b in range(c.blocks))
        for b in range(c.blocks):                       # the branch decides membership: live slots are exactly the positive scores
            assert int((score[b] > 0).sum()) == live[b]
    if c.name.startswith("huge_flat"):
        assert float(D.float().min()) >= 29952.0
        u = torch.tensor(1.0 / c.N).bfloat16()
        assert bool((P[0::2] == u).all()), "after the maximum subtraction an all-equal row is the uniform softmax"
    if c.name.startswith("subnormal_p"):
        assert float(finv.max()) < 6.5e-4


def sequence_key_counts(seq):
    """Per step: (#keys == 0, #keys == 32767, #slots) under the previous step's log-normalisers c~ = m + ln s (0 before the first
    step), as the scan of the fused selection forms them: key(min(max_g(D_g - c~_g), -2^-12))."""
    ctil = np.zeros((seq.blocks, seq.G), dtype=np.float32)
    out = []
    for t in range(8):
        D, P, nm, sm = oracle_softmax(seq.q[t], seq.lm, seq.blocks, seq.G, seq.N, seq.alpha)
        assert_bits_equal(seq.logits[t], D, f"{seq.name} step {t}: designed logits")
        d = D.float().numpy()
        kap = (d - ctil[:, :, None]).max(axis=1)
        key = W.kappa_key(np.minimum(kap, np.float32(-2.0 ** -12)))
        out.append((int((key == 0).sum()), int((key == 32767).sum()), key.size, int(((key > 0) & (key < 32767)).sum())))
        ctil = (nm[:, 0].double() - torch.log(sm[:, 0].double())).float().numpy()
        assert np.isfinite(ctil).all()
    return out


@pytest.mark.parametrize("seq", SEQS, ids=[s.name for s in SEQS])
def test_scale_jump_sequence_reaches_both_end_keys(seq):
    counts = sequence_key_counts(seq)
    print(f"\n{seq.name}: (keys == 0, keys == 32767, slots, between) per step: {counts}")
    for t in (0, 1, 4, 6):
        assert counts[t][1] == counts[t][2], f"step {t}: every kappa >= 0 -> every key 32767"
    for t in (3, 5):
        assert counts[t][0] == counts[t][2], f"step {t}: every kappa < -128 -> every key 0"
    for t in (2, 7):
        # (at 2^118 the logits are 2^111 apart or equal: the row splits into the two end codes with nothing between)
        assert sum(n > 0 for n in (counts[t][0], counts[t][1], counts[t][3])) >= 2, f"step {t}: mixed keys"
    # step 5 inverts the ranking of step 4 (the same bank, scale -100 / -2^118): its maximum is step 4's minimum, scaled
    assert torch.equal(seq.logits[5].float().max(-1).values, (seq.logits[4].double().min(-1).values * seq.scales[5]).float().bfloat16().float())
    # step 6: the cliff's closed form through the oracle
    D, P, _, _ = oracle_softmax(seq.q[6], seq.lm, seq.blocks, seq.G, seq.N, seq.alpha)
    sel = oracle.group_max_topk(P, None, seq.blocks, seq.G, seq.N, seq.S)
    assert [sel[b].tolist() for b in range(seq.blocks)] == seq.cliff_expected
    top = float(max(l.float().abs().max() for l in seq.logits))
    assert math.isfinite(top) and (seq.scales[1] == 100.0 or top == 22.0 * W.HUGE)


def test_kappa_key_restatement():
    x = np.array([-1e30, -129.0, -128.0, -127.999, -127.99609375, -64.0, -2.0 ** -12, 0.0, 5.0, 1e30, np.nan, -np.inf, np.inf],
                 dtype=np.float32)
    assert W.kappa_key(x).tolist() == [0, 0, 0, 0, 1, 16384, 32767, 32767, 32767, 32767, 0, 0, 32767]


@pytest.mark.parametrize("kv_len,splits", [(300, 8), (2497, 32)])
@pytest.mark.parametrize("kind", ["rising", "plateau", "vmag"])
@pytest.mark.parametrize("shape", [(1, 32, 8), (1, 32, 4), (2, 16, 2)], ids=["mfma-g4", "mfma-g8", "mfma-g8-bs2"])
def test_late_maximum_inputs_keep_the_two_oracles_inside_the_error_model(shape, kind, kv_len, splits):
    """The inputs of test_gpu_wide_range_attention.py::test_late_maximum_and_dead_splits, for the bodies that round their weights
    to bf16: the oracle that rounds them where the pass does (sparse_attention_p16) against the f32-weight oracle stays inside
    the bound util.check_attention asserts between the device and the f32-weight oracle (the bf16-weight error model) - the
    gate can be met on these inputs and seeds.  The margin is printed."""
    bs, Hq, Hkv = shape
    a, v = W.late_maximum_case(kind, bs, Hkv, kv_len, splits, seed=kv_len + len(kind))
    q, k, v = W.attention_inputs(a, Hq, seed=kv_len, v=v)
    labels = standalone_pass_labels(bs, Hq, Hkv, kv_len, splits)
    assert labels is not None
    _, a32 = oracle.sparse_attention(q, k, v, kv_len, W.ATTN_SCALE)
    _, aabs = oracle.sparse_attention(q, k, v.abs(), kv_len, W.ATTN_SCALE)
    _, p16, flip = oracle.sparse_attention_p16(q, k, v, kv_len, W.ATTN_SCALE, *labels, with_flip=True)
    assert bool(torch.isfinite(a32).all()) and bool(torch.isfinite(p16).all())
    err, tol = (p16 - a32).abs(), attention_tolerance(a32, aabs)
    print(f"\n{kind} {shape} [{kv_len}-{splits}]: oracle pair max err / bound {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())
