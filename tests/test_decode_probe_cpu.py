"""CPU: the attended-row read-out of tests/decode_probe.py on a torch model of the decode attention contract (split pass with
(m, l, acc) records and combine; slot list; the overlapped form with resident splits, one record per miss tile and the merge from
t0 = cnt / 8) - the read-out returns the row set the plan attends, names eight seeded defects by (sequence, head, row, kind),
and the oracle reproduces the probe's keys bit for bit from the token-keyed factors under the identity RoPE table.  For every
seeded defect the existing gate (tests/util.check_attention, its labels) is evaluated on Gaussian inputs of the same shape:
the record is profiles/decode_attention_readout_tests.txt (PYTHONPATH=. python tests/test_decode_probe_cpu.py prints it)."""
import functools
import math

import pytest
import torch

import attn_probe as ap
import decode_probe as dp
import oracle
from util import attention_tolerance, check_attention

# the headline row layout: 448 local + outlier rows, S = 256 selected chunks, generated rows behind the region
SS, S_SEL, GEN, SLACK = 448, 256, 3, 50
G = 4
DEFECTS = ["last row of a split dropped", "first row of the next split taken twice", "row at kv_len attended",
           "hit chunks of the mixed tile attended by both sides", "miss chunks of the mixed tile attended by neither side",
           "unselected resident slot attended", "V rows swapped inside one miss tile", "one generated row skipped"]


# ------------------------------------------------------------------------------------------------ exactness facts
def test_rounding_facts():
    """The kernels divide acc / l with the f32 division HIP compiles by default (not IEEE's): every f32 within 8 ulp of
    mult / l still rounds to one bf16, and bf16(1 / l) names l."""
    assert ap.rounding_facts(128, 8) == (True, True) and ap.rounding_facts(ap.TABLE_L, 8) == (True, True)


@pytest.mark.parametrize("style", ["neox", "glm"])
def test_factors_and_identity_rope_reproduce_the_keys_bit_for_bit(style):
    """oracle.batch_gather_gemm over the token-keyed factors, then the oracle's RoPE-and-push with the identity table, writes
    exactly the probe's K rows of the gathered chunks into the cache."""
    kv, N, Cc, S = 2, 600, 8, 8
    probe = dp.TokenProbe(N, 1, bs=1, Hq=2 * kv, Hkv=kv, seed=3)
    _, k, _ = probe.inputs(0)
    U, SV = dp.token_factors(k, probe.C)
    assert torch.equal(torch.einsum("blr,bhdr->bhld", U.float(), SV.float()).bfloat16().view(torch.int16), k.view(torch.int16))
    cs = dp.identity_rope(style, N + 8)
    assert cs.shape == (N + 8, 128 if style == "neox" else 64)
    g = torch.Generator().manual_seed(1)
    ids = torch.stack([torch.randperm(N // Cc, generator=g)[:S] for _ in range(kv)]).to(torch.int32).view(1, kv, S).contiguous()
    pre = torch.zeros(1, kv, S * Cc, 128, dtype=torch.bfloat16)
    zero = torch.zeros(kv, dtype=torch.int32)
    oracle.batch_gather_gemm(U, SV, None, None, ids, pre, 1, kv, N, 128, 160, S * Cc, 0, Cc, zero)
    tok = (ids[0].long().unsqueeze(-1) * Cc + torch.arange(Cc)).view(kv, S * Cc)
    want = torch.gather(k[0], 1, tok.unsqueeze(-1).expand(-1, -1, 128))
    assert torch.equal(pre[0].view(torch.int16), want.view(torch.int16))
    start, end = 16, 16 + S * Cc
    kor = torch.full((1, kv, end + 4, 128), 3.0, dtype=torch.bfloat16)
    ints = (1, kv, S * Cc, 128, pre.stride(0), pre.stride(1), pre.stride(2), 1, cs.stride(0), ids.stride(0), ids.stride(1),
            ids.stride(2), kor.stride(0), kor.stride(1), kor.stride(2), start, end, 64, Cc)
    (oracle.apply_rotary_pos_emb_push_cache_opt_glm if style == "glm" else oracle.apply_rotary_pos_emb_push_cache_opt)(
        pre, cs, ids, kor, zero, *ints)
    assert torch.equal(kor[0, :, start:end].view(torch.int16), want.view(torch.int16))
    assert bool((kor[0, :, :start] == 3.0).all()) and bool((kor[0, :, end:] == 3.0).all())


def test_planted_landmarks_score_the_same_for_every_probed_class():
    lm = dp.planted_landmarks(456, seed=2)
    a = lm[:, 0]
    assert lm.dtype == torch.bfloat16 and a.unique().numel() == 456 and bool((lm == a.view(-1, 1)).all()) and bool((a > 0).all())
    probe = dp.TokenProbe(4192, 1, bs=1, Hq=8, Hkv=2)
    scores = [probe.inputs(s)[0][0, :, 0].float() @ lm.float().T for s in (0, 7, 32)]
    assert all(torch.equal(sc, (64.0 * a.float()).expand(8, -1)) for sc in scores)


# ------------------------------------------------------------------------------------------------ the clean families
def _check_plan(rows, plan, round_p=None, Hq=G, seed=0):
    probe = dp.model_read_out(rows, Hq, 1, [[plan]], seed=seed, round_p=round_p)
    exp = dp.plan_mask(plan, rows).view(1, 1, rows)
    return probe, exp


@pytest.mark.parametrize("kv_len,splits", [(1, 1), (1, 8), (5, 62), (17, 24), (64, 3), (129, 8), (257, 32), (1000, 62)])
def test_standalone_plan_reads_out_as_rows_below_kv_len(kv_len, splits):
    rows = kv_len + SLACK
    for n in (kv_len, rows + 1000):                               # host length; device length past the rows: the clamp
        plan = dp.standalone_plan(n, rows, splits)
        probe, exp = _check_plan(rows, plan, seed=kv_len)
        assert torch.equal(exp.flatten(), torch.arange(rows) < min(n, rows))
        dp.assert_conditions(exp, probe.C, two=min(n, rows) >= 256)
        assert dp.check(probe, exp) == G * min(n, rows)


@pytest.mark.parametrize("R,n", [(32, 1), (32, 16), (32, 32), (64, 0)])
def test_listed_plan_reads_out_as_the_listed_slots(R, n):
    g = torch.Generator().manual_seed(R + n)
    slots = torch.randperm(R, generator=g)[:n].tolist()
    kv_len = 24 + 8 * R + 5
    rows = kv_len + SLACK
    plan = dp.listed_plan(kv_len, rows, 8, slots, 24, 8 * R)
    probe, exp = _check_plan(rows, plan, seed=n)
    want = torch.zeros(rows, dtype=torch.bool)
    want[:24] = True
    want[24 + 8 * R:kv_len] = True
    for s in slots:
        want[24 + 8 * s:24 + 8 * s + 8] = True
    assert torch.equal(exp.flatten(), want)
    dp.check(probe, exp)


@pytest.mark.parametrize("cnt", [32, 31, 20, 8, 1, 0])
def test_overlapped_plan_reads_out_as_every_slot_once(cnt):
    S = 32
    g = torch.Generator().manual_seed(cnt)
    dst = torch.randperm(S, generator=g).tolist()
    kv_len = 24 + 8 * S + 3
    rows = kv_len + SLACK
    plan, rp = dp.overlapped_plan(kv_len, rows, 4, dst, cnt, 24, 8 * S)
    assert len(plan) == 4 + S // 8 - cnt // 8
    probe, exp = _check_plan(rows, plan, round_p=rp, seed=cnt)
    assert torch.equal(exp.flatten(), torch.arange(rows) < kv_len)
    assert dp.check(probe, exp) == G * kv_len


# ------------------------------------------------------------------------------------------------ seeded defects
@functools.lru_cache(maxsize=None)
def _standalone_case():
    kv_len, splits = 2499, 32
    rows = kv_len + SLACK
    return kv_len, rows, dp.standalone_plan(kv_len, rows, splits), None


@functools.lru_cache(maxsize=None)
def _overlapped_case(R=S_SEL + 32, cnt=172):
    """S = 256 of R = 288 resident slots, cnt = 172 hits (cnt % 8 = 4: tile t0 = 21 holds 4 hit and 4 miss chunks), 24 splits."""
    kv_len = SS + 8 * R + GEN
    rows = kv_len + SLACK
    g = torch.Generator().manual_seed(5)
    dst = torch.randperm(R, generator=g)[:S_SEL].tolist()
    plan, rp = dp.overlapped_plan(kv_len, rows, 24, dst, cnt, SS, 8 * R)
    return kv_len, rows, plan, rp, dst, cnt, sorted(set(range(R)) - set(dst))


def _slot_rows(s):
    return list(range(SS + 8 * s, SS + 8 * s + 8))


def _edit(plan, i, k=None, v=None):
    plan = list(plan)
    plan[i] = (list(plan[i][0]) if k is None else k, list(plan[i][1]) if v is None else v)
    return plan


@functools.lru_cache(maxsize=None)
def seeded(name):
    """-> (rows, clean plan, defective plan, round_p, {(row, kind)} the read-out must name, exact: whether it names nothing
    else, the rows the defect touches)."""
    if name in DEFECTS[:3]:
        kv_len, rows, plan, rp = _standalone_case()
        i = 7
        if name == "last row of a split dropped":
            r = plan[i][0][-1]
            return rows, plan, _edit(plan, i, plan[i][0][:-1], plan[i][1][:-1]), rp, {(r, "dropped")}, True, [r]
        if name == "first row of the next split taken twice":
            r = plan[i + 1][0][0]
            return rows, plan, _edit(plan, i, plan[i][0] + [r], plan[i][1] + [r]), rp, {(r, "multiplicity")}, True, [r]
        return rows, plan, _edit(plan, -1, plan[-1][0] + [kv_len], plan[-1][1] + [kv_len]), rp, {(kv_len, "added")}, True, [kv_len]
    kv_len, rows, plan, rp, dst, cnt, unsel = _overlapped_case()
    splits, t0 = 24, cnt // 8
    if name == "hit chunks of the mixed tile attended by both sides":
        hits = [r for j in range(8 * t0, cnt) for r in _slot_rows(dst[j])]
        bad = _edit(plan, splits, hits + plan[splits][0], hits + plan[splits][1])
        return rows, plan, bad, rp, {(r, "multiplicity") for r in hits}, True, hits
    if name == "miss chunks of the mixed tile attended by neither side":
        miss = plan[splits][0]
        return rows, plan, _edit(plan, splits, [], []), rp, {(r, "dropped") for r in miss}, True, miss
    if name == "unselected resident slot attended":
        r = _slot_rows(unsel[3])
        return rows, plan, _edit(plan, 7, plan[7][0] + r, plan[7][1] + r), rp, {(x, "added") for x in r}, True, r
    if name == "V rows swapped inside one miss tile":
        tile = plan[splits + 3][0]
        C = ap.n_classes(rows)
        a, b = [(a, b) for a in tile[:8] for b in tile[8:] if a // C != b // C][0]
        vr = [b if r == a else a if r == b else r for r in tile]
        return rows, plan, _edit(plan, splits + 3, v=vr), rp, {(a, "dropped"), (b, "dropped")}, False, [a, b]
    if name == "one generated row skipped":
        r = kv_len - 2
        i = [j for j in range(splits) if r in plan[j][0]][0]
        keep = [x for x in plan[i][0] if x != r]
        return rows, plan, _edit(plan, i, keep, keep), rp, {(r, "dropped")}, True, [r]
    raise KeyError(name)


@pytest.mark.parametrize("name", DEFECTS)
def test_seeded_defect_is_named(name):
    """The clean plan reads out as its row set; the defective plan is named by (sequence, head, row, kind) in every head of the
    group - and, where the defect changes membership alone, nothing else is named."""
    rows, plan, bad, rp, want, exact, _ = seeded(name)
    exp = dp.plan_mask(plan, rows).view(1, 1, rows)
    if name in (DEFECTS[0], DEFECTS[3]):                           # one clean read-out per family
        probe = dp.model_read_out(rows, G, 1, [[plan]], round_p=rp)
        dp.assert_conditions(exp, probe.C, two=True)
        assert dp.problems(probe, exp) == []
    got = set(dp.problems(dp.model_read_out(rows, G, 1, [[bad]], round_p=rp), exp, limit=100000))
    named = {(0, h, r, kind) for h in range(G) for r, kind in want}
    assert named <= got, sorted(named - got)[:8]
    if exact:
        assert got == named, sorted(got - named)[:8]
    else:                                                           # a V row of another token: its key shows as added / doubled
        assert all(kind in ("added", "multiplicity") for _, _, _, kind in got - named) and len(got - named) == 2 * G


# ------------------------------------------------------------------------------------------------ the existing gate
def _compact(plan, rp):
    """Row order and rounding labels of the oracle's view of a clean plan: the records' rows one after the other, the rows of a
    record that rounds its weights (a miss tile) labelled with its number."""
    order, grp = [], []
    for i, (kr, _) in enumerate(plan):
        order += kr
        grp += [i if (rp is not None and rp[i]) else -1] * len(kr)
    return order, torch.tensor(grp, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _gaussian(rows, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(1, G, 128, generator=g) * 1.5).bfloat16()
    k = torch.randn(1, 1, rows, 128, generator=g).bfloat16()
    v = torch.randn(1, 1, rows, 128, generator=g).bfloat16()
    return q, k, v


def gaussian_with_light_rows(rows, where, efolds=None):
    """Gaussian q / k / v [1, G | 1, rows, 128] whose lightest keys (smallest score, the largest over the G heads) sit at the
    rows `where`: the same rows as for every other defect, in another order.  efolds: those keys are then moved along
    -(q_0 + .. + q_G-1) until each weighs at most exp(-efolds) of the mean weight in every head (the G heads of a group share
    every row, and a Gaussian key that is light in all of them at once does not exist among 2,500)."""
    q, k, v = _gaussian(rows)
    score = (q[0].float() @ k[0, 0].float().T).amax(0)
    light = score.argsort()[:len(where)].tolist()
    a, b = [d for d in where if d not in light], [x for x in light if x not in where]
    perm = torch.arange(rows)
    perm[a], perm[b] = torch.tensor(b, dtype=torch.long), torch.tensor(a, dtype=torch.long)
    k, v = k[:, :, perm].contiguous(), v[:, :, perm].contiguous()
    if efolds is not None:
        u = q[0].float().sum(0)
        u = u / u.norm()
        base = torch.logsumexp((q[0].float() @ k[0, 0].float().T) * dp.SCALE, -1) - math.log(rows)      # log mean weight, per head
        for r in where:
            lo, hi = 0.0, 64.0
            for _ in range(30):
                t = (lo + hi) / 2
                kr = (k[0, 0, r].float() - t * u).bfloat16().float()
                ok = bool((((q[0].float() @ kr) * dp.SCALE - base) <= -efolds).all())
                lo, hi = (lo, t) if ok else (t, hi)
            k[0, 0, r] = (k[0, 0, r].float() - hi * u).bfloat16()
    return q, k, v


def tolerance_share(name, efolds=None):
    """The defect against the existing gate on Gaussian inputs of the same shape, the rows it touches holding the lightest keys
    -> (weight of the heaviest touched row as a multiple of the mean weight, share of the clean model, share of the
    defective model, the defect's own f32 error as a share of the bound, whether util.check_attention passes the defective
    output).  Shares are max |err| / attention_tolerance(ref) against the oracle check_attention compares with."""
    rows, plan, bad, rp, _, _, where = seeded(name)
    q, k, v = gaussian_with_light_rows(rows, where, efolds)
    order, grp = _compact(plan, rp)
    kc, vc = k[:, :, order].contiguous(), v[:, :, order].contiguous()
    n = len(order)
    both = sorted(set(order) | set(where))
    w = torch.softmax((q[0].float() @ k[0, 0, both].float().T) * dp.SCALE, -1).amax(0) * len(both)
    weight = float(w[[both.index(r) for r in where]].max())
    labels = None if rp is None else (grp.view(1, 1, n).contiguous(), torch.zeros(1, 1, n, dtype=torch.int32))
    if labels is None:
        _, ref = oracle.sparse_attention(q, kc, vc, n, dp.SCALE)
    else:
        _, ref = oracle.sparse_attention_p16(q, kc, vc, n, dp.SCALE, *labels)
    tol = attention_tolerance(ref)
    clean = dp.run_plan(q[0], k[0, 0], v[0, 0], plan, rp)
    c32, b32 = (dp.run_plan(q[0], k[0, 0], v[0, 0], p, rp, rounded=False) for p in (plan, bad))
    got = dp.run_plan(q[0], k[0, 0], v[0, 0], bad, rp)
    share = lambda o: float(((o.float().view(1, G, 128) - ref).abs() / tol).max())          # noqa: E731
    try:
        check_attention(f"test_decode_probe_cpu[{name}]", got.float().view(1, G, 128), q, kc, vc, n, dp.SCALE, labels)
        passes = True
    except AssertionError:
        passes = False
    return weight, share(clean), share(got), float(((b32 - c32).abs().view(1, G, 128) / tol).max()), passes


EFOLDS = 5.0


def share_table():
    head = f"{'seeded defect':58s} {'weight / mean':>13s} {'clean':>7s} {'defect':>7s} {'own f32':>8s}  existing gate"
    lines = []
    for title, ef in (("the defect at the lightest Gaussian keys of the head group", None),
                      (f"the same keys moved to exp(-{EFOLDS:g}) of the mean weight in every head", EFOLDS)):
        lines += [title, head]
        for name in DEFECTS:
            wt, c, d, own, ok = tolerance_share(name, ef)
            lines.append(f"{name:58s} {wt:13.4f} {c:7.3f} {d:7.3f} {own:8.4f}  {'passes' if ok else 'FAILS'}")
        lines.append("")
    return "\n".join(lines)


@pytest.mark.parametrize("name", DEFECTS)
def test_the_existing_gate_against_the_seeded_defect(name):
    """What the record shows (profiles/decode_attention_readout_tests.txt), on a headline-shaped attention (2,499 / 2,755 rows,
    G = 4) over Gaussian K / V.  Seeded at the lightest Gaussian keys, the gate catches every one of the eight: the four heads of
    a group share each row, so the lightest row still weighs 0.075 of the mean in one of them, and the bound is 1e-5 absolute
    where the reference is near zero.  With the same keys at exp(-5) of the mean weight in every head - a few e-folds below
    average - every one passes the gate, the single-row ones at under a third of the bound;
    the read-out names them all (test_seeded_defect_is_named)."""
    weight, clean, defect, own, passes = tolerance_share(name)
    assert clean <= 1.0 and own > 1.0 and not passes, (name, weight, clean, defect, own)
    weight, clean, defect, own, passes = tolerance_share(name, EFOLDS)
    assert weight <= math.exp(-EFOLDS) * 1.05 and clean <= 1.0 and passes, (name, weight, clean, defect, own)
    if "tile attended" not in name and "slot" not in name:          # one or two rows, not the 8 or 32 of a slot / half a tile
        assert own < 1.0 / 3 and defect <= 1.0, (name, own, defect)


if __name__ == "__main__":
    print(share_table())
