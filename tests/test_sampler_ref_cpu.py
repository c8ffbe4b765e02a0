"""tests/sampler_ref.py on its own, without a GPU: the winners against a brute-force definition, the nucleus against the
reference's filter restated in torch ops, the counter hash as a multinomial sampler (frequencies, correlations, bit balance),
and the two conditions the GPU tests lean on - MARGIN is at least 16 times the f32 evaluation's deviation from f64, and the
reference alone leaves every case of tests/test_gpu_sampler_exact.py under the undecided cap with no edge rank.  Writes
profiles/sampler_exact_margin.txt."""
import os

import numpy as np
import pytest
import torch

import sampler_cases as sc
import sampler_ref as sr

N_POS = 200_000
_RECORD = {}


# ------------------------------------------------------------------------------------------------ (a) winners, brute force
def _brute(vals, k):
    """O(V k): take the largest (lowest id first) k times -> thr; everything above, then the ties by id, 64 in all"""
    left, thr = list(range(len(vals))), None
    for _ in range(k):
        j = max(left, key=lambda i: (vals[i], -i))
        left.remove(j)
        thr = vals[j]
    gt = [i for i in range(len(vals)) if vals[i] > thr]
    eq = [i for i in range(len(vals)) if vals[i] == thr][:sr.KEEP_MAX - len(gt)]
    return sorted(gt + eq, key=lambda i: (-vals[i], i))


def _short_rows():
    g = torch.Generator().manual_seed(sc.ROW_SEED)
    ninf = float("-inf")
    for n in range(240):
        V = [8, 16, 24, 64, 72, 200, 512][n % 7]
        kind = n % 6
        x = torch.randn(V, generator=g) * 2.0
        if kind == 1:                                   # coarse values: ties everywhere, at the k-th value too
            x = torch.round(x)
        elif kind == 2:                                 # more than 64 tied at the top (where V allows)
            x[torch.randperm(V, generator=g)[:min(V - 1, 100)]] = 9.0
        elif kind == 3:
            x = torch.full((V,), -0.75 if n % 2 else 3.0)
        elif kind == 4:                                 # -inf entries, a few finite
            x[torch.randperm(V, generator=g)[:V - 3 - n % 4]] = ninf
        elif kind == 5:
            x = -x.abs() - 0.5
        x = torch.where(x == 0, torch.ones_like(x), x)   # (the keys order -0 below +0; no row of any test holds a zero)
        k = int(torch.randint(1, min(V, 64) + 1, (1,), generator=g))
        yield x.bfloat16(), k


def test_winners_against_brute_force():
    capped = 0
    for row, k in _short_rows():
        want = _brute(row.float().tolist(), k)
        got = sr.winners(row, k).tolist()
        assert got == want, (row.shape, k)
        capped += len(want) == sr.KEEP_MAX and len(want) > k
    assert capped >= 10                                  # rows whose ties run into the 64-winner limit were among them


# ------------------------------------------------------------------------------- (b) nucleus against the reference's filter
def _filter_f64(logits, top_k, top_p):
    """The reference's top-k / top-p filter on f64 logits [1, V]: topk, everything below the k-th value removed; sort, softmax,
    cumsum, the mask shifted right by one with its first place cleared, scattered back.  Returns the ids that stay."""
    x = logits.clone()
    kth = torch.topk(x, min(top_k, x.size(-1)))[0][:, [-1]]
    x[x < kth] = float("-inf")
    if top_p > 0.0:
        s, order = torch.sort(x, descending=True)
        mask = torch.cumsum(torch.softmax(s, dim=-1), dim=-1) > top_p
        mask = torch.cat((torch.zeros_like(mask[..., :1]), mask[..., :-1]), dim=-1)
        x[torch.zeros_like(mask).scatter(1, order, mask)] = float("-inf")
    return set(torch.isfinite(x[0]).nonzero().flatten().tolist())


def test_nucleus_against_the_reference_filter():
    g = torch.Generator().manual_seed(sc.ROW_SEED + 1)
    grid = torch.arange(0x3E00, 0x4200, dtype=torch.int16).view(torch.bfloat16).float()   # 1,024 distinct bf16 values in [1/8, 32):
    assert grid.unique().numel() == 1024                                                   # no tie leaves the sort order open
    checked = 0
    for n in range(300):
        V, k = [64, 300, 1024][n % 3], [1, 2, 50, 64][n % 4]
        T, top_p = [0.6, 1.0, 4.0, 0.05][n % 4 - 1], [0.9, 0.5, 0.0, 1.0, 0.3][n % 5]
        row = (grid[torch.randperm(1024, generator=g)[:V]] * [1.0, 0.25][n % 2]).bfloat16()
        ids = sr.winners(row, k)
        v = sr.scaled(row, ids, T).astype(np.float64)
        kept, edges = sr.nucleus(v, top_p)
        if edges.any():
            continue
        tp = float(np.float32(top_p))
        want = _filter_f64((row.float() / np.float32(T)).double().view(1, -1), k, tp)
        assert set(ids[kept].tolist()) == want, (n, V, k, T, top_p)
        checked += 1
    assert checked >= 270


# ------------------------------------------------------------------------------------------------------ (c) the generator
def _frequencies(v, top_p, seed, b, pos0):
    counts = np.zeros(len(v), np.int64)
    for lo in range(0, N_POS, 50_000):
        r = sr.race(v, top_p, seed, np.arange(pos0 + lo, pos0 + lo + 50_000, dtype=np.uint64), b)
        counts += np.bincount(r.rank, minlength=len(v))
    e = np.where(r.kept, np.exp(v.astype(np.float64) - v.max()), 0.0)
    return counts, e / e.sum()


def _binomial_tail(n, q, m):
    """min(P(X <= m), P(X >= m)) * 2 for X ~ Binomial(n, q) with n q < 50, summed exactly from the log pmf"""
    from math import lgamma, log, exp, log1p
    if q <= 0.0:
        return 2.0 if m == 0 else 0.0
    pmf = [exp(lgamma(n + 1) - lgamma(j + 1) - lgamma(n - j + 1) + j * log(q) + (n - j) * log1p(-q)) for j in range(0, max(m, 400) + 1)]
    lo = sum(pmf[:m + 1])
    return 2 * min(lo, 1.0 - lo + pmf[m])


@pytest.mark.parametrize("family", ["N(0,2) k50 T0.6 p0.9", "near-flat k64 T1 p0", "peaked N(0,6) k50 T2 p0"])
def test_draw_frequencies_follow_the_renormalised_nucleus(family):
    sigma, k, T, top_p = {"N": (2.0, 50, 0.6, 0.9), "n": (0.05, 64, 1.0, 0.0), "p": (6.0, 50, 2.0, 0.0)}[family[0]]
    worst, compared = 0.0, 0
    for b in range(4):
        row = sc.random_rows(32000, 16, sigma)[b]
        ids = sr.winners(row, k)
        counts, p = _frequencies(sr.scaled(row, ids, T), top_p, 1 + b * (2 ** 33 + 5), b, 10 ** 6 * b)
        assert counts[p == 0].sum() == 0
        big = N_POS * p >= 50
        z = (counts[big] - N_POS * p[big]) / np.sqrt(N_POS * p[big] * (1 - p[big]))
        # a token with fewer than 50 expected misses: the normal z is not its law, so the same two-sided level (P(|z| > 5) of a
        # normal variable) is asked of the exact binomial tail of its misses
        for i in np.nonzero(big & (N_POS * (1 - p) < 50))[0]:
            tail = _binomial_tail(N_POS, 1 - p[i], N_POS - int(counts[i]))
            z[list(np.nonzero(big)[0]).index(i)] = 0.0 if tail >= 2 * 2.8665e-7 else 99.0
        worst, compared = max([worst] + np.abs(z).tolist()), compared + int(big.sum())
    _RECORD[f"frequencies {family}"] = f"{compared} tokens with N p >= 50 over 4 rows x {N_POS} positions, max |z| {worst:.2f}"
    assert worst <= 5.0 and compared >= 20, (family, worst, compared)


def _rho(a, b):
    return float(np.corrcoef(a.ravel(), b.ravel())[0, 1])


def test_uniforms_are_uncorrelated_and_balanced():
    bound = 5.0 / np.sqrt(N_POS)
    for seed, p0 in ((1, 0), (2 ** 64 - 1, 2 ** 31 - 77), (2 ** 32 + 1, 2 ** 40)):
        pos = p0 + np.arange(N_POS, dtype=object)
        u = sr.uniforms(seed, pos, 3, [0, 1, 49, 50])
        pairs = {"neighbouring ranks": (u[:, 0], u[:, 1]), "ranks 49 / 50": (u[:, 2], u[:, 3]),
                 "neighbouring rows": (u[:, 0], sr.uniforms(seed, pos, 4, [0])[:, 0]),
                 "consecutive positions": (u[:-1, 0], u[1:, 0]),
                 "positions p, p + 2^32": (u[:, 0], sr.uniforms(seed, pos + 2 ** 32, 3, [0])[:, 0]),
                 "seeds s, s + 2^32": (u[:, 0], sr.uniforms((seed + 2 ** 32) % 2 ** 64, pos, 3, [0])[:, 0])}
        for name, (a, b) in pairs.items():
            rho = _rho(a, b)
            _RECORD[f"rho {name} (seed {seed}, from position {p0})"] = f"{rho:+.5f} (bound {bound:.5f})"
            assert abs(rho) <= bound, (name, seed, rho)
        h = sr.hash_bits(seed, pos, 3, [0, 7])
        assert float(u.min()) > 0.0 and float(u.max()) <= 1.0
        for bit in range(8, 32):                         # the 24 bits of u
            ones = ((h >> np.uint64(bit)) & np.uint64(1)).astype(np.float64).mean(0)
            assert np.all(np.abs(2 * ones - 1) <= bound), (bit, ones)


# ------------------------------------------------------------------------------------------------- (d) margin and cap
def _families():
    """(name, rows, k, T, top_p): the row families of the GPU tests"""
    yield "N(0,2) rows, k 50, T 0.6, top_p 0.9", sc.random_rows(32000, 16), 50, 0.6, 0.9
    yield "N(0,2) rows, V 151552, k 64, T 4, top_p 0", sc.random_rows(151552, 16), 64, 4.0, 0.0
    yield "N(0,2) rows, k 50, T 0.05, top_p 0.9", sc.random_rows(32000, 16), 50, 0.05, 0.9
    for V in (8000, 151552):
        rows, names = sc.content_rows(V)
        for r, name in enumerate(names):
            yield f"{name}, V {V}", rows[r:r + 1], 50, 0.6, 0.9
    yield "boundary rows, V 524288", sc.boundary_rows(524288)[0], 50, 0.6, 0.9
    yield "16 equal logits, rest -inf, k 64, T 1, top_p 0", sc.nucleus_rows(16)[0][:4], 64, 1.0, 0.0


def test_margin_covers_the_f32_evaluation_and_the_shares_stay_small():
    P = 5000
    pos = np.arange(P, dtype=np.uint64)
    triples, worst, lines = 0, 0.0, []
    for name, rows, k, T, top_p in _families():
        und = edge = 0
        for b in range(rows.shape[0]):
            ids = sr.winners(rows[b], k)
            v32 = sr.scaled(rows[b], ids, T)
            r = sr.race(v32, top_p, 1, pos, b)
            und, edge = und + int((~r.decided).sum()), edge + int(r.edges.any())
            # the kernel's formula in numpy float32 with libm exp / log
            u32 = sr.uniforms(1, pos, b, np.arange(len(ids))).astype(np.float32)
            s32 = np.exp(v32 - v32.max())[None, :] / np.maximum(-np.log(u32), np.float32(1e-30))
            v64 = v32.astype(np.float64)
            s64 = np.exp(v64 - v64.max())[None, :] / np.maximum(-np.log(u32.astype(np.float64)), 1e-30)
            ok = (r.kept & (np.exp(v64 - v64.max()) > 1e-30))[None, :] & (s64 > 0)
            worst = max(worst, float((np.abs(s32.astype(np.float64) - s64) / np.where(ok, s64, 1.0))[np.broadcast_to(ok, s64.shape)].max()))
            triples += int(np.broadcast_to(ok, s64.shape).sum())
        share = und / (P * rows.shape[0])
        lines.append(f"{name}: rows {rows.shape[0]} x {P} positions, undecided share {share:.2e}, rows with an edge rank {edge}")
        assert share <= sr.CAP / 2 and edge == 0, lines[-1]
    _RECORD["margin"] = lines + [f"f32 (numpy, libm exp / log) score against f64: {triples} (row, position, rank) triples, largest relative "
                                 f"deviation {worst:.3e}; MARGIN 2^{int(np.log2(sr.MARGIN))} = {sr.MARGIN:.3e} = {sr.MARGIN / worst:.0f} x that"]
    assert triples >= 10 ** 6
    assert sr.MARGIN >= 16 * worst, worst


def test_every_gpu_case_is_under_the_cap_without_the_kernel():
    """The draws the GPU tests will ask for, predicted here: no case can miss the cap or meet an edge rank because of the
    reference or its rows."""
    total = und = 0
    per_family = {}
    for case in sc.all_gpu_cases():
        pred = sc.predict(case)
        assert pred.undecided <= sr.CAP * pred.tokens.size, (str(case), pred.undecided, pred.tokens.size)
        assert not pred.edge_rows, (str(case), pred.edge_rows)
        assert all(pred.tokens[l, b] in a for (l, b), a in pred.allowed.items())
        if case.ranges and "fallback" not in str(case):      # the range rows: the last range's leader and several other tokens
            V = case.rows().shape[1]
            for b in range(pred.tokens.shape[1]):
                want = pred.tokens[:, b]
                assert (want >= V - 16).any() and len(set(want[want < V - 16].tolist())) >= 4, (str(case), b)
        for row, ids in case.planted or []:
            assert set(ids) <= set(pred.tokens[:, row].tolist()), (str(case), row)
        f = per_family.setdefault(case.family, [0, 0, 0])
        f[0], f[1], f[2] = f[0] + 1, f[1] + pred.tokens.size, f[2] + pred.undecided
    for variant in sc.sorted_variants():
        pred = sc.predict_sorted_variant(*variant)[-1]
        assert pred.undecided <= sr.CAP * pred.tokens.size, (variant, pred.undecided)
        f = per_family.setdefault("skv_sample_advance", [0, 0, 0])
        f[0], f[1], f[2] = f[0] + 1, f[1] + pred.tokens.size, f[2] + pred.undecided
    _RECORD["cases"] = [f"{name}: {c} cases, {d} draws, {u} undecided, no edge rank" for name, (c, d, u) in per_family.items()]


def test_advance_counters():
    a = sr.advance([10, 20], 93, 5, 2496, 96, 7, launches=3)
    assert a == dict(pos=[13, 23], gen=96, row_idx=2496 + 0, kv_len=2496 + 96, step_idx=1)
    a = sr.advance([0], 10, None, 2496, 96, 7)
    assert a == dict(pos=[1], gen=11, row_idx=2496 + 11, kv_len=2496 + 12, step_idx=None)


@pytest.fixture(scope="module", autouse=True)
def margin_record():
    """After the last test of the file: what the tests measured, as profiles/sampler_exact_margin.txt (whole-file runs only)."""
    yield
    if not {"margin", "cases"} <= set(_RECORD):
        return
    out = ["tests/test_sampler_ref_cpu.py: the sampler reference on its own (no GPU)", ""]
    out += _RECORD["margin"] + [""] + ["the cases of tests/test_gpu_sampler_exact.py, predicted without the kernel:"] + _RECORD["cases"] + [""]
    out += [f"{k}: {v}" for k, v in _RECORD.items() if k not in ("margin", "cases")]
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sampler_exact_margin.txt")
    try:
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")
    except OSError:
        pass                                             # a read-only checkout: the assertions above are the test
