"""Rows and cases of tests/test_gpu_sampler_exact.py, and the prediction of a whole case by tests/sampler_ref.py.  They live
apart from the test so that tests/test_sampler_ref_cpu.py can check, without a GPU, that the reference alone leaves every one
of those cases under the undecided cap and meets no edge rank.  Every row comes from ROW_SEED; builders are cached and their
tensors are never modified."""
import functools
from dataclasses import dataclass, field
from typing import Callable

import numpy as np
import torch

from dense_ref import order_keys
from sampler_ref import EDGE, _cut, _sorted_top, nucleus, race, scaled

ROW_SEED = 20261017     # every row of the GPU tests is generated from this

# the launcher's documented arithmetic (sample_topk_advance in skv_sample.hip)
THREADS = 1024
PART_MAX = THREADS * 16 * 8          # 131,072 logits one pass holds in registers
MAX_PARTS = 4
SMP_CAND = 2 * THREADS               # candidates the exact search takes


def launch_path(V):
    """(SEGV, parts, part_len) the launcher reaches for a row of V logits."""
    parts = -(-V // PART_MAX)
    part_len = (-(-V // parts) + 7) & ~7
    per_thread = -(-(part_len // 8) // THREADS)
    segv = next(s for s in (1, 2, 4, 8, 16) if per_thread <= s)
    return segv, parts, part_len


# ------------------------------------------------------------------------------------------------------------------ rows
def _g(*tag):
    """A generator seeded from ROW_SEED and the integers of `tag`"""
    seed = ROW_SEED
    for t in tag:
        seed = (seed * 1000003 + int(t)) % (2 ** 62)
    return torch.Generator().manual_seed(seed)


# (k, T, top_p) of every case that reads rows with a nucleus: the parameter axes of 2b / 2f around the default
NUCLEUS_COMBOS = [(k, 0.6, 0.9) for k in (1, 2, 49, 50, 63, 64)] + [(50, t, 0.9) for t in (0.05, 1.0, 4.0)] + [(50, 0.6, 0.5), (50, 0.6, 1.0)]


def edge_free(row, combos=NUCLEUS_COMBOS):
    """No rank of the row's winners has a nucleus decision within EDGE of top_p, for any of the combinations."""
    top = _sorted_top(row)
    return not any(nucleus(scaled(row, _cut(*top, min(k, row.numel())), T).astype(np.float64), tp)[1].any() for k, T, tp in combos)


@functools.lru_cache(maxsize=6)
def random_rows(V, bs, sigma=2.0, tag=0):
    """bf16 [bs, V], N(0, sigma^2).  A row on which some case would meet an edge rank (about 3 % of random rows: a partial sum
    within 2^-14 of top_p) is drawn again from the generator, so that no case depends on the edge allowance."""
    g = _g(V, bs, int(sigma * 16), tag)
    rows = (torch.randn(bs, V, generator=g) * sigma).bfloat16()
    for b in range(bs):
        while not edge_free(rows[b]):
            rows[b] = (torch.randn(V, generator=g) * sigma).bfloat16()
    return rows


def kept_ranks(row, k, T=0.6, top_p=0.9):
    """Ranks of the row's winners that the nucleus keeps"""
    return int(nucleus(scaled(row, _cut(*_sorted_top(row), k), T).astype(np.float64), top_p)[0].sum())


def _edge_free_set(build, combos=((50, 0.6, 0.9),), min_kept=1):
    """build(tag) for the first tag whose rows are all edge-free (and keep at least min_kept ranks in the nucleus)"""
    for tag in range(100, 228):
        rows = build(tag)
        if all(edge_free(r, combos) and all(kept_ranks(r, *c) >= min_kept for c in combos) for r in rows):
            return rows
    raise AssertionError("no edge-free row set")


def boundary_ids(V):
    """First and last ids, the 8-logit vector boundary, and both sides of every part boundary."""
    _, parts, part_len = launch_path(V)
    ids = [0, 7, 8, V - 8, V - 1]
    for p in range(1, parts):
        ids += [p * part_len - 1, p * part_len]
    return sorted(set(ids))


def boundary_rows(V):
    """(rows bf16 [m, V], planted [m] lists): the boundary ids, at most 8 per row, planted 6 above the row's maximum with one
    value.  m equal logits of p = 1 / m each lie in the 0.9 nucleus iff (m - 1) / m <= 0.9, so 8 is the most a row can carry
    with every one kept; at T = 0.6 the rest of the row shares exp(-10) of the mass: every planted id has p > 12 %."""
    ids = boundary_ids(V)
    m = -(-len(ids) // 8)
    groups = [ids[i::m] for i in range(m)]
    def build(tag):
        rows = random_rows(V, m, 2.0, tag=tag).clone()
        for r, g in enumerate(groups):
            rows[r, g] = (rows[r].float().max() + 6.0).bfloat16()
        return rows

    return _edge_free_set(build), groups


def _spread(V, n, phase=0):
    """n distinct ids spread over the whole row (every part gets its share)"""
    return (torch.arange(n, dtype=torch.int64) * V // n + phase) % V


@functools.lru_cache(maxsize=4)
def content_rows(V):
    """The rows of 2c, bf16 [7, V], and their names."""
    _, parts, part_len = launch_path(V)
    segv = launch_path(V)[0]
    base = random_rows(V, 7, 0.5, tag=2).clone()                          # |x| < 3 everywhere
    assert float(base.float().abs().max()) < 3.5
    rows, names = [], []
    names.append("all negative")
    rows.append((-random_rows(V, 1, 2.0, tag=3)[0].float().abs() - 3.0).bfloat16())
    names.append("all equal")
    rows.append(torch.full((V,), -1.25).bfloat16())
    names.append("one dominant")
    r = random_rows(V, 1, 2.0, tag=4)[0].clone()
    r[V // 3] = (r.float().max() + 12.0).bfloat16()
    rows.append(r)
    names.append("3 finite")
    r = torch.full((V,), float("-inf")).bfloat16()
    r[torch.tensor([5, V // 2 + 1, V - 2])] = torch.tensor([1.5, 2.0, 1.0]).bfloat16()
    rows.append(r)
    # leaders: 40 distinct values one bf16 step (2^-5 in [4, 8)) apart above the tied value 5.0
    lead = 5.0 + (1 + torch.arange(40)) * 2.0 ** -5
    for name, ties in (("40 leaders 20 tied", 20), ("40 leaders 54 tied", 54)):
        r = base[len(rows)].clone()
        r[_spread(V, 40) // 2 * 2] = lead[torch.randperm(40, generator=_g(V, 40))].bfloat16()
        r[_spread(V, ties, 10) // 2 * 2 + 1] = 5.0                           # (leaders on even ids, ties on odd ones)
        assert int((r.float() >= 5.0).sum()) == 40 + ties
        names.append(name)
        rows.append(r)
    # 50 leaders in consecutive ids from the start of one thread's register slice (8 * SEGV logits; fewer than 50 threads hold a
    # leader), and 3,000 logits per part tied just below them: the 50th per-thread maximum is the tied value, so the prefilter's
    # candidates are the 3,000 + the part's leaders > SMP_CAND = 2 * 1,024 in EVERY part: the all-slots path runs with a real
    # threshold.  (3,000 in all would leave each of two parts under SMP_CAND.)
    r = base[len(rows)].clone()
    assert 3000 > SMP_CAND and 3000 * parts + 50 <= V // 2
    tied = _spread(V, 3000 * parts, 1)
    r[tied] = 4.0
    s0 = (part_len // 2) // (8 * segv) * (8 * segv)                       # a slice start inside part 0
    r[s0:s0 + 50] = (4.0 + (1 + torch.randperm(50, generator=_g(V, 50))) * 2.0 ** -5).bfloat16()
    names.append("50 leaders in one slice, 3000 tied below")
    rows.append(r)
    return torch.stack(rows), names


def range_keys(rows):
    """int32 [bs, V // 16]: what the lm_head launch leaves, from dense_ref's key function (never from the GEMV)"""
    bs, V = rows.shape
    return order_keys(rows.reshape(-1)).view(bs, V // 16, 16).max(-1).values


@functools.lru_cache(maxsize=4)
def range_rows(V):
    """Rows of 2d: random N(0, 2) with a logit planted in the LAST range that ties with the row's maximum: it shares the first
    two ranks (the id decides which), takes a quarter of the draws or so, and the 0.9 nucleus keeps dozens of ranks from ranges
    all over the row - their order, the merge, the nucleus and the hash all decide tokens on this path."""
    def build(tag):
        rows = random_rows(V, 8, 2.0, tag=tag).clone()
        for r in range(rows.shape[0]):
            rows[r, V - 1 - (r % 16)] = rows[r].float().max().bfloat16()
        return rows

    return _edge_free_set(build, ((64 if V == 1024 else 50, 0.6, 0.9),), min_kept=10)      # (a row with a lone peak keeps 2 or 3)


@functools.lru_cache(maxsize=2)
def many_ranges_rows(V=128256):
    """'300 tied at the top' and 'every 7th tied' of test_lm_head_range_maxima_and_the_sampler_that_reads_them: more than
    SMP_CAND / 16 = 128 ranges reach the k-th range maximum, the kernel falls back to streaming the row."""
    def build(tag):
        base = random_rows(V, 2, 2.0, tag=tag).clone()
        base[0, torch.randperm(V, generator=_g(V, 300))[:300]] = (base[0].float().max() + 1.0).bfloat16()
        base[1, ::7] = (base[1].float().max() + 0.5).bfloat16()
        return base

    return _edge_free_set(build, [(k, 0.6, 0.9) for k in (1, 50, 64)])


@functools.lru_cache(maxsize=8)
def nucleus_rows(n, V=4096, bs=64):
    """2e: n equal finite logits (ids differ per row), every other logit -inf"""
    rows = torch.full((bs, V), float("-inf")).bfloat16()
    ids = []
    for b in range(bs):
        i = torch.randperm(V, generator=_g(V, n, b))[:n].sort().values
        rows[b, i] = 2.5
        ids.append(i.tolist())
    return rows, ids


# -------------------------------------------------------------------------------------------------- cases of the GPU tests
@dataclass
class Case:
    name: str
    rows: Callable            # () -> bf16 [bs, V] (cached builders above; never modified)
    k: int = 50
    T: float = 0.6
    top_p: float = 0.9
    seed: int = 1
    pos0: int = 0             # row b starts at pos0 + b * pos_stride
    pos_stride: int = 1
    L: int = 24
    ranges: bool = False
    edge: float = EDGE
    family: str = ""
    planted: list = field(default_factory=list)     # [(row, ids that must be drawn)]
    with_step: bool = True    # a step table is passed (step_idx is nullable)
    keep: int = 0             # 2e: ranks the nucleus keeps

    def __str__(self):
        return self.name


def _with_boundary(V):
    rows, groups = boundary_rows(V)
    return torch.cat([random_rows(V, 16), rows]), [(16 + i, g) for i, g in enumerate(groups)]


SHAPES_2A = [64, 72, 8000, 8192, 8200, 16384, 32000, 64000, 65536, 128256, 131072, 131080, 151552, 262152, 393224, 524288]


def shape_case(V):
    rows, planted = _with_boundary(V)
    return Case(f"V{V}", lambda: rows, L=32, family="N(0,2) k50 T0.6 p0.9", planted=planted)


# One axis at a time around the default (k 50, T 0.6, top_p 0.9, bs 16, seed 1, position 0), the default itself once, and the
# corners (k = 64 with T = 4 and top_p = 0; k = 1 at every T - T = 0.6 is the k axis' own k = 1).  The positions cross both word
# boundaries during the launches.
PARAM_VARIANTS = ([{}] + [dict(k=k) for k in (1, 2, 49, 63, 64)] + [dict(T=t) for t in (0.05, 1.0, 4.0)]
                  + [dict(top_p=p) for p in (0.0, 0.5, 1.0)] + [dict(bs=b) for b in (1, 3, 64)]
                  + [dict(seed=s) for s in (2 ** 32 + 1, 2 ** 64 - 1)] + [dict(pos0=p) for p in (2 ** 31 - 3, 2 ** 32 - 3, 2 ** 40 + 5)]
                  + [dict(k=64, T=4.0, top_p=0.0)] + [dict(k=1, T=t) for t in (0.05, 1.0, 4.0)])


def variant_name(var):
    return "-".join(f"{a}{b}" for a, b in var.items()) or "default"


def param_case(V, var):
    c = dict(dict(k=50, T=0.6, top_p=0.9, bs=16, seed=1, pos0=0), **var)
    bs = c.pop("bs")
    return Case(f"V{V}-{variant_name(var)}", functools.partial(random_rows, V, bs), L=40, family="parameters",
                with_step=c["k"] != 49, **c)                # (one case of each V runs without a step table)


def param_cases():
    return [param_case(V, var) for V in (32000, 151552) for var in PARAM_VARIANTS]


def content_cases(V):
    rows, names = content_rows(V)
    return Case(f"V{V}-contents", lambda: rows, L=40, family="row contents"), names


def range_cases():
    out = [Case(f"ranges-V{V}", functools.partial(range_rows, V), ranges=True, L=40, family="ranges")
           for V in (16 * (8 * 25 + r) for r in (0, 1, 3, 7))]
    out.append(Case("ranges-V1024-k64", functools.partial(range_rows, 1024), k=64, ranges=True, L=40, family="ranges"))
    out.append(Case("ranges-V262144", functools.partial(range_rows, 262144), ranges=True, L=40, family="ranges"))
    for k in (1, 50, 64):
        out.append(Case(f"ranges-fallback-k{k}", many_ranges_rows, k=k, ranges=True, L=40, family="ranges"))
    return out


@dataclass
class Prediction:
    tokens: np.ndarray      # [L, bs]
    decided: np.ndarray     # [L, bs]
    allowed: dict           # (l, b) -> set of token ids, for the undecided draws
    ratio: np.ndarray       # [L, bs] best / second
    edge_rows: list         # rows with an edge rank
    winners: list           # per row: ids

    @property
    def undecided(self):
        return int((~self.decided).sum())


def predict(case, rows=None):
    rows = case.rows() if rows is None else rows
    bs = rows.shape[0]
    tokens, decided = np.zeros((case.L, bs), np.int64), np.zeros((case.L, bs), bool)
    ratio, allowed, edge_rows, win = np.zeros((case.L, bs)), {}, [], []
    for b in range(bs):
        ids = _cut(*_top_of(rows, b), case.k)
        r = race(scaled(rows[b], ids, case.T), case.top_p, case.seed, case.pos0 + b * case.pos_stride + np.arange(case.L, dtype=object), b, case.edge)
        tokens[:, b], decided[:, b], ratio[:, b] = ids[r.rank], r.decided, r.ratio
        for l in np.nonzero(~r.decided)[0]:
            allowed[(int(l), b)] = {int(t) for t in ids[r.allowed[l]]}
        if r.edges.any():
            edge_rows.append(b)
        win.append(ids)
    return Prediction(tokens, decided, allowed, ratio, edge_rows, win)


_TOP_CACHE = {}


def _top_of(rows, b):
    """_sorted_top of rows[b], remembered per row tensor (the parameter cases share rows; the sort does not depend on k)"""
    key = (id(rows), b)                                  # (the entry holds the tensor, so its id stays its own)
    hit = _TOP_CACHE.get(key)
    if hit is None:
        if len(_TOP_CACHE) > 512:
            _TOP_CACHE.clear()
        hit = (rows, _sorted_top(rows[b]))
        _TOP_CACHE[key] = hit
    return hit[1]


def predict_sorted(vals_f32, idx, top_p, seed, pos0, L, edge=EDGE):
    """As predict for skv_sample_advance: vals f32 [bs, k] sorted descending, idx int64 [bs, k]; row b starts at pos0[b]."""
    bs = vals_f32.shape[0]
    tokens, decided, allowed = np.zeros((L, bs), np.int64), np.zeros((L, bs), bool), {}
    ratio = np.zeros((L, bs))
    for b in range(bs):
        ids = np.asarray(idx[b])
        r = race(vals_f32[b], top_p, seed, int(pos0[b]) + np.arange(L, dtype=object), b, edge)
        tokens[:, b], decided[:, b], ratio[:, b] = ids[r.rank], r.decided, r.ratio
        for l in np.nonzero(~r.decided)[0]:
            allowed[(int(l), b)] = {int(t) for t in ids[r.allowed[l]]}
    return Prediction(tokens, decided, allowed, ratio, [], [])


def sorted_inputs(k, bs, T=0.6):
    """Inputs of skv_sample_advance (2f): (vals f32 [bs, k] = the k largest logits of random rows / T, sorted; idx int64 [bs, k])"""
    rows = random_rows(32000, bs)
    idx = np.stack([_top_of(rows, b)[0][:k] for b in range(bs)])
    vals = np.stack([scaled(rows[b], idx[b], T) for b in range(bs)])
    return vals, idx + 1000 * np.arange(bs)[:, None]


def sorted_variants():
    """(k, bs, L, T / top_p / seed / pos0 as keywords) of every skv_sample_advance case: k x bs, then at k 50 / bs 16 the default,
    the T, top_p, seed and position variants of 2b and its corners; row b starts at pos0 + 3 b"""
    out = [(k, bs, 40 if bs < 64 else 24, {}) for k in (1, 50, 64) for bs in (1, 3, 64)]
    for var in PARAM_VARIANTS:
        if "bs" not in var and set(var) != {"k"}:
            var = dict(var)
            out.append((var.pop("k", 50), 16, 40, var))
    return out


def sorted_name(variant):
    return f"k{variant[0]}-bs{variant[1]}-{variant_name(variant[3])}"


def predict_sorted_variant(k, bs, L, var):
    var = dict(dict(T=0.6, top_p=0.9, seed=1, pos0=0), **var)
    vals, idx = sorted_inputs(k, bs, var["T"])
    pos0 = [var["pos0"] + 3 * b for b in range(bs)]
    return vals, idx, pos0, var, predict_sorted(vals, idx, var["top_p"], var["seed"], pos0, L)


def all_gpu_cases():
    """Every Case of tests/test_gpu_sampler_exact.py that is fixed before the GPU runs (2a - 2e)."""
    for V in SHAPES_2A:
        yield shape_case(V)
    yield from param_cases()
    for V in (8000, 128256, 151552):
        yield content_cases(V)[0]
    yield from range_cases()
    for n in (4, 8, 16):
        yield from nucleus_cases(n)


def nucleus_cases(n):
    """2e: (case, ranks kept) for top_p = j / n (keeps j + 1) and j / n - 2^-20 (keeps j); no edge allowance"""
    rows, _ = nucleus_rows(n)
    for j in range(1, n):
        for top_p, keep in ((j / n, j + 1), (j / n - 2.0 ** -20, j)):
            yield Case(f"nucleus-n{n}-j{j}-keep{keep}", lambda: rows, k=64, T=1.0, top_p=top_p, L=16, edge=0.0, family="nucleus",
                       keep=keep)
