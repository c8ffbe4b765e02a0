"""CPU reference of the sampler (shadowkv_amd/csrc/skv_sample.hip): every single draw predicted, in f64, from the contract alone.

The contract (header comments of skv_sample.hip; the reference's top-k / top-p filter):
  * thr = the k-th largest logit of the row; the winners are every id with a logit > thr plus the ids with a logit == thr in
    ascending id order, KEEP_MAX winners in all at most, ordered by (value descending, id ascending);
  * v = f32(logit) / f32(temperature); p = softmax(v) over the winners; rank i stays iff i == 0 or top_p <= 0 or
    cumsum(p)[i - 1] <= top_p (the EXCLUSIVE sum);
  * u(seed, position, batch row, rank) is a counter-based hash, 24 bits, exact in f32; the token is argmax_i p_i / -ln u_i.
So a draw is a pure function of (row, k, temperature, top_p, seed, position, batch row), and the CPU can name the token the
kernel must return - unless the two best scores lie closer than the kernel's f32 arithmetic resolves (MARGIN) or a nucleus
decision sits on the f32 scan's rounding (EDGE).  Such draws are `undecided`: the kernel may return any token of `allowed`,
and at most CAP of a case's draws may be undecided.  

No value here comes from a kernel, and nothing mirrors the kernel's parts, prefilter or histogram.  The rows and cases of the
GPU tests live in tests/sampler_cases.py."""
from dataclasses import dataclass

import numpy as np
import torch

from dense_ref import order_keys

MARGIN = 2.0 ** -10     # relative gap of the two best scores below which a draw is undecided (set as DESIGN.md 4.4 describes)
EDGE = 2.0 ** -14       # |cumsum(p)[i - 1] - top_p| below which rank i's nucleus decision is an edge
CAP = 0.005             # largest undecided share of a case's draws
KEEP_MAX = 64           # winners a row hands to the draw (SMP_KEEP)


# ------------------------------------------------------------------------------------------------------------- the contract
def _sorted_top(row_bf16):
    """One stable sort of the row by (value descending, id ascending): (ids, keys) of its first KEEP_MAX places."""
    keys = order_keys(row_bf16.reshape(-1)).numpy().astype(np.uint16)
    order = np.argsort((0xFFFF - keys).astype(np.uint16), kind="stable")[:KEEP_MAX]
    return order.astype(np.int64), keys[order].astype(np.int64)


def _cut(order, skeys, k):
    thr = skeys[k - 1]                                   # the k-th largest value
    return order[:int((skeys >= thr).sum())]             # everything above it, then the ties in id order, KEEP_MAX at most


def winners(row_bf16, k):
    """Token ids int64 [n] of the winners of a bf16 row, ordered by (value descending, id ascending); k <= n <= KEEP_MAX."""
    assert 1 <= k <= KEEP_MAX and k <= row_bf16.numel()
    return _cut(*_sorted_top(row_bf16), k)


def nucleus(vals_f64, top_p, edge=EDGE):
    """(kept, edges): bool [n] each.  vals descending; top_p as the kernel gets it (an f32)."""
    v = np.asarray(vals_f64, dtype=np.float64)
    n = v.shape[0]
    kept, edges = np.ones(n, bool), np.zeros(n, bool)
    tp = float(np.float32(top_p))
    if tp <= 0.0:
        return kept, edges
    e = np.exp(v - v.max())
    before = (np.cumsum(e / e.sum()))[:-1]               # cumsum(p)[i - 1] for i = 1 ..
    kept[1:] = before <= tp
    edges[1:] = np.abs(before - tp) < edge
    return kept, edges


_M32 = np.uint64(0xFFFFFFFF)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def _mix32(x):
    """lowbias32 finaliser on uint64 arrays that hold 32-bit values"""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def hash_bits(seed, pos, b, ranks):
    """The 32-bit hash h [P, n] of (seed, position, batch row, rank); u uses its upper 24 bits."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    pos = _u64([int(p) & 0xFFFFFFFFFFFFFFFF for p in np.atleast_1d(pos).tolist()])
    ranks = _u64(np.atleast_1d(ranks))
    s_lo, s_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    p_lo, p_hi = pos & _M32, pos >> np.uint64(32)
    h = _mix32(s_lo ^ _mix32((s_hi + ((np.uint64(0x9E3779B9) * p_lo) & _M32)) & _M32))
    row = np.uint64((0x85EBCA6B * (int(b) + 1)) & 0xFFFFFFFF)
    lane = (np.uint64(0xC2B2AE35) * (ranks + np.uint64(1))) & _M32
    return _mix32(h[:, None] ^ row ^ lane[None, :] ^ p_hi[:, None])


def uniforms(seed, pos, b, ranks):
    """u in (0, 1], f64 [P, n]: ((h >> 8) + 1) / 2^24"""
    return ((hash_bits(seed, pos, b, ranks) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) / 16777216.0


@dataclass
class Race:
    rank: np.ndarray        # [P] the winner's rank
    decided: np.ndarray     # [P] bool
    allowed: np.ndarray     # [P, n] bool: ranks the kernel may return
    ratio: np.ndarray       # [P] best / second-best score among the kept ranks (inf with one kept rank)
    kept: np.ndarray        # [n]
    edges: np.ndarray       # [n]


def race(v_f32, top_p, seed, pos, b, edge=EDGE, margin=MARGIN):
    """The exponential race over the winners' v = logit / temperature (f32 values, descending) at every position of `pos`."""
    v = np.asarray(v_f32, dtype=np.float32).astype(np.float64)
    n = v.shape[0]
    kept, edges = nucleus(v, top_p, edge)
    e = np.exp(v - v.max())
    u = uniforms(seed, pos, b, np.arange(n))
    score = e[None, :] / np.maximum(-np.log(u), 1e-30)
    ks = np.where(kept[None, :], score, -1.0)
    rank = ks.argmax(1)
    top2 = -np.partition(-ks, 1, axis=1)[:, :2] if n > 1 else np.concatenate([ks, -np.ones_like(ks)], 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(top2[:, 1] > 0, top2[:, 0] / top2[:, 1], np.inf)
    # a rank may be returned if it is kept under some resolution of the edge ranks and its score is within the margin of the
    # best score of the ranks that are kept under every resolution
    sure = kept & ~edges
    best_sure = np.where(sure[None, :], score, -1.0).max(1)
    allowed = (sure | edges)[None, :] & (score * (1.0 + margin) >= best_sure[:, None])
    return Race(rank, allowed.sum(1) == 1, allowed, ratio, kept, edges)


def scaled(row_bf16, ids, temperature):
    """v = f32(logit) / f32(temperature): one f32 division, as the kernel does it"""
    return row_bf16.reshape(-1)[torch.as_tensor(ids)].float().numpy() / np.float32(temperature)


def _one(r, ids):
    return int(ids[r.rank[0]]), bool(r.decided[0]), {int(t) for t in np.asarray(ids)[r.allowed[0]]}


def draw(row_bf16, k, temperature, top_p, seed, pos, b, edge=EDGE):
    """(token, decided, allowed) of one draw of skv_sample_topk_advance from a bf16 row."""
    ids = winners(row_bf16, k)
    return _one(race(scaled(row_bf16, ids, temperature), top_p, seed, [pos], b, edge), ids)


def draw_sorted(vals_f32, idx, top_p, seed, pos, b, edge=EDGE):
    """(token, decided, allowed) of one draw of skv_sample_advance: the top-k is given (values sorted descending, their ids)."""
    return _one(race(vals_f32, top_p, seed, [pos], b, edge), np.asarray(idx))


def advance(pos, gen, step, base, slack, table_len, launches=1):
    """The five counters after `launches` launches, in plain integers.  pos: list per batch row; step None: no table."""
    pos = [int(p) for p in pos]
    row_idx = kv_len = None
    for _ in range(launches):
        pos = [p + 1 for p in pos]
        gen += 1
        row_idx = base + gen % slack
        kv_len = base + min(gen + 1, slack)
        if step is not None:
            step = (step + 1) % table_len
    return dict(pos=pos, gen=gen, row_idx=row_idx, kv_len=kv_len, step_idx=step)
