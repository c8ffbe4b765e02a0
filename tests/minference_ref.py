"""PyTorch restatements of the MInference vertical + slash contract that the tests check the kernels
against: the window mask (vectorised and brute force), the index estimate and the masked attention in f64."""
import math

import torch

BLOCK = 64


def _members(idx, L):
    """An index list (any order, duplicates) -> the sorted set of its entries in [0, L)."""
    return sorted({int(x) for x in torch.as_tensor(idx).flatten().tolist() if 0 <= int(x) < L})


def block_coverage(L, slash, blocks=None):
    """bool [n_blk, L] (or [len(blocks), L]): key j lies in a window of block b (offsets s < e_b, e_b = 64 (b + 1), window
    [max(e_b - s, 64) - 64, max(e_b - s, 64)))."""
    if blocks is None:
        blocks = torch.arange((L + BLOCK - 1) // BLOCK, dtype=torch.int64)
    blocks = torch.as_tensor(blocks, dtype=torch.int64)
    n_blk = blocks.numel()
    s = torch.tensor(_members(slash, L), dtype=torch.int64)
    e = BLOCK * (blocks + 1)
    diff = torch.zeros(n_blk, L + BLOCK + 1, dtype=torch.int64)
    if s.numel():
        hi = torch.clamp(e.view(-1, 1) - s.view(1, -1), min=BLOCK)              # [n_blk, n_s]
        on = (s.view(1, -1) < e.view(-1, 1)).long()
        diff.scatter_add_(1, hi - BLOCK, on)
        diff.scatter_add_(1, hi, -on)
    return diff.cumsum(1)[:, :L] > 0


def window_mask(L, vertical, slash, rows=None):
    """bool [len(rows), L]: row i attends key j iff j <= i and (j in a window of block i // 64 or j a vertical column)."""
    rows = torch.arange(L) if rows is None else torch.as_tensor(rows, dtype=torch.int64).cpu()
    blocks, where = torch.unique(rows // BLOCK, return_inverse=True)
    cov = block_coverage(L, slash, blocks)
    vert = torch.zeros(L, dtype=torch.bool)
    v = _members(vertical, L)
    if v:
        vert[torch.tensor(v)] = True
    keys = torch.arange(L)
    return (cov[where] | vert.view(1, -1)) & (keys.view(1, -1) <= rows.view(-1, 1))


def brute_mask(L, vertical, slash):
    """The same mask, one (i, j) at a time, straight from the definition."""
    vs, ss = set(_members(vertical, L)), set(_members(slash, L))
    out = torch.zeros(L, L, dtype=torch.bool)
    for i in range(L):
        e = BLOCK * (i // BLOCK + 1)
        for j in range(i + 1):
            hit = j in vs
            if not hit:
                for s in ss:
                    if s < e:
                        hi = max(e - s, BLOCK)
                        if hi - BLOCK <= j < hi:
                            hit = True
                            break
            out[i, j] = hit
    return out


def attention_ref(q, k, v, vertical, slash, rows=None):
    """f64 (out [bs, n, Hq, D], absv [bs, n, Hq, D]) of softmax(q.k / sqrt(D)) over the masked keys; vertical / slash
    [bs, Hq, n] lists.  A row with no key is 0."""
    bs, Hq, L, D = q.shape
    G = Hq // k.shape[1]
    rows = torch.arange(L) if rows is None else torch.as_tensor(rows, dtype=torch.int64).cpu()
    out = torch.zeros(bs, rows.numel(), Hq, D, dtype=torch.float64, device=q.device)
    absv = torch.zeros_like(out)
    for b in range(bs):
        for h in range(Hq):
            mask = window_mask(L, vertical[b, h].cpu(), slash[b, h].cpu(), rows).to(q.device)
            kh, vh = k[b, h // G].double(), v[b, h // G].double()
            s = (q[b, h, rows.to(q.device)].double() @ kh.T) / math.sqrt(D)
            s.masked_fill_(~mask, float("-inf"))
            p = torch.softmax(s, dim=-1).nan_to_num(0.0)
            out[b, :, h] = p @ vh
            absv[b, :, h] = p @ vh.abs()
            del s, p, mask
    return out, absv


def scores_ref(q, k):
    """f64 (c, d) [bs, Hq, L] of the estimate: A = q_r . k_j (no scale) for the last m = min(64, L) rows, causal, softmax
    over j; c[j] = sum_r P[r, j] (+inf for j < 30), d[s] = sum_r P[r, r - s] (+inf for s < 100)."""
    bs, Hq, L, D = q.shape
    G = Hq // k.shape[1]
    m = min(64, L)
    r = torch.arange(L - m, L, device=q.device)
    j = torch.arange(L, device=q.device)
    c = torch.empty(bs, Hq, L, dtype=torch.float64, device=q.device)
    d = torch.empty_like(c)
    for b in range(bs):
        for h in range(Hq):
            a = q[b, h, L - m:].double() @ k[b, h // G].double().T                   # [m, L]
            a.masked_fill_(j.view(1, -1) > r.view(-1, 1), float("-inf"))
            p = torch.softmax(a, dim=-1)
            c[b, h] = p.sum(0)
            s = r.view(-1, 1) - j.view(1, -1)                                         # offset of (r, j)
            dd = torch.zeros(L, dtype=torch.float64, device=q.device)
            ok = s >= 0
            dd.index_add_(0, s[ok], p[ok])
            d[b, h] = dd
    c[..., :30] = float("inf")
    d[..., :100] = float("inf")
    return c, d


def check_topk_sets(score_ref, got_idx, count, what="", rel=1e-4):
    """got_idx: the kept indices of one head (padding >= L dropped); count: how many the contract keeps.  Up to near-ties
    (reference scores within rel of the k-th value): every index scoring clearly above the k-th value is kept, and every
    kept index scores no less than just below it.  Returns the number of near-tied indices at the boundary."""
    L = score_ref.numel()
    got = [int(x) for x in got_idx.tolist() if 0 <= int(x) < L]
    assert len(got) == count and len(set(got)) == count, f"{what}: {len(got)} indices ({len(set(got))} distinct), want {count}"
    srt = torch.sort(score_ref, descending=True).values
    thr = float(srt[count - 1])
    tol = rel * abs(thr) + 1e-9 if math.isfinite(thr) else 0.0
    above = set((score_ref > thr + tol).nonzero().flatten().tolist())
    assert above <= set(got), f"{what}: an index clearly above the k-th value is missing"
    low = [g for g in got if float(score_ref[g]) < thr - tol]
    assert not low, f"{what}: indices {low[:5]} score below the k-th value"
    return int(((score_ref - thr).abs() <= tol).sum())
