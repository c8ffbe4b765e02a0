"""Selection inputs whose bf16 logits are known exactly, at logit ranges past every cut-off of the softmax contract
(DESIGN.md section 4): shared by tests/test_wide_range_cpu.py (which proves on the CPU that every case reaches its edge) and
tests/test_gpu_wide_range_selection.py (which compares the device with the oracle on them, bit for bit).

Construction.  alpha = 0.125.  Query head g of a block owns lane g of the dot product (dimensions 8g .. 8g + 7): its profile sits
on the three dimensions 8g + 1, 8g + 3, 8g + 5 (landmark entry = one bf16 "piece" of the slot's logit, query entry = 8 x the
step's scale, 0 in every other head), so

    logit[g][j] = bf16(alpha * sum_p q[g][8g + 1 + 2p] * piece_p[g][j])            (exact in f32, one bf16 rounding)

and every piece is chosen so that the sum is exact in f32.  The other five dimensions of lanes 0 .. 7 hold small integers
(query: +-1 .. 3, the same for every head; landmark: -3 .. 3), and lane l + 8 repeats lane l with the landmark's sign flipped
(0 under the profile dimensions): all 16 lanes carry non-zero terms, every partial sum is a small multiple of a power of two
(exact), and the filler cancels in the last add of the tree.  The CPU test asserts the result bit for bit."""
import math

import numpy as np
import torch

ALPHA = 0.125
QV = 8.0                      # query entry on a profile dimension at scale 1: alpha * QV == 1
# Largest power-of-two query scale: with |profile| <= 22 and |filler| <= 3 x 3 on 5 dimensions of 8 lanes, every partial sum of
# the dot is at most (8 x 22 + 8 x 45) x scale = 536 x scale, which must stay below 2^128: scale <= 2^118 (2^119 can overflow).
# The logits then reach 22 x 2^118 = 7.3e36, the largest finite ones these shapes produce without an f32 overflow in the dot.
HUGE = 2.0 ** 118


def bf16_exact(x):
    """f64 tensor -> bf16, asserting that nothing is lost: the value is a bf16 number."""
    b = x.float().bfloat16()
    assert torch.equal(b.double(), x.double()), "a designed input is not a bf16 number"
    return b


def build_inputs(pieces, qv, seed):
    """pieces f64 [P <= 3][blocks][G][N] (bf16 numbers), qv f64 [blocks][G][P] query entries (bf16 numbers), -> (q bf16
    [blocks][G][128], landmarks bf16 [blocks][N][128], designed logits bf16 [blocks][G][N])."""
    P, blocks, G, N = pieces.shape
    assert P <= 3 and G <= 8
    g = torch.Generator().manual_seed(seed)
    fill_dims = torch.tensor([8 * l + e for l in range(8) for e in (0, 2, 4, 6, 7)])
    lm = torch.zeros(blocks, N, 128, dtype=torch.float64)
    lm[:, :, fill_dims] = torch.randint(-3, 4, (blocks, N, fill_dims.numel()), generator=g).double()
    lm[:, :, fill_dims + 64] = -lm[:, :, fill_dims]
    qf = torch.randint(1, 4, (blocks, 1, fill_dims.numel()), generator=g).double() * \
        (torch.randint(0, 2, (blocks, 1, fill_dims.numel()), generator=g).double() * 2 - 1)
    q = torch.zeros(blocks, G, 128, dtype=torch.float64)
    # the filler rides the scale of the head's first profile entry (a sequence scales the whole query)
    scale = (qv[:, :, :1].abs().max(dim=-1, keepdim=True).values / QV)
    qfill = (qf * scale).float().bfloat16().double()                        # rounded once; lane l + 8 gets the same bits
    q[:, :, fill_dims] = qfill
    q[:, :, fill_dims + 64] = qfill
    for h in range(G):
        for p in range(P):
            lm[:, :, 8 * h + 1 + 2 * p] = pieces[p, :, h, :]
            q[:, h, 8 * h + 1 + 2 * p] = qv[:, h, p]
    exact = ALPHA * torch.einsum("bgp,pbgn->bgn", qv, pieces)               # f64: exact for the magnitudes used here
    assert torch.equal(exact.float().double(), exact), "a designed logit is not exact in f32"
    return bf16_exact(q), bf16_exact(lm), exact.float().bfloat16()


def _idx_and_resident(blocks, N, S, seed):
    g = torch.Generator().manual_seed(seed + 1)
    lm_idx = torch.stack([torch.sort(torch.randperm(N + 48, generator=g)[:N]).values for _ in range(blocks)]).to(torch.int64)
    cached = torch.stack([lm_idx[b][torch.randperm(N, generator=g)[:S]] for b in range(blocks)])
    return lm_idx, cached


def _scatter(g, N, n, exclude=()):
    """n distinct slots scattered over the row (a random subset), none of `exclude`."""
    ex = set(exclude)
    perm = [int(x) for x in torch.randperm(N, generator=g).tolist() if int(x) not in ex]
    return sorted(perm[:n])


def _low(g, shape):
    """logits 90 .. 300 below a maximum of 12, on the bf16 grid (even integers)."""
    return 12.0 - 90.0 - 2.0 * torch.randint(0, 106, shape, generator=g).double()


class Case:
    """One step of selection inputs.  expected: per block the closed-form selected SLOTS (sorted), or None."""

    def __init__(self, name, blocks, G, N, S, prof, expected=None, qscale=None, extra=None, seed=0):
        self.name, self.blocks, self.G, self.N, self.S = name, blocks, G, N, S
        pieces = prof if prof.dim() == 4 else prof.unsqueeze(0)
        P = pieces.shape[0]
        qv = torch.full((blocks, G, P), QV, dtype=torch.float64) * (1.0 if qscale is None else qscale)
        self.q, self.lm, self.logits = build_inputs(pieces, qv, seed)
        self.lm_idx, self.cached = _idx_and_resident(blocks, N, S, seed)
        self.expected = expected
        self.alpha = ALPHA
        self.extra = extra or {}

    def expected_ids(self):
        return None if self.expected is None else torch.stack(
            [self.lm_idx[b][torch.tensor(self.expected[b])] for b in range(self.blocks)])


# ---------------------------------------------------------------------------------------------------------------------
# 1. cliff
# ---------------------------------------------------------------------------------------------------------------------
def cliff(blocks, G, N, S, variant="same", n_hi=None, seed=100):
    """n_hi slots within [m - 6, m] (m = 12, multiples of 1/8), every other slot 90 .. 300 below m: their softmax weight is
    exactly 0, so the selection is the n_hi slots plus the S - n_hi lowest-numbered others (ties at 0 -> lowest slot).
      same     : every head of the group has the same high slots
      per_head : high slot i belongs to head i % G alone (low in the others), head g's maximum is 12 + g: the group max decides
      one      : n_hi = 1
      dead_head: head 0 has none of the high slots: its only weight is 1.0 on one slot z of its own, which is selected too"""
    g = torch.Generator().manual_seed(seed + N + S)
    n_hi = (1 if variant == "one" else S - min(40, S // 4)) if n_hi is None else n_hi       # S - 40 (S = 32: 24)
    prof = torch.empty(blocks, G, N, dtype=torch.float64)
    expected = []
    for b in range(blocks):
        hi = _scatter(g, N, n_hi)
        low = _low(g, (G, N))
        vals = 12.0 - torch.randint(0, 49, (n_hi,), generator=g).double() / 8.0
        row = low.clone()
        chosen = set(hi)
        if variant == "per_head":
            for h in range(G):
                mine = torch.tensor(hi[h::G], dtype=torch.long)
                if mine.numel():
                    v = vals[h::G].clone()
                    v[0] = 12.0
                    row[h, mine] = v + h                       # 12 + h - k / 8 is on the bf16 grid (spacing 1/8 below 32)
                else:
                    row[h, hi[0]] = 12.0 + h
        else:
            vals[0] = 12.0
            row[:, torch.tensor(hi, dtype=torch.long)] = vals
            if variant == "dead_head":
                z = _scatter(g, N, 1, exclude=hi)[0]
                row[0] = _low(g, (N,)) - 12.0                  # head 0: everything at least 90 below its own maximum ...
                row[0, z] = 12.0                               # ... which sits on slot z alone
                chosen.add(z)
        prof[b] = row
        rest = [j for j in range(N) if j not in chosen]
        expected.append(sorted(chosen | set(rest[:S - len(chosen)])))
    return Case(f"cliff/{variant}[{blocks}-{G}-{N}-{S}]", blocks, G, N, S, prof, expected, seed=seed)


# ---------------------------------------------------------------------------------------------------------------------
# 2. straddle
# ---------------------------------------------------------------------------------------------------------------------
def straddle(blocks, G, N, S, seed=200):
    """Slots on both sides of the `x < -80 -> 0` branch.  Even blocks: m = 12 and slots at m - 79.5, m - 80, m - 80.5, m - 81
    (the bf16 grid at that magnitude is 0.5: these are -80 and its bf16 neighbours); odd blocks: m = 80 and slots at 0.5, 0,
    +-2^-10, +-2^-7, -0.5, -1, where the f32 difference D - m lands on the f32 neighbours of -80 that no bf16 logit pair
    with a small m reaches.  The high slots (within 25 of m: some at m - 10 .. m - 24.5, inside the shifted range of
    exp_to_fixed) sit in tiles 1 and 5 only, and tile 2 and the last tile hold no live slot at all: every other tile maximum is 79.5
    or more below the row maximum, and softmax_finalize sees spec_exp(m_t - m) tiny or exactly 0.  Even blocks: n_hi + #(slots >= m - 80) = S - 5 (five zero-score slots
    complete the selection: the lowest); odd blocks: S + 5 (the selection ends among the slots at exactly m - 80, lowest
    first).  Every head carries the same profile: P is monotone in the logit, so the selection is the closed form
    "by logit, ties and zeros to the lowest slot"."""
    g = torch.Generator().manual_seed(seed + N + S)
    prof = torch.empty(blocks, G, N, dtype=torch.float64)
    expected, n_live = [], []
    T = (N + 255) // 256
    hi_tiles = [t for t in (1, 5) if t < T] or [0]
    for b in range(blocks):
        m = 12.0 if b % 2 == 0 else 80.0
        below = [m - 80.5, m - 81.0] + ([] if b % 2 == 0 else [-(2.0 ** -10), -(2.0 ** -7)])     # weight exactly 0
        edge = [m - 79.5] + ([] if b % 2 == 0 else [0.5, 2.0 ** -10, 2.0 ** -7])                 # weight > 0, above the edge
        at = m - 80.0                                                                          # exp(-80): still > 0
        want_live = S - 5 if b % 2 == 0 else S + 5
        n_hi, n_edge = want_live // 2, want_live // 4
        n_at = want_live - n_hi - n_edge
        row = torch.tensor(below, dtype=torch.float64)[torch.randint(0, len(below), (N,), generator=g)]
        # a few dead slots far below as well (-90 .. -300): more zero terms in the tile sums
        far = torch.tensor(_scatter(g, N, N // 10), dtype=torch.long)
        row[far] = m - 90.0 - 2.0 * torch.randint(0, 100, (far.numel(),), generator=g).double()
        pool = [j for t in hi_tiles for j in range(256 * t, min(256 * t + 256, N))]
        hi = sorted(pool[i] for i in torch.randperm(len(pool), generator=g)[:n_hi].tolist())
        hv = m - torch.randint(0, 49, (n_hi,), generator=g).double() / 2.0        # m .. m - 24 in steps of 1/2
        hv[0] = m
        hv[1:4] = torch.tensor([m - 10.0, m - 16.0, m - 24.5])[:max(0, min(3, n_hi - 1))]
        row[torch.tensor(hi, dtype=torch.long)] = hv
        dead = [j for t in {2, T - 1} - set(hi_tiles) for j in range(256 * t, min(256 * t + 256, N))]     # tiles with no live slot
        others = _scatter(g, N, n_edge + n_at, exclude=hi + dead)
        e_slots, a_slots = others[:n_edge], others[n_edge:]
        row[torch.tensor(e_slots, dtype=torch.long)] = torch.tensor(edge, dtype=torch.float64)[
            torch.randint(0, len(edge), (n_edge,), generator=g)]
        row[torch.tensor(a_slots, dtype=torch.long)] = at
        prof[b] = row.expand(G, N)
        x = row - m
        live = x >= -80.0
        order = sorted(range(N), key=lambda j: (-(float(x[j]) if bool(live[j]) else -math.inf), j))
        expected.append(sorted(order[:S]))
        n_live.append(int(live.sum()))
    return Case(f"straddle[{blocks}-{G}-{N}-{S}]", blocks, G, N, S, prof, expected, extra={"n_live": n_live}, seed=seed)


# ---------------------------------------------------------------------------------------------------------------------
# 3. subnormal P
# ---------------------------------------------------------------------------------------------------------------------
def subnormal_p(blocks, G, N, S, n_max=2000, seed=300):
    """n_max slots at the maximum m = 80 (inv = 1 / n_max < 6.5e-4 for n_max >= 1,540), the others spread over [m - 70, m - 80]:
    on the 0.5 grid and, between m - 79.74 and m - 80 where spec_exp(D - m) * inv drops below 2^-126, on the logits k / 128,
    k = 0 .. 40.  P = bf16(spec_exp(D - m) * inv) is then an f32 denormal product and a bf16 subnormal for that tail.  No closed
    form: the oracle's IEEE arithmetic (gradual underflow, one rounding to the f32 denormal, one to bf16) is the contract."""
    g = torch.Generator().manual_seed(seed + N + S)
    n_max = min(n_max, N * 2 // 3)
    prof = torch.empty(blocks, G, N, dtype=torch.float64)
    for b in range(blocks):
        for h in range(G):
            row = torch.where(torch.rand(N, generator=g) < 0.5,
                              torch.randint(0, 21, (N,), generator=g).double() * 0.5,            # m - 80 .. m - 70
                              torch.randint(0, 41, (N,), generator=g).double() / 128.0)          # m - 80 .. m - 79.69
            row[torch.tensor(_scatter(g, N, n_max), dtype=torch.long)] = 80.0
            prof[b, h] = row
    return Case(f"subnormal_p[{blocks}-{G}-{N}-{S}]", blocks, G, N, S, prof, None, seed=seed)


# ---------------------------------------------------------------------------------------------------------------------
# 5. huge but flat
# ---------------------------------------------------------------------------------------------------------------------
def huge_flat(blocks, G, N, S, seed=500):
    """alpha * dot = 30016 + d with |d| <= 0.5, as three bf16 pieces 29952 + 64 + d.  30016 is the midpoint of the neighbouring
    bf16 numbers 29952 and 30080.  Even blocks: d <= 0 (d = 0 is the tie, to even: 29952): every logit is 29952, the softmax
    after the maximum subtraction is the uniform one (P = bf16(1 / N)) and the selection the S lowest slots.  Odd blocks: 100
    slots have d > 0 -> 30080, 128 above the rest: those 100 plus the lowest others."""
    g = torch.Generator().manual_seed(seed + N + S)
    pieces = torch.empty(3, blocks, G, N, dtype=torch.float64)
    pieces[0], pieces[1] = 29952.0, 64.0
    expected = []
    n_up = min(100, S // 2)
    for b in range(blocks):
        d = -torch.randint(0, 5, (N,), generator=g).double() / 8.0               # 0, -1/8 .. -1/2
        up = []
        if b % 2 == 1:
            up = _scatter(g, N, n_up)
            d[torch.tensor(up, dtype=torch.long)] = torch.randint(1, 5, (n_up,), generator=g).double() / 8.0
        pieces[2, b] = d.expand(G, N)
        rest = [j for j in range(N) if j not in set(up)]
        expected.append(sorted(set(up) | set(rest[:S - len(up)])))
    return Case(f"huge_flat[{blocks}-{G}-{N}-{S}]", blocks, G, N, S, pieces, expected, seed=seed)


# ---------------------------------------------------------------------------------------------------------------------
# 4. scale-jump sequences (fused selection: the state carries the previous step's log-normalisers)
# ---------------------------------------------------------------------------------------------------------------------
class Sequence:
    """Eight steps over ONE landmark table with three profile banks (A, B: logits 10 .. 22 in steps of 1/8, different per head
    and slot; C: a cliff): step t multiplies the whole query by scale[t] and reads bank[t].
        step   0    1     2     3      4    5      6        7
        scale  1   x100  x100  x0.01   1   x-100   1 (C)    1
    (big = 100: the scaled entries 100 .. 800 and bf16(0.01 k) are bf16 numbers, so the logits stay designed; big = 2^118: the
    largest magnitudes, see HUGE.)  Under the previous step's log-normalisers c~: steps 0, 1, 4, 6 have every kappa >= 0 (every
    key 32767), steps 3 and 5 every kappa < -128 (every key 0), steps 2 and 7 are mixed; step 5 inverts the ranking."""
    BANKS = (0, 0, 1, 1, 0, 0, 2, 1)

    def __init__(self, blocks, G, N, S, big=100.0, seed=400):
        self.name = f"jump/{'x100' if big == 100.0 else 'x2^118'}[{blocks}-{G}-{N}-{S}]"
        self.blocks, self.G, self.N, self.S, self.alpha = blocks, G, N, S, ALPHA
        small = 0.01 if big == 100.0 else 1.0 / big
        self.scales = (1.0, big, big, small, 1.0, -big, 1.0, 1.0)
        g = torch.Generator().manual_seed(seed + N + S)
        banks = torch.empty(3, blocks, G, N, dtype=torch.float64)
        for p in range(2):
            banks[p] = 10.0 + torch.randint(0, 97, (blocks, G, N), generator=g).double() / 8.0
        c = cliff(blocks, G, N, S, "per_head", seed=seed + 7)
        self.cliff_expected = c.expected
        banks[2] = c.logits.double()
        self.lm_idx, self.cached = _idx_and_resident(blocks, N, S, seed)
        self.q, self.logits = [], []
        self.lm = None
        for t, (s, bank) in enumerate(zip(self.scales, self.BANKS)):
            qv = torch.zeros(blocks, G, 3, dtype=torch.float64)
            entry = float(torch.tensor(QV * s).bfloat16()) if abs(s) < 1 and big == 100.0 else QV * s
            qv[:, :, bank] = entry
            q, lm, logit = build_inputs(banks, qv, seed)          # same seed: the same filler and landmark table every step
            assert self.lm is None or torch.equal(self.lm.view(torch.int16), lm.view(torch.int16))
            self.lm = lm
            self.q.append(q)
            self.logits.append(logit)


def cliff_steps(blocks, G, N, S, entry=QV, seed=600):
    """Three cliff steps (same / per_head / dead_head) over ONE landmark table, as three profile banks: step t reads bank t with
    the query entry `entry` (16: the logits under alpha = 1 / sqrt(128) are 1.414 x the profile - the low slots 127 or more
    below the maximum, the high ones within 8.5 of it: the cliff and its closed form stand).  -> (landmarks, [q_t], [expected
    slots per block]_t)."""
    cs = [cliff(blocks, G, N, S, v, seed=seed + 10 * i) for i, v in enumerate(("same", "per_head", "dead_head"))]
    banks = torch.stack([c.logits.double() for c in cs])
    qs, lm = [], None
    for t in range(3):
        qv = torch.zeros(blocks, G, 3, dtype=torch.float64)
        qv[:, :, t] = entry
        q, lm, _ = build_inputs(banks, qv, seed)
        qs.append(q)
    return lm, qs, [c.expected for c in cs]


def kappa_key(x):
    """skv_kappa_key (csrc/skv_select_front.h) restated: f32 array -> 15-bit key; floor((x + 128) * 256) clamped to
    [0, 32767], 0 at or below -128 and for NaN."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x + np.float32(128.0)) * np.float32(256.0)
        k = np.where(t >= np.float32(32767.0), 32767, np.where(np.isfinite(t), t, 0).astype(np.int64))
    return np.where(x > np.float32(-128.0), k, 0).astype(np.int64)


def selection_cases():
    """Every single-step case: N ~ 3,000 with S = 256 and the short-row shape (3 blocks, G = 8, N = 777, S = 32)."""
    out = []
    for blocks, G, N, S in ((2, 4, 3000, 256), (3, 8, 777, 32)):
        out += [cliff(blocks, G, N, S, "same"), cliff(blocks, G, N, S, "per_head"), cliff(blocks, G, N, S, "one"),
                cliff(blocks, G, N, S, "dead_head"), straddle(blocks, G, N, S), huge_flat(blocks, G, N, S)]
    # (1,540 slots at the maximum do not fit a 777-slot row: the subnormal products need the long rows)
    out += [subnormal_p(2, 4, 3000, 256), subnormal_p(2, 8, 2900, 32)]
    return out


def sequences():
    return [Sequence(2, 4, 3000, 256, 100.0), Sequence(2, 4, 3000, 256, HUGE), Sequence(3, 8, 777, 32, 100.0)]


# ---------------------------------------------------------------------------------------------------------------------
# decode attention: designed logits (tests/test_gpu_wide_range_attention.py)
# ---------------------------------------------------------------------------------------------------------------------
ATTN_SCALE = 0.125


def attention_inputs(a, Hq, seed, v=None):
    """a f64 [bs][Hkv][rows]: the logit of every key row (bf16 numbers), the same for every query head of the group.  The key
    row holds a on its first 8 dimensions and junk on the others, the query 1 on the first 8 and 0 elsewhere: scale x q.k =
    0.125 x 8 a = a in f32 under any order of the sum.  -> (q bf16 [bs][Hq][128], k, v bf16 [bs][Hkv][rows][128])."""
    bs, Hkv, rows = a.shape
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(bs, Hkv, rows, 128, generator=g).bfloat16()
    k[..., :8] = bf16_exact(a).unsqueeze(-1)
    q = torch.zeros(bs, Hq, 128, dtype=torch.bfloat16)
    q[..., :8] = 1.0
    if v is None:
        v = torch.randn(bs, Hkv, rows, 128, generator=g).bfloat16()
    return q, k.contiguous(), v.contiguous()


def dominant_positions(kv_len, splits):
    """Rows where a dominant key can go wrong: first / last attended row, first / last row of a split in the middle, first / last
    row of a wave's 32-row step and of the 128-row workgroup step inside it."""
    per = -(-kv_len // splits)
    s = min(max(1, splits // 2), (kv_len - 1) // per)
    k0 = s * per
    cand = [0, kv_len - 1, k0, min(k0 + per, kv_len) - 1, k0 - 1, k0 + 31, k0 + 32, k0 + 63, k0 + 127, k0 + 128, per - 1, per]
    out = []
    for r in cand:
        if 0 <= r < kv_len and r not in out:
            out.append(r)
    return out


def background_logits(bs, Hkv, rows, seed):
    """ordinary logits, |a| <= 8, on the bf16 grid"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(bs, Hkv, rows, generator=g) * 2).clamp(-8, 8).bfloat16().double()


def late_maximum_case(kind, bs, Hkv, kv_len, splits, seed):
    """Inputs for the tolerance gate (util.check_attention), rows = kv_len + 50 -> (a f64 [bs][Hkv][rows], v or None).
      rising : the logit grows by 3 per row (bf16(3 r)): the running maximum moves at every step, corr = exp(-3 x step rows)
      plateau: the maximum 150 sits on one row with ten rows within 5 of it in the same split; two whole splits hold a flat
               plateau at 0 (their records: finite m = 0, weight exp(-150) = 0 in the merge), the rest ordinary logits
      vmag   : ordinary logits, V rows of magnitude 1e4 next to rows of magnitude 1e-4"""
    g = torch.Generator().manual_seed(seed)
    rows = kv_len + 50
    a = background_logits(bs, Hkv, rows, seed)
    v = None
    per = -(-kv_len // splits)
    if kind == "rising":
        a[:] = (3.0 * torch.arange(rows, dtype=torch.float64)).float().bfloat16().double()
    elif kind == "plateau":
        nsp = -(-kv_len // per)
        for b in range(bs):
            for h in range(Hkv):
                smax = int(torch.randint(0, nsp, (1,), generator=g))
                for s in {(smax + 1) % nsp, (smax + 2) % nsp} - {smax}:
                    a[b, h, s * per:min((s + 1) * per, kv_len)] = 0.0
                lo, hi = smax * per, min((smax + 1) * per, kv_len)
                idx = lo + torch.randperm(hi - lo, generator=g)[:11]
                a[b, h, idx] = 150.0 - torch.randint(0, 6, (idx.numel(),), generator=g).double()      # (bf16 spacing 1 there)
                a[b, h, idx[0]] = 150.0
    elif kind == "vmag":
        mag = torch.where(torch.rand(bs, Hkv, rows, 1, generator=g) < 0.5, 1e4, 1e-4)
        v = (torch.randn(bs, Hkv, rows, 128, generator=g) * mag).bfloat16()
    else:
        raise ValueError(kind)
    return a, v
