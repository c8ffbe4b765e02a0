"""Mask read-out for the prefill attention kernels (DESIGN.md sections 8 and 9): probe inputs for which the bf16 output of a
causal / sparse attention names, for every (query row, key) pair, whether the row attended the key and how many times.  Plain
torch, no library import: the CPU tests run it on a small torch attention, the GPU tests on the kernels.

The probe (D = 128, L = kv_len <= 16,384, C = ceil(L / 128) classes):
  key j has class j % C and group j // C (< 128);  K[j] = 64 e_kdim(class),  V[j] = e_vdim(group);
  query row i of launch s probes class t = (i + s + shift) % C:  Q[i] = 64 e_kdim(t).
  kdim / vdim are bijections (a x + b) mod 128, a odd, that change with the launch, the sequence and the KV head.
A probed key scores 4096, any other key 0: in the log2 domain the gap is 4096 log2(e) / sqrt(128) = 522, so next to an
attended probed key every other key weighs exp2(-522) = 0 in f32 (below the smallest denormal), and the rescale of what was
accumulated before the first probed key is exactly 0 too.  A row that attends n probed keys (with multiplicity: l = n <= 128)
therefore writes bf16(mult_g / l) at vdim(g) for each of them and +0 elsewhere; the values name l and every multiplicity
(rounding_facts()).  A row that attends no probed key weighs its other keys 1 each and writes the mean of their one-hot V rows,
which the expected mask predicts (within one bf16 ulp: l is not bounded there); a row with no key at all writes +0 bits.
C launches (s = 0 .. C - 1) read every pair once.  L <= 16,384 because a class must not hold more than 128 keys: 128 one-hot V
dimensions tell that many keys apart, and bf16(1 / l) stops being injective soon after l = 128 (8 significand bits).

What the read-out cannot see, by construction: a reading (row, class) is one softmax, and a softmax over a key attended twice
and nothing else, or over the same keys all attended twice, equals the plain one - so a doubled key shows only when its class
holds a second attended key in that row; and a row whose attended keys all lie in ONE group (the dense rows i < C when
C > 1) writes e_vdim(group) whichever non-empty subset of the group it attends.  The cases with C = 1 (L <= 128) read those
first rows exactly."""
import math

import torch

D = 128
L_MAX = 128 * D
TABLE_L = 136                       # l the decoder can name: 128 plus what a seeded / real defect may add


def n_classes(L):
    if not 1 <= L <= L_MAX:
        raise ValueError(f"the probe reads kv_len in [1, {L_MAX}], got {L}")
    return (L + D - 1) // D


def bf16_of(x):
    """f64 value(s) -> the bf16 the kernel's f32 -> bf16 rounding gives, as f32."""
    return torch.as_tensor(x, dtype=torch.float64).to(torch.float32).to(torch.bfloat16).float()


def _ratio_table():
    l = torch.arange(1, TABLE_L + 1, dtype=torch.float64).view(-1, 1)
    m = torch.arange(1, 4, dtype=torch.float64).view(1, -1)
    return bf16_of(m / l)                                    # [TABLE_L, 3]: bf16(mult / l)


def rounding_facts(max_l=128, ulps=8):
    """The two facts the decoder rests on, recomputed: (every f32 within `ulps` ulp of mult / l rounds to one bf16, for
    l <= max_l and mult <= 3;  bf16(1 / l) != bf16(1 / (l + 1)) for l < max_l)."""
    l = torch.arange(1, max_l + 1, dtype=torch.float64).view(-1, 1, 1)
    m = torch.arange(1, 4, dtype=torch.float64).view(1, -1, 1)
    x = (m / l).to(torch.float32)
    near = (x.view(torch.int32) + torch.arange(-ulps, ulps + 1, dtype=torch.int32).view(1, 1, -1)).view(torch.float32)
    stable = bool((near.to(torch.bfloat16) == x.to(torch.bfloat16)).all())
    inv = bf16_of(1.0 / torch.arange(1, max_l + 1, dtype=torch.float64))
    return stable, bool((inv[1:] != inv[:-1]).all())


def launch_maps(p):
    """(kdim, vdim) of permutation number p: int64 [128] bijections of 0 .. 127.  The 16-byte chunk of kdim(0) and the
    32-dimension output block of vdim(0) step through all their values as p counts up."""
    x = torch.arange(D)
    ak, bk = 2 * ((5 * p + 1) % 64) + 1, (8 * p + p // 16) % D
    av, bv = 2 * ((3 * p + 2) % 64) + 1, (32 * p + 8 * (p // 4) + p // 16) % D
    return (ak * x + bk) % D, (av * x + bv) % D


class Probe:
    """Probe inputs and read-out of one case: q [bs, Hq, R, 128] over k / v [bs, Hkv, L, 128], R = q_len query rows.
    Sequence b and query head h shift the probed class by seq_shift b + h, so sequences and heads differ."""

    def __init__(self, L, R=None, bs=1, Hq=1, Hkv=1, device="cpu", seed=0, seq_shift=1):
        self.L, self.R, self.C = L, L if R is None else R, n_classes(L)
        self.bs, self.Hq, self.Hkv, self.G = bs, Hq, Hkv, Hq // Hkv
        self.device, self.seed = torch.device(device), seed
        assert bs == 1 or self.C == 1 or seq_shift % self.C, "the sequences would probe the same classes"
        shift = seq_shift * torch.arange(bs).view(-1, 1) + torch.arange(Hq).view(1, -1)
        self.shift = shift.to(self.device)                                                      # [bs, Hq]
        self.grid = torch.zeros(bs, Hq, self.R, D, self.C, dtype=torch.bfloat16, device=self.device)
        self.seen = torch.zeros(self.C, dtype=torch.bool)

    def _maps(self, s):
        """kdim, vdim int64 [bs, Hkv, 128] of launch s."""
        km = torch.empty(self.bs, self.Hkv, D, dtype=torch.int64)
        vm = torch.empty_like(km)
        for b in range(self.bs):
            for hk in range(self.Hkv):
                km[b, hk], vm[b, hk] = launch_maps(self.seed + s + 11 * b + 5 * hk)
        return km.to(self.device), vm.to(self.device)

    def _classes(self, s):
        """int64 [bs, Hq, R]: the class row i of (b, h) probes in launch s."""
        i = torch.arange(self.R, device=self.device).view(1, 1, -1)
        return (i + s + self.shift.unsqueeze(-1)) % self.C

    def inputs(self, s):
        """(q [bs, Hq, R, 128], k, v [bs, Hkv, L, 128]) bf16, contiguous, of launch s."""
        km, vm = self._maps(s)
        j = torch.arange(self.L, device=self.device)
        shape = (self.bs, self.Hkv, self.L, D)
        k = torch.zeros(shape, dtype=torch.bfloat16, device=self.device)
        v = torch.zeros(shape, dtype=torch.bfloat16, device=self.device)
        k.scatter_(3, km[:, :, j % self.C].unsqueeze(-1), 64.0)
        v.scatter_(3, vm[:, :, j // self.C].unsqueeze(-1), 1.0)
        kq = km.repeat_interleave(self.G, dim=1)                                                # [bs, Hq, 128]
        q = torch.zeros(self.bs, self.Hq, self.R, D, dtype=torch.bfloat16, device=self.device)
        q.scatter_(3, torch.gather(kq, 2, self._classes(s)).unsqueeze(-1), 64.0)
        return q, k, v

    def read(self, s, out):
        """Files the output of launch s, out [bs, R, Hq, 128] bf16 (the kernels' layout), under (row, group, class)."""
        assert out.shape == (self.bs, self.R, self.Hq, D) and out.dtype == torch.bfloat16
        _, vm = self._maps(s)
        vq = vm.repeat_interleave(self.G, dim=1).unsqueeze(2).expand(-1, -1, self.R, -1)        # [bs, Hq, R, 128]
        vals = torch.gather(out.permute(0, 2, 1, 3), 3, vq)                                     # [b, h, i, g]
        t = self._classes(s).view(self.bs, self.Hq, self.R, 1, 1).expand(-1, -1, -1, D, -1)
        self.grid.scatter_(4, t, vals.unsqueeze(-1))
        self.seen[s % self.C] = True

    def decode(self, b, h, rows, expected):
        """Multiplicities int8 [len(rows), 128 C] of the rows `rows` (a slice) of (sequence b, head h) against expected
        bool [len(rows), L]; see decode_readings."""
        assert bool(self.seen.all()), "launches s = 0 .. C - 1 must all be read first"
        return decode_readings(self.grid[b, h, rows], expected.to(self.device), self.L)


def _by_value(vals):
    """vals bf16 [r, 128, C] -> (mult int64 [r, 128, C], form_a bool [r, C]): each reading taken as {bf16(mult_g / l)} with
    sum(mult) = l <= TABLE_L, the smallest value being bf16(1 / l), and whether it has that form."""
    x = vals.float()
    nz = vals.view(torch.int16) != 0                                           # -0 and NaN are not +0
    table = _ratio_table().to(vals.device)
    vmin = torch.where(nz & (x > 0), x, torch.full_like(x, float("inf"))).amin(1)              # [r, C]
    hit = vmin.unsqueeze(-1) == table[:, 0]                                                    # [r, C, TABLE_L]
    l_hat = torch.where(hit.any(-1), hit.int().argmax(-1) + 1, torch.zeros_like(hit[..., 0], dtype=torch.int64))
    want = table[(l_hat - 1).clamp(min=0)]                                                     # [r, C, 3]
    eq = x.unsqueeze(-1) == want.unsqueeze(1)                                                  # [r, 128, C, 3]
    mult = (eq.long() * torch.arange(1, 4, device=vals.device)).sum(-1)                        # [r, 128, C]
    return mult, (l_hat > 0) & ((mult > 0) == nz).all(1) & (mult.sum(1) == l_hat)


def _is_mean(vals, keys):
    """bool [r, C]: reading (row, class) is the mean of the one-hot V rows of the row's keys of the OTHER classes, keys
    int64 [r, 128, C] multiplicities, within one bf16 ulp of the f64 value; +0 bits where that mean has nothing."""
    others = keys.sum(2, keepdim=True) - keys
    pred = others.double() / others.sum(1, keepdim=True).clamp(min=1).double()
    ulp = torch.exp2(torch.floor(torch.log2(pred.clamp(min=1e-300))) - 7)
    nz = vals.view(torch.int16) != 0
    return torch.where(pred > 0, (vals.double() - pred).abs() <= ulp, ~nz).all(1)              # NaN fails


def decode_readings(vals, expected, L):
    """vals bf16 [r, 128, C] (row, group, probed class), expected bool [r, L] -> int8 [r, 128 C]: how many times each row
    attended each key (column g C + t); columns >= L are keys that do not exist.

    Pass / fail rests on `expected` alone.  A row is clean iff every one of its C readings is what `expected` predicts:
    a class with expected keys reads {bf16(mult_g / l)}, sum(mult) = l, with mult equal to `expected` (each key once); a class
    with none reads the mean of the row's expected keys within one bf16 ulp, +0 bits if the row has no key at all.  A clean
    row returns `expected`.  Any other row never does: _attribute names its defects as well as it can, and a reading it
    cannot explain returns -1 for all its keys."""
    r, _, C = vals.shape
    E = torch.zeros(r, D * C, dtype=torch.bool, device=vals.device)
    E[:, :L] = expected
    Ei = E.view(r, D, C).long()
    has = Ei.any(1)                                                                            # [r, C]
    mult, form_a = _by_value(vals)
    clean = torch.where(has, form_a & (mult == Ei).all(1), _is_mean(vals, Ei))                 # [r, C]
    res = Ei.clone()
    bad = (~clean.all(1)).nonzero().flatten()
    if bad.numel():
        res[bad] = _attribute(vals[bad], Ei[bad], mult[bad], form_a[bad], clean[bad])
    return res.to(torch.int8).reshape(r, D * C)


def _attribute(vals, Ei, mult, form_a, clean):
    """Best-effort reading of rows that are not clean (the same shapes as in decode_readings, those rows only) -> int64
    [n, 128, C].  A defect in one class changes the mean the other classes of its row read, so the order is: classes with
    expected keys (as expected / all missing = the mean of the other expected keys / by value); then classes without, as the
    mean of what the row was read as so far, one class after the other; what is left by value (extra keys) or -1.  Which
    key of a group is extra cannot be told when the row attends nothing outside that group (the module docstring)."""
    n, _, C = Ei.shape
    has = Ei.any(1, keepdim=True)                                                              # [n, 1, C]
    zero, unread = torch.zeros_like(mult), torch.full_like(mult, -1)
    by_value = torch.where(form_a.unsqueeze(1), mult, unread)
    b1 = _is_mean(vals, Ei).unsqueeze(1)
    prior = (form_a & (mult == Ei).all(1)).unsqueeze(1)
    # (both can fit, e.g. 128 other keys, one per group, against 128 keys of the class: then the fewer defects)
    fewer = (Ei.sum(1) <= torch.where(form_a, (mult != Ei).sum(1), torch.full_like(form_a, D * C, dtype=torch.int64)))
    res = torch.where(prior, Ei, torch.where(b1 & fewer.unsqueeze(1), zero, by_value))
    res = torch.where(has, res, torch.where(b1, zero, by_value))
    cur = torch.where(has, torch.where(res < 0, Ei, res), zero)
    opened = (~has & ~b1).squeeze(1)                                                           # [n, C]
    for tentative in (False, True):        # first against the classes with expected keys, then with the open ones by value
        if tentative:
            cur = torch.where(opened.unsqueeze(1), res.clamp(min=0), cur)
        for t in opened.any(0).nonzero().flatten().tolist():
            others = cur.sum(2) - cur[:, :, t]                                                 # [n, 128]
            fits = _is_mean(vals[:, :, t:t + 1], torch.stack([torch.zeros_like(others), others], 2))[:, 0] & opened[:, t]
            res[:, :, t] = torch.where(fits.unsqueeze(1), zero[:, :, t], res[:, :, t])
            cur[:, :, t] = torch.where(fits.unsqueeze(1), zero[:, :, t], cur[:, :, t])
            opened[:, t] &= ~fits
    # a row that is not clean never reads as expected: what made it so is then unreadable
    same = (res == Ei).all(2).all(1)
    return torch.where((same.view(-1, 1) & ~clean).unsqueeze(1), unread, res)


def defects(mult, expected, L, row0=0, limit=8):
    """[(row, key, kind)]: the first `limit` pairs where mult (decode) differs from expected, kind in "missing", "extra",
    "doubled" (any multiplicity above one) or "unreadable" (a reading of neither form)."""
    E = torch.zeros_like(mult, dtype=torch.bool)
    E[:, :L] = expected.to(mult.device)
    bad = (mult != E.to(torch.int8)).nonzero()[:limit].tolist()
    out = []
    for i, j in bad:
        m = int(mult[i, j])
        kind = "unreadable" if m < 0 else "doubled" if m > 1 else "missing" if m == 0 else "extra"
        out.append((row0 + i, j, kind))
    return out


def check(probe, expected_of, slab=512):
    """Asserts that the read-out equals the contract's mask: for every (sequence, head), in slabs of rows, the decoded bool
    matrix equals expected_of(b, h, row0, row1) (bool [row1 - row0, L]) under torch.equal, every attended key has
    multiplicity one, and no key >= L shows.  Returns the number of attended pairs."""
    problems, pairs = [], 0
    for b in range(probe.bs):
        for h in range(probe.Hq):
            for r0 in range(0, probe.R, slab):
                r1 = min(probe.R, r0 + slab)
                exp = expected_of(b, h, r0, r1).to(probe.device)
                mult = probe.decode(b, h, slice(r0, r1), exp)
                pairs += int(exp.sum())
                same = torch.equal(mult[:, :probe.L] > 0, exp) and bool((mult >= 0).all())
                once = bool((mult <= 1).all()) and not bool(mult[:, probe.L:].any())
                if not (same and once):
                    problems += [(b, h) + d for d in defects(mult, exp, probe.L, r0)]
            if len(problems) >= 8:
                break
    assert not problems, "(sequence, head, row, key, kind): " + ", ".join(map(str, problems[:8]))
    return pairs


def attend(mult, q, k, v):
    """The contract's attention of q [R, 128] over k / v [L, 128] with key j attended mult[i, j] times by row i (int
    [R, L]): f32, softmax(q.k / sqrt(D)), the weights rounded to bf16 for P.V and not for the row sum, a row with no key
    is 0.  -> bf16 [R, 128]."""
    s = (q.float() @ k.float().T) / math.sqrt(D)
    on = mult > 0
    s = torch.where(on, s, torch.full_like(s, float("-inf")))
    mx = s.amax(1, keepdim=True)
    p = torch.where(on, torch.exp(s - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))), torch.zeros_like(s))
    m = mult.float()
    l = (m * p).sum(1, keepdim=True)
    o = (m * p.to(torch.bfloat16).float()) @ v.float()
    return torch.where(l > 0, o / l.clamp(min=1e-30), torch.zeros_like(o)).to(torch.bfloat16)


def causal_mask(q_len, kv_len, row0=0, row1=None, device="cpu"):
    """bool [row1 - row0, kv_len]: the dense contract, j <= kv_len - q_len + i."""
    rows = torch.arange(row0, q_len if row1 is None else row1, device=device).view(-1, 1)
    return torch.arange(kv_len, device=device).view(1, -1) <= kv_len - q_len + rows


# ------------------------------------------------------------------------------------------------ index-list families
BIG = [2 ** 31 + 5, 2 ** 33, -2 ** 40]              # int64 entries beyond int32: outside [0, L) either way


def _distinct(L, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(L, generator=g)[:min(n, L)].tolist()


def sparse_families(L, starred=False):
    """[(name, slash list, vertical list)] for prompt length L: the (slash family, vertical family) pairs of the mask
    read-out tests.  Lists are plain ints in any order; entries outside [0, L) are part of the test (the kernel ignores
    them).  starred=True: only the families that are also run at the long length.  The comment at each family names the
    condition of vs_attn_kernel (csrc/skv_minference.hip) it is chosen for."""
    nb = (L + 63) // 64
    e_last, e_mid = 64 * nb, 64 * max(1, nb // 2)
    cols = lambda n, seed=0: _distinct(L, n, 1000 * L + n + seed)          # noqa: E731
    fam = []

    def add(name, slash, vert, star=False):
        if star or not starred:
            fam.append((name, [int(x) for x in slash] or [-1], [int(x) for x in vert] or [-1]))

    # ---- slash families
    # `int top = e, cov = e` + the first absorb: s = 0 gives hi == cov, the window [e - 64, e) opens the walk
    add("s0", [0], cols(1))
    add("s0+v64", [0], cols(64))
    # `if (hi < cov) break;` on the very first entry, then `if (sp < n_slash) { ... top = max(e - s, FT_KB)`: a new range
    add("no-s0", [3, 70], cols(63))
    # `cur_start + FT_KB - 1 <= qw` (the unmasked fast path): the tile's last key e - s - 1 at qw + 1, qw, qw - 1 of wave 1
    # (qw = e - 32: s = 30, 31, 32; 33, 34 beyond) and of wave 0 (qw = e - 64: s = 62, 63, 64; 65, 66 beyond)
    for s in (30, 31, 32, 33, 34, 62, 63, 64, 65, 66):
        add(f"iso{s}", [s], [0] if s % 2 else [L + 1])
    # `if (hi < cov) break;`: windows that overlap by one key, touch (hi == cov merges), leave a gap of one key
    for gap in (63, 64, 65):
        add(f"pair{gap}", [5, 5 + gap], cols(2, gap))
    # `cov > top - FT_KB` / `start = max(cov, top - FT_KB)`: runs merge into one range, cut from the top, short bottom tile
    for n in (1, 2, 63, 64, 65, 200):
        add(f"run{n}", range(7, 7 + n), cols(65, n), star=True)
    # `cov = min(cov, hi - FT_KB)` with hi unchanged: duplicated offsets
    add("dup-s", [4, 4, 4, 90, 90, 4], cols(3))
    # `const int hi = max(e - s, FT_KB)` (clamp to [0, 64)) and `if (s >= lim) { sp = n_slash; break; }` around e_b
    for name, e in (("b0", 64), ("bmid", e_mid), ("blast", e_last)):
        add(f"edge-{name}", [e - 65, e - 64, e - 63, e - 1, e, e + 1], cols(5, e))
    for d in (-65, -63, -1, 0):
        add(f"edge-last{d}", [e_last + d], [L - 1] if d else [])
    # lim = min(e, L): the largest offset that exists
    add("s-last", [L - 1], cols(64, 1))
    # `while (sp < n_slash && sl[sp] < 0) ++sp;` and s >= lim everywhere: verticals only / nothing at all
    add("no-slash+v", [-5, -1, L, L + 7] + BIG, cols(65, 2))
    add("nothing", [-1, L] + BIG, [-2, L + 3] + BIG)

    # ---- vertical families (`vl[vp] < lim`, tile_key, the dedup and the cover test of load_tile)
    for n in (1, 63, 64, 65, 128, 129):                                   # `vp += FT_KB`: one, two, three gather tiles
        add(f"v{n}", [1, 40 + n], cols(n, 3))
    # `if (i > 0 && vl[i - 1] == key)` across a gather tile: the duplicate pair at sorted positions 63 / 64
    c = max(1, L // 2)
    lower = sorted(cols(min(c, 63), 4) if c >= 63 else list(range(c)))
    lower = [x % c for x in lower]
    front = [-1] * (63 - len(set(lower))) + sorted(set(lower))
    add("dup-63-64", [2], front + [c, c] + [x for x in (c + 1, c + 9, L - 1) if x < L])
    add("triples", [0, 130], [x for y in cols(22, 5) for x in (y, y, y)])
    # the cover test `lo = max(0, e - key - FT_KB)`, `hi = min(L - 1, key < FT_KB ? e - 1 : e - key - 1)`, vs_any_bit's edge
    # masks: window offsets at bit 0 / bit 31 of a bitmap word; columns lo - 1, lo, hi - 1, hi of the window [lo, hi) of the
    # middle and last block; key % 32 == 0 makes [e - key - 64, e - key - 1] span two words, any other key three, a key in
    # the last 32 rows of the block one (clamped at 0)
    for s in (32, 63, 64, 95):
        v = []
        for e in (e_mid, e_last):
            lo, hi = max(e - s, 64) - 64, max(e - s, 64)
            v += [lo - 1, lo, hi - 1, hi, e - 20, e - 32, e - 33]
        add(f"cover-s{s}", [s], v, star=True)
    add("cover-mixed", [32, 63, 64, 200], list(range(max(0, e_mid - 140), min(L, e_mid))), star=True)
    # `key < FT_KB ? e - 1 : ...`: the clamped branch of the cover test (any offset in (e - 64, e) covers keys < 64)
    add("v-0-63-64", [e_mid - 10], [0, 63, 64])
    add("v-0-63-64-far", [e_mid + 70], [0, 63, 64])
    # `id[j] <= qi` inside a gathered tile: a column equal to a row of the block, and the one above it
    add("v-diagonal", [-1], [e_mid - 64 + 5, e_mid - 64 + 6, e_last - 64, e_last - 63, L - 1])
    # `tmin > wave_hi`: the tile's smallest column lies in rows 32 .. 63 of a block, wave 0 has nothing to do
    add("v-wave0-skip", [-1], [e_mid - 64 + 40])
    add("v-wave0-skip-last", [L], [max(0, L - 3)])
    # `vl[vp] < lim` / `x < lim`: columns >= min(e_b, L) for the early blocks, below it for the later ones
    add("v-late", [1], [10, 100, 500, L - 1, L - 2, e_mid, e_mid - 1])
    # a gather tile with nothing to add: all duplicates (entries 64 .. of one column), all covered (every offset kept)
    add("v-all-dup", [-1], [max(0, L - 7)] * 130 + [1])
    add("v-all-covered", range(L), cols(129, 6))
    # `(x >= 0 && x < lim) ? x : INT_MAX`: negative entries (sorted to the front of the first gather tile) and entries >= L
    add("v-outside", [0], [-3, -1, 5, L, L + 1] + BIG + cols(60, 7))
    return fam
