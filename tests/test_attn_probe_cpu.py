"""CPU: the mask read-out of tests/attn_probe.py on a plain f32 torch attention that takes a multiplicity matrix - the decoder
returns the mask it was given, names a seeded defect (one pair dropped, added or doubled) by pair and kind, and rests on two
rounding facts asserted here; and one stated case of why the tolerance tests cannot see membership."""
import functools

import pytest
import torch

import attn_probe as ap
from minference_ref import attention_ref, brute_mask, window_mask
from util import attention_tolerance


def read_out(mult, L, R=None, seed=0):
    """All C launches of the probe through ap.attend with the multiplicity matrix mult [R, L] -> the filled Probe."""
    probe = ap.Probe(L, R, seed=seed)
    for s in range(probe.C):
        q, k, v = probe.inputs(s)
        probe.read(s, ap.attend(mult, q[0, 0], k[0, 0], v[0, 0]).view(1, probe.R, 1, ap.D))
    return probe


def decoded(mult, expected, L, R=None):
    return read_out(mult, L, R).decode(0, 0, slice(None), expected)


@functools.lru_cache(maxsize=None)
def family_mask(L, name):
    slash, vert = {n: (s, v) for n, s, v in ap.sparse_families(L)}[name]
    return brute_mask(L, torch.tensor(vert), torch.tensor(slash))


def test_rounding_facts():
    """What the decoder rests on: for l <= 128 and mult <= 3 every f32 within 8 ulp of mult / l rounds to one bf16 (a
    reciprocal that is not IEEE's cannot change a bit), and bf16(1 / l) names l."""
    stable, injective = ap.rounding_facts(128, 8)
    assert stable and injective
    # the decoder's table goes a few l further, for rows to which a defect adds keys: the same two facts there
    assert ap.rounding_facts(ap.TABLE_L, 8) == (True, True)
    t = ap._ratio_table()
    assert bool((t[:, 0] < t[:, 1]).all()) and bool((t[:, 1] < t[:, 2]).all())
    # the score gap: exp2(-522) and exp(-362) are 0 in f32, with or without denormals (2^-149 is the smallest)
    gap = 4096.0 * 1.4426950408889634 / 128 ** 0.5
    assert gap > 520 and float(torch.exp2(torch.tensor(-gap, dtype=torch.float32))) == 0.0


def test_probe_inputs():
    p = ap.Probe(1000, bs=2, Hq=4, Hkv=2, seed=3)
    assert p.C == 8
    chunks_k, chunks_q, blocks_v = set(), set(), set()
    for s in range(p.C):
        q, k, v = p.inputs(s)
        for t in (q, k, v):
            assert t.dtype == torch.bfloat16 and t.is_contiguous() and bool(((t != 0).sum(-1) == 1).all())
        assert set(q.unique().tolist()) == {0.0, 64.0} == set(k.unique().tolist()) and set(v.unique().tolist()) == {0.0, 1.0}
        # a row's probed keys are those of class (i + s + shift) % C, and score 4096; every other key scores 0
        sc = q[1, 3].float() @ k[1, 1].float().T
        cls = (torch.arange(1000).view(-1, 1) + s + 1 + 3) % 8 == (torch.arange(1000) % 8).view(1, -1)
        assert torch.equal(sc, torch.where(cls, 4096.0, 0.0))
        # V names the group: keys of one group share a dimension, groups differ
        vd = v[0, 0].float().argmax(-1)
        assert torch.equal(vd[::8][:125].unique().numel() * torch.ones(1), 125.0 * torch.ones(1)) and bool((vd[:8] == vd[0]).all())
        chunks_k |= set((k[0, 0].float().argmax(-1) // 8).tolist())
        chunks_q |= set((q[0, 0].float().argmax(-1) // 8).tolist())
        blocks_v |= set((vd // 32).tolist())
    assert len(chunks_k) == 16 and len(chunks_q) == 16 and blocks_v == {0, 1, 2, 3}
    with pytest.raises(ValueError):
        ap.n_classes(16385)
    assert ap.n_classes(16384) == 128 and ap.n_classes(128) == 1 and ap.n_classes(129) == 2


@pytest.mark.parametrize("L", [2, 65, 130])
def test_read_out_returns_the_mask(L):
    for name, slash, vert in ap.sparse_families(L):
        mask = family_mask(L, name)
        assert torch.equal(mask, window_mask(L, torch.tensor(vert), torch.tensor(slash))), name
        mult = decoded(mask.int(), mask, L)
        assert torch.equal(mult[:, :L] > 0, mask) and bool((mult[:, :L] <= 1).all()) and not bool(mult[:, L:].any()), name
        assert ap.defects(mult, mask, L) == []


@pytest.mark.parametrize("name", ["cover-mixed", "v-late"])
def test_read_out_returns_the_mask_at_1000(name):
    L = 1000
    mask = family_mask(L, name)
    probe = read_out(mask.int(), L)
    assert ap.check(probe, lambda b, h, r0, r1: mask[r0:r1], slab=300) == int(mask.sum())


def test_read_out_returns_every_family_at_1000():
    """All families at L = 1000 against window_mask (held to brute_mask above and in test_minference_cpu.py: brute_mask
    itself takes seconds per family at this length)."""
    L = 1000
    for name, slash, vert in ap.sparse_families(L):
        mask = window_mask(L, torch.tensor(vert), torch.tensor(slash))
        mult = decoded(mask.int(), mask, L)
        assert torch.equal(mult[:, :L] > 0, mask) and bool((mult[:, :L] <= 1).all()) and not bool(mult[:, L:].any()), name


def test_read_out_of_the_dense_masks():
    for q_len, kv_len in ((1, 1), (128, 128), (129, 129), (300, 300), (1, 2), (65, 128), (130, 195), (200, 533)):
        mask = ap.causal_mask(q_len, kv_len)
        probe = read_out(mask.int(), kv_len, q_len)
        assert ap.check(probe, lambda b, h, r0, r1: mask[r0:r1]) == int(mask.sum())


# ---------------------------------------------------------------------------------------------------- seeded defects
def observable(row, j, kind, C):
    """Whether the probe can show the defect at key j of a row whose attended keys are `row` (bool [L]): see the last
    paragraph of attn_probe's docstring."""
    keys = row.nonzero().flatten()
    same = keys[(keys % C == j % C) & (keys != j)]
    rest = keys[keys % C != j % C]
    if kind == "doubled":
        return same.numel() >= 1
    if same.numel() >= 1:
        return True
    if rest.numel() == 0:                # the only key of the row: an extra one shows, but names only its group when C > 1
        return kind == "dropped" or C == 1
    return bool((rest // C != j // C).any())


def places(mask, kind, C):
    """{place: (row, key)} for a defect of `kind` in mask [R, L]: the first and the last row that can show one, a row
    whose class set becomes (dropped) or was (extra) empty, and a row whose class set holds 128 keys."""
    R, L = mask.shape
    off = L - R

    def candidates(i):
        row = mask[i]
        if kind == "extra-below":
            cand = (~row[:off + i + 1]).nonzero().flatten().tolist()
        elif kind == "extra-above":
            cand = ((~row[off + i + 1:]).nonzero().flatten() + off + i + 1).tolist()
        else:
            cand = row.nonzero().flatten().tolist()
        what = kind if kind in ("doubled", "dropped") else "extra"
        return [j for j in cand[:3] + cand[-3:] if observable(row, j, what, C)]

    found = {}
    for tag, order in (("first", range(R)), ("last", range(R - 1, -1, -1))):
        for i in order:
            cand = candidates(i)
            if cand:
                found[tag] = (i, cand[0])
                break
    for i in range(R):
        for j in candidates(i):
            n_class = int(mask[i, j % C::C].sum())
            if kind != "doubled" and n_class == (1 if kind == "dropped" else 0):
                found.setdefault("class set empty", (i, j))
            if n_class == 128:
                found.setdefault("class set of 128", (i, j))
    return found


DEFECT_MASKS = [("dense", 128, 128), ("dense", 256, 256), ("dense", 70, 326), ("run65", 130, 130), ("cover-mixed", 130, 130),
                ("v-late", 65, 65), ("s0", 2, 2), ("v-late", 300, 300), ("cover-mixed", 1000, 1000)]


@pytest.mark.parametrize("kind", ["dropped", "extra-below", "extra-above", "doubled"])
@pytest.mark.parametrize("name, R, L", DEFECT_MASKS)
def test_seeded_defect_is_named(name, R, L, kind):
    mask = ap.causal_mask(R, L) if name == "dense" else family_mask(L, name)
    C = ap.n_classes(L)
    spots = places(mask, kind, C)
    want_kind = {"dropped": "missing", "doubled": "doubled"}.get(kind, "extra")
    if name == "dense" and R in (128, 256) and kind in ("dropped", "doubled", "extra-above"):
        assert "class set of 128" in spots or kind == "extra-above"
    if kind == "dropped":
        assert {"first", "last"} <= set(spots)
    for place, (i, j) in spots.items():
        mult = mask.int().clone()
        mult[i, j] = {"dropped": 0, "doubled": 2}.get(kind, 1)
        got = decoded(mult, mask, L, R)
        assert ap.defects(got, mask, L) == [(i, j, want_kind)], (place, i, j)
        assert int(got[i, j]) == int(mult[i, j])
        probe = read_out(mult, L, R)
        with pytest.raises(AssertionError, match=rf"\(0, 0, {i}, {j}, '{want_kind}'\)"):
            ap.check(probe, lambda b, h, r0, r1: mask[r0:r1])


@pytest.mark.parametrize("L", [130, 300, 1000])
@pytest.mark.parametrize("name", ["v-diagonal", "nothing"])
def test_extra_key_in_an_empty_row_is_found(name, L):
    """A row that must attend nothing and writes anything but +0 fails, below and above the diagonal, for any C; the key is
    named exactly when the defect is two keys of different groups and classes, otherwise by its group (the other keys of the
    group, of the other classes, give the same output)."""
    mask = window_mask(L, *[torch.tensor(x) for x in reversed({n: (s, v) for n, s, v in ap.sparse_families(L)}[name])])
    C = ap.n_classes(L)
    empty = (~mask.any(1)).nonzero().flatten().tolist()
    assert empty
    i = empty[len(empty) // 2]
    for j in (0, i - 1, i, i + 1, L - 1):
        mult = mask.int().clone()
        mult[i, j] = 1
        got = ap.defects(decoded(mult, mask, L), mask, L)
        assert len(got) == 1 and got[0][0] == i and got[0][1] // C == j // C and got[0][2] == "extra", (i, j, got)
        with pytest.raises(AssertionError, match=rf"\(0, 0, {i}, \d+, 'extra'\)"):
            ap.check(read_out(mult, L), lambda b, h, r0, r1: mask[r0:r1])
    mult = mask.int().clone()
    j2 = (L // C - 2) * C + (3 % C + 1) % C                     # another group and another class than key 3
    mult[i, 3] = mult[i, j2] = 1
    assert ap.defects(decoded(mult, mask, L), mask, L) == [(i, 3, "extra"), (i, j2, "extra")]
    # a value that is no mean of one-hot rows in an empty row
    probe = read_out(mask.int(), L)
    probe.grid[0, 0, i, 7, 0] = -0.0
    assert ap.defects(probe.decode(0, 0, slice(None), mask), mask, L)[0][2] == "unreadable"


def test_every_place_is_exercised():
    """The four places of the defect tests exist among DEFECT_MASKS for each kind that can have them."""
    seen = {k: set() for k in ("dropped", "extra-below", "extra-above", "doubled")}
    for name, R, L in DEFECT_MASKS[:8]:
        mask = ap.causal_mask(R, L) if name == "dense" else family_mask(L, name)
        for kind in seen:
            seen[kind] |= set(places(mask, kind, ap.n_classes(L)))
    assert seen["dropped"] == {"first", "last", "class set empty", "class set of 128"}
    assert seen["doubled"] >= {"first", "last", "class set of 128"}
    assert seen["extra-below"] >= {"first", "last", "class set empty"}
    assert seen["extra-above"] >= {"first", "last", "class set empty"}


def test_what_no_probe_can_see():
    """A key attended twice and nothing else of its class is the same softmax: the same bits (attn_probe's docstring)."""
    mask = ap.causal_mask(130, 130)
    twice = mask.int().clone()
    twice[0, 0] = 2
    a, b = read_out(mask.int(), 130), read_out(twice, 130)
    assert torch.equal(a.grid.view(torch.int16), b.grid.view(torch.int16))


def test_unreadable_output_is_reported():
    mask = ap.causal_mask(65, 65)
    probe = read_out(mask.int(), 65)
    probe.grid[0, 0, 40, 3, 0] = 0.3                       # no bf16(mult / l)
    probe.grid[0, 0, 41, 90, 0] = 1.0                      # a key >= L
    got = probe.decode(0, 0, slice(None), mask)
    assert bool((got[40] == -1).all()) and ("unreadable" in {d[2] for d in ap.defects(got, mask, 65)})
    assert bool((got[41] == -1).all())
    with pytest.raises(AssertionError, match="unreadable"):
        ap.check(probe, lambda b, h, r0, r1: mask[r0:r1])
    nan = read_out(mask.int(), 65)
    nan.grid[0, 0, 7] = float("nan")
    assert bool((nan.decode(0, 0, slice(None), mask)[7] == -1).all())


# ------------------------------------------------------------------------------- why the tolerance tests are not enough
def test_one_missing_key_hides_inside_the_tolerance():
    """L = 4113, the "random" lists of test_gpu_minference_attention (G = 4, bs = 1): drop ONE attended key of the last row
    from the f64 reference.  In every head whose last row attends 512 keys or more (a single key then weighs 1 / n < 2^-9 on
    average) the change from losing the key of median weight stays inside the bound that test asserts,
    attention_tolerance(ref) + 2^-8 absv.  Measured: six such heads (757 to 2,644 keys), change / bound 0.095 to 0.419 for
    the median key, and 8,633 of all 9,757 single-key removals (88 %) stay inside the bound; the head of 173 keys shows
    its median key (1.69)."""
    import test_gpu_minference_attention as t
    L, G, bs, Hq = 4113, 4, 1, 8
    vi, si = t._lists(bs, Hq, L, torch.Generator().manual_seed(31 * L + G + bs), "random", device="cpu")
    gen = torch.Generator().manual_seed(17 * L + G + bs)
    rnd = lambda shape, scale=1.0: (torch.randn(*shape, generator=gen) * scale).to(torch.bfloat16)      # noqa: E731
    q, k, v = rnd((bs, Hq, L, 128), 1.5), rnd((bs, 2, L, 128)), rnd((bs, 2, L, 128))
    ref, absv = attention_ref(q, k, v, vi, si, rows=[L - 1])
    inside = total = 0
    worst_median = 0.0
    for h in range(Hq):
        mask = window_mask(L, vi[0, h], si[0, h], rows=[L - 1])[0]
        keys = mask.nonzero().flatten()
        sc = (q[0, h, L - 1].double() @ k[0, h // G, keys].double().T) / 128 ** 0.5
        p = torch.softmax(sc, 0)
        vh = v[0, h // G, keys].double()
        assert float((p @ vh - ref[0, 0, h]).abs().max()) < 1e-12
        # out without key n: (out - p_n v_n) / (1 - p_n), for every n at once
        less = (ref[0, 0, h].view(1, -1) - p.view(-1, 1) * vh) / (1 - p).view(-1, 1)
        bound = (attention_tolerance(ref[0, 0, h]) + 2.0 ** -8 * absv[0, 0, h]).view(1, -1)
        ratio = ((less - ref[0, 0, h].view(1, -1)).abs() / bound).amax(1)                 # per removed key
        med = float(ratio[p.argsort()[keys.numel() // 2]])
        print(f"head {h}: {keys.numel()} keys, median-weight key ratio {med:.3f}, inside {float((ratio < 1).float().mean()):.3f}")
        assert bool((ratio < 1).any())                                                    # every head hides some key
        if keys.numel() >= 512:
            inside += int((ratio < 1).sum())
            total += keys.numel()
            worst_median = max(worst_median, med)
    print(f"rows of >= 512 keys: worst median-key ratio {worst_median:.3f}; {inside} of {total} removals inside the bound")
    assert total > 0 and worst_median < 1.0
    assert inside > total // 2
