"""GPU: every draw of the sampler (shadowkv_amd/csrc/skv_sample.hip) against tests/sampler_ref.py, path by path.

The sampler is counter-based: u is a pure function of (seed, position, batch row, winner rank), exact in f32, so the CPU names
the token of every launch.  A draw the reference decides must return its token; an undecided one (the
two best scores within sampler_ref.MARGIN, or an edge rank of the nucleus involved) must return a token of `allowed`, and at
most sampler_ref.CAP of a case's draws may be undecided.  Rows lie in buffers with row_stride > V whose gap holds a logit
above the whole row, range keys in buffers whose gap holds the largest key, and every counter has a guard word behind it:
a read or a write past an end shows as a wrong token or a changed guard.  No expected value comes from a kernel."""
import numpy as np
import pytest
import torch

import sampler_cases as sc
import sampler_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x5A5A5A5A5A5A
BASE, SLACK, TABLE = 2496, 96, 7          # counters: gen starts below the slack and runs past it, step_idx wraps


def _L():
    from shadowkv_amd import _lib
    return _lib, _lib.lib(), _lib.current_stream_handle()


def _guarded(values, dtype=torch.long):
    """[n + 1] on the device: the values, then the guard word"""
    g = GUARD if dtype == torch.long else 0x5A5A5A5A
    return torch.tensor(list(values) + [g], dtype=dtype, device=DEV)


class Counters:
    def __init__(self, pos, gen=90, step=5):
        self.pos0, self.gen0, self.step0 = [int(p) for p in pos], gen, step
        self.token, self.pos = _guarded([-1] * len(pos)), _guarded(pos)
        self.gen, self.row, self.step = _guarded([gen]), _guarded([-1]), _guarded([step])
        self.kvl = _guarded([-1], torch.int32)

    def args(self, _lib, with_step=True):
        p = _lib.ptr
        return (p(self.token), p(self.pos), p(self.gen), p(self.row), p(self.kvl), p(self.step) if with_step else 0, BASE, SLACK, TABLE)

    def check(self, launches, what, with_step=True):
        want = sr.advance(self.pos0, self.gen0, self.step0 if with_step else None, BASE, SLACK, TABLE, launches)
        bs = len(self.pos0)
        assert self.pos[:bs].tolist() == want["pos"], what
        assert (int(self.gen[0]), int(self.row[0]), int(self.kvl[0])) == (want["gen"], want["row_idx"], want["kv_len"]), what
        assert int(self.step[0]) == (want["step_idx"] if with_step else self.step0), what
        for name in ("token", "pos", "gen", "row", "step"):
            assert int(getattr(self, name)[-1]) == GUARD, f"{what}: written past {name}"
        assert int(self.kvl[-1]) == 0x5A5A5A5A, f"{what}: written past kv_len"


def device_rows(rows):
    """bf16 [bs, V + 16] on the device: the rows, and behind each a finite logit 8 above the row's maximum, which a kernel that
    reads past V draws at once (as id >= V, or as a winner of the next row).  Returns the [bs, V] view."""
    bs, V = rows.shape
    f = rows.float()
    top = torch.where(torch.isfinite(f), f, torch.full_like(f, -1e30)).amax(1, keepdim=True) + 8.0
    buf = top.bfloat16().expand(bs, V + 16).contiguous()
    buf[:, :V] = rows
    return buf.to(DEV)[:, :V]


def device_keys(rows):
    """int16 [bs, n_ranges rounded up to 8, + 8] on the device: dense_ref's keys, the gap filled with the largest key"""
    bs, V = rows.shape
    n = V // 16
    buf = torch.full((bs, (n + 7) // 8 * 8 + 8), -1, dtype=torch.int16)
    buf[:, :n] = sc.range_keys(rows).to(torch.int16)
    return buf.to(DEV)


def launch(case, rows):
    """case.L launches on rows [bs, V]; the token tensor is copied out after each.  Returns (tokens int64 [L, bs], Counters)."""
    _lib, L, st = _L()
    bs, V = rows.shape
    x = device_rows(rows)
    keys = device_keys(rows) if case.ranges else None
    c = Counters([case.pos0 + b * case.pos_stride for b in range(bs)])
    out = []
    for _ in range(case.L):
        tail = (bs, case.k, case.T, case.top_p, case.seed & (2 ** 64 - 1), *c.args(_lib, case.with_step), 0, 0, 0, st)
        if keys is not None:
            rc = L.skv_sample_topk_advance_ranges(_lib.ptr(x), x.stride(0), V, _lib.ptr(keys), keys.stride(0), *tail)
        else:
            rc = L.skv_sample_topk_advance(_lib.ptr(x), x.stride(0), V, *tail)
        assert rc == 0, (str(case), rc)
        out.append(c.token[:bs].clone())
    torch.cuda.synchronize()
    c.check(case.L, str(case), case.with_step)
    return torch.stack(out).cpu().numpy(), c


def hold(name, got, pred):
    """What each draw asserts.  Prints the case's record line first."""
    dec = pred.decided
    wrong = np.argwhere(dec & (got != pred.tokens))
    und = np.argwhere(~dec)
    outside = [(int(l), int(b)) for l, b in und if int(got[l, b]) not in pred.allowed[(int(l), int(b))]]
    runner = sum(int(got[l, b] != pred.tokens[l, b]) for l, b in und)
    mr = float(pred.ratio[dec].min()) if dec.any() else float("inf")
    print(f"SAMPLER {name}: draws {got.size}  undecided {len(und)}  to the runner-up {runner}  smallest decided best/second {mr:.6f}"
          f"  wrong {len(wrong)}")
    assert len(wrong) == 0, f"{name}: {len(wrong)} of {int(dec.sum())} decided draws differ, first (launch, row) {wrong[0].tolist()}: " \
                            f"got {int(got[tuple(wrong[0])])}, want {int(pred.tokens[tuple(wrong[0])])}, best/second {pred.ratio[tuple(wrong[0])]:.6f}"
    assert not outside, f"{name}: undecided draws outside `allowed` at {outside[:4]}"
    assert len(und) <= sr.CAP * got.size, f"{name}: {len(und)} of {got.size} draws undecided"


def run(case):
    rows = case.rows()
    got, _ = launch(case, rows)
    pred = sc.predict(case, rows)
    hold(str(case), got, pred)
    return got, pred


# ------------------------------------------------------------------------------------------------------------- 2a: shapes
def test_shape_table_reaches_every_instantiation_and_part_count():
    paths = [sc.launch_path(V) for V in sc.SHAPES_2A]
    assert {p[0] for p in paths} == {1, 2, 4, 8, 16} and {p[1] for p in paths} == {1, 2, 3, 4}
    assert max(sc.SHAPES_2A) == sc.MAX_PARTS * sc.PART_MAX                # the largest row the ABI takes
    assert sum(1 for V in sc.SHAPES_2A if V // 8 < 50) >= 2              # fewer threads with data than k


@pytest.mark.parametrize("V", sc.SHAPES_2A)
def test_every_shape_draws_the_predicted_tokens(V):
    case = sc.shape_case(V)
    got, pred = run(case)
    for row, ids in case.planted:                       # every boundary id: drawn by the reference, hence by the kernel
        for i in ids:
            assert (pred.tokens[:, row] == i).any(), (V, i, "the reference never draws it")
            assert (got[:, row] == i).any(), (V, i)
    assert got.max() < V


# --------------------------------------------------------------------------------------------------------- 2b: parameters
@pytest.mark.parametrize("case", sc.param_cases(), ids=str)
def test_parameters(case):
    run(case)


# -------------------------------------------------------------------------------------------------------- 2c: row contents
@pytest.mark.parametrize("V", [8000, 128256, 151552])
def test_row_contents(V):
    case, names = sc.content_cases(V)
    got, pred = run(case)
    rows = case.rows()
    r = names.index("all equal")
    assert pred.winners[r].tolist() == list(range(64))
    r = names.index("3 finite")
    assert len(pred.winners[r]) == 64 and bool(torch.isfinite(rows[r].float()[torch.as_tensor(got[:, r])]).all())
    for name, kept in (("40 leaders 20 tied", 20), ("40 leaders 54 tied", 24)):
        r = names.index(name)
        tied = (rows[r].float() == 5.0).nonzero().flatten().tolist()
        assert pred.winners[r][40:].tolist() == tied[:kept]              # the lowest ids, counted across the parts
        kept = sr.nucleus(sr.scaled(rows[r], pred.winners[r], case.T).astype(np.float64), case.top_p)[0]
        assert kept[40:].any() and not kept[40:].all()                   # the nucleus ends inside the ties: their order by id decides
    r = names.index("50 leaders in one slice, 3000 tied below")
    assert len(pred.winners[r]) == 50


# ------------------------------------------------------------------------------------------------------ 2d: range maxima
@pytest.mark.parametrize("case", sc.range_cases(), ids=str)
def test_range_maxima_path(case):
    rows = case.rows()
    V = rows.shape[1]
    got, pred = run(case)
    if "fallback" in str(case):
        k = sc.range_keys(rows)
        for b in range(rows.shape[0]):                  # more ranges reach the k-th range maximum than the buffer holds
            assert int((k[b] >= k[b].sort(descending=True).values[case.k - 1]).sum()) > sc.SMP_CAND // 16
        return
    for b in range(rows.shape[0]):                      # by the reference: the last range's leader is drawn, and several other
        want = pred.tokens[:, b]                        # tokens from ranges all over the row - hence by the kernel
        assert (want >= V - 16).any() and len(set(want[want < V - 16].tolist())) >= 4, (str(case), b, sorted(set(want.tolist())))
        assert np.isfinite(pred.ratio[:, b]).all()      # more than one rank is kept
        assert (got[:, b] >= V - 16).any() and (got[:, b] < V - 16).any()


# --------------------------------------------------------------------------------------------------- 2e: nucleus boundary
@pytest.mark.parametrize("n", [4, 8, 16])
def test_exact_nucleus_boundary(n):
    """n equal logits, T = 1: p = 1 / n and every partial sum are exact in f32, so top_p = j / n keeps exactly the j + 1 lowest
    ids and top_p = j / n - 2^-20 exactly j - no edge allowance."""
    rows, ids = sc.nucleus_rows(n)
    for case in sc.nucleus_cases(n):
        assert float(np.float32(case.top_p)) == case.top_p
        got, pred = run(case)
        rank = np.array([[ids[b].index(int(t)) if int(t) in ids[b] else -1 for b, t in enumerate(line)] for line in got])
        assert set(np.unique(rank).tolist()) == set(range(case.keep)), (str(case), np.unique(rank))


# --------------------------------------------------------------------------------------------------- 2f: skv_sample_advance
@pytest.mark.parametrize("variant", sc.sorted_variants(), ids=sc.sorted_name)
def test_sample_advance_draws_the_predicted_tokens(variant):
    _lib, Lb, st = _L()
    k, bs, L, var = variant
    vals, idx, pos0, var, pred = sc.predict_sorted_variant(*variant)
    name = f"sorted-k{k}-bs{bs}-" + "-".join(f"{a}{b}" for a, b in var.items())
    vd, idd = torch.from_numpy(vals).to(DEV), torch.from_numpy(idx).to(DEV)
    c = Counters(pos0)
    hits_in, hits = torch.arange(300, dtype=torch.int32, device=DEV), _guarded([11])
    out = []
    for _ in range(L):
        rc = Lb.skv_sample_advance(_lib.ptr(vd), _lib.ptr(idd), bs, k, var["top_p"], var["seed"], *c.args(_lib), _lib.ptr(hits_in),
                                   300, _lib.ptr(hits), st)
        assert rc == 0, (name, rc)
        out.append(c.token[:bs].clone())
    torch.cuda.synchronize()
    c.check(L, name)                                                     # (step_idx wraps at the table's 7 rows)
    assert hits.tolist() == [11 + L * sum(range(300)), GUARD], name      # hit_cnts summed once per launch
    hold(name, torch.stack(out).cpu().numpy(), pred)


# ------------------------------------------------------------------------------------------------- 2g: the Python wrapper
def _wrapper_tokens(rows, n, **kw):
    from shadowkv_amd import tensor_op
    out = []
    for _ in range(n):
        t = tensor_op.sample_token_native(rows, 0.6, 50, 0.9, **kw)
        assert t is not None
        out.append(t.flatten().clone())
    torch.cuda.synchronize()
    return torch.stack(out).cpu().numpy()


def test_wrapper_counts_positions_per_state_and_seed():
    from shadowkv_amd import tensor_op
    rows = sc.random_rows(32000, 3)
    x, keys = device_rows(rows), device_keys(rows)

    def want(seed, pos0, n, name):
        return sc.predict(sc.Case(name, lambda: rows, seed=seed, pos0=pos0, pos_stride=0, L=n), rows)

    old = torch.initial_seed()
    try:
        a, b = {}, {}
        hold("wrapper seed 7, calls 0..11", _wrapper_tokens(x, 12, seed=7, state=a), want(7, 0, 12, "w"))
        hold("wrapper seed 7, calls 12..19, ranges", _wrapper_tokens(x, 8, seed=7, state=a, range_max=keys), want(7, 12, 8, "w"))
        hold("wrapper second state", _wrapper_tokens(x, 6, seed=7, state=b, range_max=keys), want(7, 0, 6, "w"))       # independent
        hold("wrapper new seed restarts", _wrapper_tokens(x, 6, seed=2 ** 40 + 9, state=a), want(2 ** 40 + 9, 0, 6, "w"))
        tensor_op.set_sampler_seed(None)
        torch.manual_seed(4321)                                                                  # seed None: torch's seed
        hold("wrapper torch.manual_seed", _wrapper_tokens(x, 6, state=a), want(4321, 0, 6, "w"))
        tensor_op.set_sampler_seed(99)                                                           # ... unless one is set
        hold("wrapper set_sampler_seed", _wrapper_tokens(x, 6, state=a), want(99, 0, 6, "w"))
        hold("wrapper set_sampler_seed goes on", _wrapper_tokens(x, 4, state=a, range_max=keys), want(99, 6, 4, "w"))
    finally:
        tensor_op.set_sampler_seed(None)
        torch.manual_seed(old)


def test_captured_decode_steps_emit_the_predicted_tokens():
    """GraphDecoder on the two-layer config of test_decode_with_range_maxima_draws_the_same_tokens, 10 replays: the logits of the
    captured lm_head launch (the tensor forward_fused returned during capture, rewritten by every replay) predict every token."""
    from shadowkv_amd import llama
    cfg = llama.ModelConfig(name="h4096", hidden_size=4096, intermediate_size=2048, num_hidden_layers=2,
                            num_attention_heads=32, num_key_value_heads=8, vocab_size=32000)
    m = llama.DecoderLM(cfg=cfg, batch_size=1, max_length=4608, device=DEV, sparse_budget=256, rank=160, chunk_size=8,
                        seed=5, chunk_layout="inplace", overlap_attention=True)
    llama.build_synthetic_context(m, 4608, seed=77)
    dec = llama.GraphDecoder(m, temperature=0.8, walk_table=llama.make_walk_table(m, 10, seed=3))
    dec.token.copy_(torch.tensor([[17]], device=DEV))
    seen, inner = [], m.forward_fused

    def spy(*a, **kw):
        seen.append(inner(*a, **kw))
        return seen[-1]

    m.forward_fused = spy
    dec.capture(warmup=2)
    m.forward_fused = inner
    logits = seen[-1]
    decided = 0
    for step in range(10):
        pos = int(dec.pos[0, 0])
        tok = int(dec.step())
        row = logits[:, -1, :].cpu()
        want, sure, allowed = sr.draw(row[0], 50, 0.8, 0.9, dec.seed, pos, 0)
        print(f"SAMPLER captured step {step}: position {pos}  token {tok}  reference {want}  decided {sure}")
        assert tok == want if sure else tok in allowed, (step, tok, want, allowed)
        assert int(dec.pos[0, 0]) == pos + 1
        decided += sure
    assert 10 - decided <= sr.CAP * 10
