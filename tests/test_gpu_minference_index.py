"""GPU: the vertical + slash index estimate (tensor_op.vertical_slash_scores / vertical_slash_indices -> skv_vs_estimate)
against the f64 restatement of DESIGN.md section 9 (tests/minference_ref.py): the scores within an f32 bound, the kept sets
equal up to near-ties (in the manner of tests/util.check_topk_against_reference), determinism, planted structure, and the
fixed sets of stream_llm heads."""
import pytest
import torch

from minference_ref import check_topk_sets, scores_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _op():
    from shadowkv_amd import tensor_op
    return tensor_op


def _qk(bs, Hq, Hkv, L, seed, qs=0.08):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    q = (torch.randn(bs, Hq, L, 128, device=DEV, generator=gen) * qs).bfloat16()
    k = torch.randn(bs, Hkv, L, 128, device=DEV, generator=gen).bfloat16()
    return q, k


def _close(got, ref, what):
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isinf(got), ~fin), f"{what}: forced +inf entries differ"
    err = (got.double()[fin] - ref[fin]).abs()
    tol = 2e-5 * ref[fin].abs() + 1e-7
    assert not bool((err > tol).any()), f"{what}: worst excess {float((err - tol).max()):.3g}"


@pytest.mark.parametrize("L", [2, 63, 64, 65, 130, 1000, 4113, 9000])
def test_scores_against_restatement(L):
    q, k = _qk(2, 8, 2, L, L)
    c, d = _op().vertical_slash_scores(q, k)
    torch.cuda.synchronize()
    assert c.shape == d.shape == (2, 8, L) and c.dtype == torch.float32
    cr, dr = scores_ref(q, k)
    _close(c, cr, f"c L={L}")
    _close(d, dr, f"d L={L}")
    # each of the m rows is a distribution: the finite mass of c and d is m minus what the forced entries hide
    m = min(64, L)
    assert float(cr.nan_to_num(posinf=0).sum(-1).max()) <= m + 1e-6


def test_scores_on_strided_views():
    bs, L, Hq, Hkv, D = 1, 3000, 8, 2, 128
    gen = torch.Generator(device=DEV).manual_seed(2)
    qkv = (torch.randn(bs, L, (Hq + 2 * Hkv) * D, device=DEV, generator=gen) * 0.1).bfloat16()
    q = qkv[..., :Hq * D].view(bs, L, Hq, D).transpose(1, 2)
    k = qkv[..., Hq * D:(Hq + Hkv) * D].view(bs, L, Hkv, D).transpose(1, 2)
    a = _op().vertical_slash_scores(q, k)
    b = _op().vertical_slash_scores(q.contiguous(), k.contiguous())
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("L", [130, 1000, 4113, 9000])
def test_sets_against_restatement(L):
    Hq = 8
    q, k = _qk(1, Hq, 2, L, 10 + L)
    vsz = [30, 40, 100, 250, 500, 31, 64, 1000]
    ssz = [50, 100, 120, 300, 700, 101, 2000, 64]
    vi, si = _op().vertical_slash_indices(q, k, vsz, ssz)
    torch.cuda.synchronize()
    cr, dr = scores_ref(q, k)
    for h in range(Hq):
        nv, ns = min(L, max(vsz[h], 30)), min(L, max(ssz[h], 50))
        assert bool((vi[0, h, 1:] >= vi[0, h, :-1]).all()) and bool((si[0, h, 1:] >= si[0, h, :-1]).all())
        check_topk_sets(cr[0, h].cpu(), vi[0, h].cpu(), nv, f"vertical L={L} head {h}")
        if ns >= 100:                 # below 100 the forced offsets tie at +inf: any 50 .. 99 of them are valid
            check_topk_sets(dr[0, h].cpu(), si[0, h].cpu(), ns, f"slash L={L} head {h}")
        else:
            got = si[0, h][si[0, h] < L].cpu()
            assert got.numel() == ns and bool((got < min(L, 100)).all())


def test_forced_sinks_and_local_offsets_are_always_kept():
    L = 6000
    q, k = _qk(1, 4, 1, L, 3, qs=0.5)
    # make other columns / diagonals dominate: the forced entries must still be kept
    k[0, 0, 3000:3010] = q[0, 0, -1:] * 40
    vi, si = _op().vertical_slash_indices(q, k, [30, 200, 1000, 30], [100, 150, 400, 6096])
    torch.cuda.synchronize()
    for h in range(4):
        v = set(vi[0, h].tolist())
        s = set(si[0, h].tolist())
        assert set(range(30)) <= v, h
        assert set(range(100)) <= s, h


def test_two_runs_are_bit_identical():
    L = 20000
    q, k = _qk(2, 8, 2, L, 4)
    c1, d1 = _op().vertical_slash_scores(q, k)
    c2, d2 = _op().vertical_slash_scores(q, k)
    v1, s1 = _op().vertical_slash_indices(q, k, 1000, 6096)
    v2, s2 = _op().vertical_slash_indices(q, k, 1000, 6096)
    torch.cuda.synchronize()
    assert torch.equal(c1.view(torch.int32), c2.view(torch.int32)) and torch.equal(d1.view(torch.int32), d2.view(torch.int32))
    assert torch.equal(v1, v2) and torch.equal(s1, s2)


def test_planted_structure_is_recovered():
    """Keys built so that a few columns and a few diagonals dominate the last 64 queries are the ones selected."""
    L, D = 8000, 128
    gen = torch.Generator(device=DEV).manual_seed(8)
    base = torch.randn(D, device=DEV, generator=gen)
    base = base / base.norm()
    qf = torch.randn(L, D, device=DEV, generator=gen) * 0.5 + base * 2.0      # a shared direction plus a per-row one
    kf = torch.randn(L, D, device=DEV, generator=gen) * 0.02
    cols = [777, 2500, 5123, 7000]
    kf[cols] = base * 6.0                                   # q . k ~ 12 for every query: vertical lines
    offs = [1234, 3333, 6000]
    rows = torch.arange(L - 64, L, device=DEV)
    for s in offs:                                          # key r - s scores ~12 for query r only: a diagonal
        qr = qf[rows]
        kf[rows - s] = qr * (12.0 / (qr * qr).sum(-1, keepdim=True))
    q, k = qf.bfloat16().view(1, 1, L, D), kf.bfloat16().view(1, 1, L, D)
    vi, si = _op().vertical_slash_indices(q, k, 34, 103)
    torch.cuda.synchronize()
    v, s = set(vi[0, 0].tolist()), set(si[0, 0].tolist())
    assert v == set(range(30)) | set(cols), sorted(v - set(range(30)))
    assert s == set(range(100)) | set(offs), sorted(s - set(range(100)))


def test_stream_llm_heads_get_fixed_sets():
    L = 3000
    q, k = _qk(1, 8, 2, L, 6)
    pat = {h: ("stream_llm", 4 + h, 50 + 10 * h, 1) for h in range(8)}
    pat[3] = ("vertical_and_slash", 100, 200, 1)
    vi, si = _op().minference_index_sets(q, k, pat)
    torch.cuda.synchronize()
    for h in range(8):
        v = [x for x in vi[0, h].tolist() if x < L]
        s = [x for x in si[0, h].tolist() if x < L]
        if h == 3:
            assert len(v) == 100 and len(s) == 200 and set(range(30)) <= set(v) and set(range(100)) <= set(s)
        else:
            assert v == list(range(4 + h)) and s == list(range(50 + 10 * h))
    # a layer of stream_llm heads only runs no estimate, and sizes beyond L are cut at L by the kernel
    vi2, si2 = _op().minference_index_sets(q[:, :, :40], k[:, :, :40], {h: ("stream_llm", 128, 4096, 1) for h in range(8)})
    torch.cuda.synchronize()
    assert vi2.shape[-1] == 128 and si2.shape[-1] == 4096 and bool((vi2[0, 0] == torch.arange(128, device=DEV)).all())
