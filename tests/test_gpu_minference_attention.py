"""GPU: the vertical + slash sparse prefill attention (tensor_op.sparse_prefill_attention -> skv_vs_sparse_attention) against
an f64 restatement of the window mask of DESIGN.md section 9 (tests/minference_ref.py), with the bound of
tests/util.attention_tolerance: 1e-3 |ref| plus the bf16 output rounding, and the error model of softmax weights rounded to
bf16 with the weight term taken at its worst case, 2^-8 relative per weight (half an ulp just above a power of two) rather
than 2^-9: with a few attended keys per row the roundings do not average out.  tests/test_gpu_prefill_attention.py bounds the
dense kernel the same way."""

import pytest
import torch

from minference_ref import attention_ref, block_coverage, window_mask
from util import attention_tolerance

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _op():
    from shadowkv_amd import tensor_op
    return tensor_op


def _rand(shape, gen, scale=1.0):
    return (torch.randn(*shape, device=DEV, generator=gen) * scale).to(torch.bfloat16)


def assert_close(got, ref, absv, what=""):
    tol = attention_tolerance(ref) + 2.0 ** -8 * absv
    err = (got.double() - ref).abs()
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements over the bound, worst excess {float((err - tol).max()):.3g}"


def _lists(bs, Hq, L, gen, kind, device=DEV):
    """Per-head index lists of different sizes (padded with entries >= L, which the kernel ignores)."""
    vs, ss = [], []
    for h in range(Hq):
        nv = 1 + (7 * h + 3) % max(1, min(L, 90))
        ns = 1 + (11 * h + 5) % max(1, min(L, 70))
        if kind == "random":
            v = torch.randint(0, L, (nv,), generator=gen)
            s = torch.randint(0, L, (ns,), generator=gen)
        elif kind == "clustered":                              # runs of neighbouring offsets / columns: merged windows
            v = (torch.randint(0, L, (1,), generator=gen) + torch.arange(nv)) % L
            s = torch.cat([torch.arange(min(ns, L)), (L // 2 + torch.arange(ns)) % L])
        else:                                                  # duplicated entries, shuffled
            v = torch.randint(0, L, (max(1, nv // 3),), generator=gen).repeat(3)
            s = torch.randint(0, L, (max(1, ns // 3),), generator=gen).repeat(3)
        vs.append(v[torch.randperm(v.numel(), generator=gen)])
        ss.append(s[torch.randperm(s.numel(), generator=gen)])
    pad = lambda xs: torch.stack([torch.cat([x, torch.full((max(map(len, xs)) - len(x),), 2 ** 31 - 1)]) for x in xs])  # noqa
    v, s = pad(vs), pad(ss)
    return v.expand(bs, -1, -1).contiguous().to(device), s.expand(bs, -1, -1).contiguous().to(device)


@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("G", [4, 8])
@pytest.mark.parametrize("L", [2, 63, 64, 65, 1000, 4113])
def test_against_restatement(L, G, bs):
    gen_cpu = torch.Generator().manual_seed(31 * L + G + bs)
    gen = torch.Generator(device=DEV).manual_seed(17 * L + G + bs)
    Hkv = 2 if G == 4 else 1
    Hq = G * Hkv
    q = _rand((bs, Hq, L, 128), gen, 1.5)
    k = _rand((bs, Hkv, L, 128), gen)
    v = _rand((bs, Hkv, L, 128), gen)
    for kind in ("random", "clustered", "duplicated"):
        vi, si = _lists(bs, Hq, L, gen_cpu, kind)
        if bs == 2:                                        # the sequences get different lists
            vi[1] = vi[1].flip(-1)
            si[1] = torch.where(si[1] < L, (si[1] + 1) % L, si[1])
        out = _op().sparse_prefill_attention(q, k, v, vi, si)
        torch.cuda.synchronize()
        assert out.shape == (bs, L, Hq, 128) and out.is_contiguous()
        ref, absv = attention_ref(q, k, v, vi, si)
        assert_close(out, ref, absv, f"L={L} G={G} bs={bs} {kind}")


def test_long_prompt_sampled_rows():
    L, Hkv, G = 32768, 2, 4
    gen = torch.Generator(device=DEV).manual_seed(5)
    gc = torch.Generator().manual_seed(5)
    q, k, v = _rand((1, Hkv * G, L, 128), gen, 1.5), _rand((1, Hkv, L, 128), gen), _rand((1, Hkv, L, 128), gen)
    vi = torch.stack([torch.cat([torch.arange(30), torch.randint(0, L, (200 + 50 * h,), generator=gc)]).narrow(0, 0, 230)
                      for h in range(8)]).unsqueeze(0).to(DEV)
    si = torch.stack([torch.cat([torch.arange(100), torch.randint(0, L, (300,), generator=gc)]) for _ in range(8)])
    si = si.unsqueeze(0).to(DEV)
    out = _op().sparse_prefill_attention(q, k, v, vi, si)
    rows = torch.cat([torch.arange(0, 70), torch.randint(0, L, (120,), generator=gc), torch.arange(L - 66, L)])
    torch.cuda.synchronize()
    ref, absv = attention_ref(q, k, v, vi, si, rows)
    assert_close(out[:, rows.to(DEV)], ref, absv, "L=32768")


@pytest.mark.parametrize("L", [65, 1000, 4113])
def test_full_coverage_is_dense_causal(L):
    gen = torch.Generator(device=DEV).manual_seed(L)
    q, k, v = _rand((2, 8, L, 128), gen, 1.5), _rand((2, 2, L, 128), gen), _rand((2, 2, L, 128), gen)
    si = torch.arange(L, device=DEV).view(1, 1, -1).expand(2, 8, -1)
    vi = torch.zeros(2, 8, 1, dtype=torch.int64, device=DEV)
    out = _op().sparse_prefill_attention(q, k, v, vi, si)
    dense = _op().causal_attention_prefill(q, k, v)
    torch.cuda.synchronize()
    ref, absv = attention_ref(q, k, v, vi, si)
    assert_close(out, ref, absv, f"full coverage L={L}")
    assert_close(dense, ref, absv, f"dense L={L}")
    assert float((out.float() - dense.float()).abs().max()) <= 2 * float((attention_tolerance(ref) + 2.0 ** -8 * absv).max())


def test_mask_is_bit_exact():
    """Replacing K and V at every key that no row of a block attends leaves that block's rows bit-identical."""
    L, Hq, Hkv = 1000, 4, 1
    gen = torch.Generator(device=DEV).manual_seed(77)
    gc = torch.Generator().manual_seed(77)
    q, k, v = _rand((1, Hq, L, 128), gen, 1.5), _rand((1, Hkv, L, 128), gen), _rand((1, Hkv, L, 128), gen)
    vi = torch.randint(0, L, (1, 1, 40), generator=gc).expand(1, Hq, -1).contiguous().to(DEV)
    si = torch.cat([torch.tensor([0, 1, 2]), torch.randint(0, L, (25,), generator=gc)]).view(1, 1, -1).expand(1, Hq, -1)
    si = si.contiguous().to(DEV)
    out = _op().sparse_prefill_attention(q, k, v, vi, si)
    cov = block_coverage(L, si[0, 0].cpu())
    vert = torch.zeros(L, dtype=torch.bool)
    vert[vi[0, 0].cpu()] = True
    for blk in (0, 3, 9, 15):
        rows = torch.arange(64 * blk, min(L, 64 * blk + 64))
        used = window_mask(L, vi[0, 0].cpu(), si[0, 0].cpu(), rows).any(0)
        assert torch.equal(used, (cov[blk] | vert) & (torch.arange(L) <= int(rows[-1])))
        unused = (~used).to(DEV)
        k2, v2 = k.clone(), v.clone()
        k2[:, :, unused] = _rand((1, Hkv, int(unused.sum()), 128), gen, 4.0)
        v2[:, :, unused] = _rand((1, Hkv, int(unused.sum()), 128), gen, 4.0)
        out2 = _op().sparse_prefill_attention(q, k2, v2, vi, si)
        torch.cuda.synchronize()
        r = rows.to(DEV)
        assert torch.equal(out[:, r].view(torch.int16), out2[:, r].view(torch.int16)), f"block {blk}"


def test_default_sizes_at_124928():
    """256 rows of a 124,928-token prompt with MInference's default sizes (1,000 columns, 6,096 offsets)."""
    L, Hkv, G = 124928, 1, 4
    gen = torch.Generator(device=DEV).manual_seed(9)
    gc = torch.Generator().manual_seed(9)
    q, k, v = _rand((1, G, L, 128), gen, 1.5), _rand((1, Hkv, L, 128), gen), _rand((1, Hkv, L, 128), gen)
    vi = torch.stack([torch.cat([torch.arange(30), torch.randperm(L - 30, generator=gc)[:970] + 30]) for _ in range(G)])
    si = torch.stack([torch.cat([torch.arange(100), torch.randperm(L - 100, generator=gc)[:5996] + 100]) for _ in range(G)])
    vi, si = vi.unsqueeze(0).to(DEV), si.unsqueeze(0).to(DEV)
    out = _op().sparse_prefill_attention(q, k, v, vi, si)
    rows = torch.cat([torch.arange(0, 64), torch.randint(64, L - 64, (128,), generator=gc), torch.arange(L - 64, L)])
    torch.cuda.synchronize()
    ref, absv = attention_ref(q, k, v, vi, si, rows)
    assert_close(out[:, rows.to(DEV)], ref, absv, "L=124928")


def test_strided_views_as_prefill_layer_passes_them():
    """q / k / v transpose views of a fused QKV projection output [bs, L, (Hq + 2 Hkv) D]: no copy needed."""
    bs, L, Hq, Hkv, D = 2, 777, 8, 2, 128
    gen = torch.Generator(device=DEV).manual_seed(3)
    gc = torch.Generator().manual_seed(3)
    qkv = _rand((bs, L, (Hq + 2 * Hkv) * D), gen)
    q = qkv[..., :Hq * D].view(bs, L, Hq, D).transpose(1, 2)
    k = qkv[..., Hq * D:(Hq + Hkv) * D].view(bs, L, Hkv, D).transpose(1, 2)
    v = qkv[..., (Hq + Hkv) * D:].view(bs, L, Hkv, D).transpose(1, 2)
    vi, si = _lists(bs, Hq, L, gc, "random")
    out = _op().sparse_prefill_attention(q, k, v, vi, si)
    ref_c = _op().sparse_prefill_attention(q.contiguous(), k.contiguous(), v.contiguous(), vi, si)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), ref_c.view(torch.int16))
    ref, absv = attention_ref(q, k, v, vi, si)
    assert_close(out, ref, absv, "strided")
