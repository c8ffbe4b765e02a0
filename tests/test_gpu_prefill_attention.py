"""GPU: the causal GQA prefill attention kernel (tensor_op.causal_attention_prefill -> skv_prefill_attention) against an f64
PyTorch restatement of flash_attn_with_kvcache(causal=True): softmax(q k^T / sqrt(D)) v over the keys j <= kv_len - q_len + i.

Bound per element: 2^-8 |ref| + 2^-8 (P-weighted mean |V|) + 1e-5 - the bf16 output rounding plus the error model of softmax
weights rounded to bf16 before P.V (tests/util.attention_tolerance)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _op():
    from shadowkv_amd import tensor_op
    return tensor_op.causal_attention_prefill


def _rand(shape, gen, scale=1.0):
    return (torch.randn(*shape, device=DEV, generator=gen) * scale).to(torch.bfloat16)


def reference(q, k, v, rows=None):
    """f64 attention: (out [bs, n, Hq, D], absv [bs, n, Hq, D]) for query rows `rows` (default: all)."""
    bs, Hq, S, D = q.shape
    Hkv, L = k.shape[1], k.shape[2]
    G = Hq // Hkv
    off = L - S
    rows = torch.arange(S, device=q.device) if rows is None else rows.to(q.device)
    out = torch.empty(bs, rows.numel(), Hq, D, dtype=torch.float64, device=q.device)
    absv = torch.empty_like(out)
    keys = torch.arange(L, device=q.device)
    mask = keys.unsqueeze(0) > (off + rows).unsqueeze(1)
    for b in range(bs):
        for h in range(Hq):
            kh, vh = k[b, h // G].double(), v[b, h // G].double()
            s = (q[b, h, rows].double() @ kh.T) / math.sqrt(D)
            s.masked_fill_(mask, float("-inf"))
            p = torch.softmax(s, dim=-1)
            out[b, :, h] = p @ vh
            absv[b, :, h] = p @ vh.abs()
            del s, p
    return out, absv


def assert_close(got, ref, absv, what=""):
    tol = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * absv + 1e-5
    err = (got.double() - ref).abs()
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements over the bound, worst excess {float((err - tol).max()):.3g}"


LENGTHS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4097, 8191]


@pytest.mark.parametrize("bs", [1, 3])
@pytest.mark.parametrize("G", [4, 8])
@pytest.mark.parametrize("S", LENGTHS)
def test_prompt_lengths(S, G, bs):
    gen = torch.Generator(device=DEV).manual_seed(1000 * S + 10 * G + bs)
    Hkv = 2 if G == 4 else 1
    Hq = G * Hkv
    q = _rand((bs, Hq, S, 128), gen, 1.5)
    k = _rand((bs, Hkv, S, 128), gen)
    v = _rand((bs, Hkv, S, 128), gen)
    out = _op()(q, k, v)
    torch.cuda.synchronize()
    assert out.shape == (bs, S, Hq, 128) and out.is_contiguous()
    ref, absv = reference(q, k, v)
    assert_close(out, ref, absv, f"S={S} G={G} bs={bs}")
    # row 0 sees key 0 only: exactly V row 0
    want = v[:, :, 0].repeat_interleave(G, dim=1)
    assert torch.equal(out[:, 0].view(torch.int16), want.view(torch.int16))


def test_continuation_on_strided_views():
    """kv_len > q_len (1000 new rows on 3000 cached ones): K a slice of a larger cache buffer, V and Q transpose views of a
    fused QKV output, as the full-attention prefill passes them."""
    gen = torch.Generator(device=DEV).manual_seed(7)
    bs, Hq, Hkv, D, past, new = 2, 8, 2, 128, 3000, 1000
    L = past + new
    buf = _rand((bs, Hkv, L + 517, D), gen)
    k = buf[:, :, :L]
    qkv = _rand((bs, L, (Hq + 2 * Hkv) * D), gen)
    v = qkv[..., (Hq + Hkv) * D:].view(bs, L, Hkv, D).transpose(1, 2)
    q = (qkv[:, past:, :Hq * D] * 1.5).view(bs, new, Hq, D).transpose(1, 2)
    assert not k.is_contiguous() and not v.is_contiguous() and not q.is_contiguous()
    out = _op()(q, k, v)
    torch.cuda.synchronize()
    ref, absv = reference(q.contiguous(), k.contiguous(), v.contiguous())
    assert_close(out, ref, absv, "continuation")
    # the same through contiguous copies: bit for bit
    out2 = _op()(q.contiguous(), k.contiguous(), v.contiguous())
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))


def test_causality_is_bit_exact():
    """Rewriting K / V rows >= j leaves every output row whose last visible key is < j unchanged, bit for bit."""
    gen = torch.Generator(device=DEV).manual_seed(11)
    bs, Hq, Hkv, S = 1, 8, 2, 300
    q = _rand((bs, Hq, S, 128), gen, 1.5)
    k = _rand((bs, Hkv, S, 128), gen)
    v = _rand((bs, Hkv, S, 128), gen)
    base = _op()(q, k, v)
    for j in (1, 63, 64, 65, 127, 128, 129, 200, 299):
        k2, v2 = k.clone(), v.clone()
        k2[:, :, j:] = _rand(k2[:, :, j:].shape, gen, 3.0)
        v2[:, :, j:] = _rand(v2[:, :, j:].shape, gen, 3.0)
        out = _op()(q, k2, v2)
        torch.cuda.synchronize()
        assert torch.equal(out[:, :j].view(torch.int16), base[:, :j].view(torch.int16)), f"j={j}"
        assert not torch.equal(out[:, j:].view(torch.int16), base[:, j:].view(torch.int16)), f"j={j}: nothing changed"


def test_forced_rescale():
    """One K row aligned with one Q row makes that row's running maximum jump at a chosen late tile (the rescale of O and l
    must be complete and taken once); checked over the full tensor against the f64 reference."""
    gen = torch.Generator(device=DEV).manual_seed(13)
    bs, Hq, Hkv, S = 1, 8, 2, 1024
    q = _rand((bs, Hq, S, 128), gen, 0.5)
    k = _rand((bs, Hkv, S, 128), gen, 0.5)
    v = _rand((bs, Hkv, S, 128), gen)
    spikes = [(900, 700, 0), (1000, 960, 5), (300, 129, 2), (640, 64, 7)]     # (query row, key row, query head)
    for i, j, h in spikes:
        qi = q[0, h, i].float()
        k[0, h // 4, j] = (qi / qi.norm() * 40.0).to(torch.bfloat16)         # score ~ 40 |q| / sqrt(128) >> the rest
    out = _op()(q, k, v)
    torch.cuda.synchronize()
    ref, absv = reference(q, k, v)
    assert_close(out, ref, absv, "forced rescale")
    for i, j, h in spikes:          # the spiked rows really are dominated by the spike key
        assert float((ref[0, i, h] - v[0, h // 4, j].double()).abs().max()) < 0.1


def test_full_size_llama_shapes():
    """Llama-3.1-8B head set (32 query / 8 KV heads) at S = 124,928: 256+ sampled query rows, first and last tiles included."""
    gen = torch.Generator(device=DEV).manual_seed(17)
    S, Hq, Hkv = 124928, 32, 8
    q = _rand((1, Hq, S, 128), gen)
    k = _rand((1, Hkv, S, 128), gen)
    v = _rand((1, Hkv, S, 128), gen)
    out = _op()(q, k, v)
    torch.cuda.synchronize()
    fixed = torch.tensor([0, 1, 2, 31, 32, 63, 64, 65, 127, 128, 129, 255, S - 129, S - 128, S - 127, S - 65, S - 64, S - 63,
                          S - 2, S - 1])
    rnd = torch.randint(0, S, (240,), generator=torch.Generator().manual_seed(5))
    rows = torch.unique(torch.cat([fixed, rnd]))
    assert rows.numel() >= 256
    ref, absv = reference(q, k, v, rows)
    assert_close(out[:, rows.to(DEV)], ref, absv, "S=124928")


def test_batch_independence():
    gen = torch.Generator(device=DEV).manual_seed(19)
    bs, Hq, Hkv, S = 3, 8, 2, 777
    q = _rand((bs, Hq, S, 128), gen, 1.5)
    k = _rand((bs, Hkv, S, 128), gen)
    v = _rand((bs, Hkv, S, 128), gen)
    out3 = _op()(q, k, v)
    for b in range(bs):
        out1 = _op()(q[b:b + 1].clone(), k[b:b + 1].clone(), v[b:b + 1].clone())
        torch.cuda.synchronize()
        assert torch.equal(out3[b:b + 1].view(torch.int16), out1.view(torch.int16)), f"sequence {b}"


def test_bad_shapes_raise():
    gen = torch.Generator(device=DEV).manual_seed(23)
    q = _rand((1, 8, 64, 128), gen)
    k = _rand((1, 2, 64, 128), gen)
    with pytest.raises(ValueError):
        _op()(q, k[:, :, :32], k[:, :, :32])           # kv_len < q_len
    with pytest.raises(ValueError):
        _op()(q, _rand((1, 3, 64, 128), gen), _rand((1, 3, 64, 128), gen))   # 8 % 3
    with pytest.raises(ValueError):
        _op()(q, k, k[:, :, :, :64])                   # k / v shapes differ
