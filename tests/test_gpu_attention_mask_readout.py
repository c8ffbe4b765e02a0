"""GPU: the exact attended-key set of both prefill attention kernels, read out of their bf16 output with the probe inputs of
tests/attn_probe.py (DESIGN.md sections 8 and 9): for every (sequence, head, row, key) the decoded mask equals the contract's
under torch.equal, every attended key counts once, every empty row is +0 bits.  No tolerance: the arithmetic is held by
test_gpu_prefill_attention.py / test_gpu_minference_attention.py, the membership here.

Dense (skv_prefill_attn_kernel, csrc/skv_prefill_attn.hip): the conditions read out are `key <= lim` (lim = off + qi),
`key0 > wave_hi` (tiles skipped above a wave), `key0 + FT_KB - 1 > wave_lo` (masked or not) and n_tiles; the lengths sit
around the 32-row wave, the 64-key tile and the 128-row workgroup, the continuations move `off` across them.
Sparse (vs_attn_kernel, csrc/skv_minference.hip): attn_probe.sparse_families names the condition next to each family."""
import pytest
import torch

import attn_probe as ap
from minference_ref import window_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 2 ** 31 - 1


def _op():
    from shadowkv_amd import tensor_op
    return tensor_op


# ------------------------------------------------------------------------------------------------------------- dense
def dense_read_out(q_len, kv_len, G, bs=1, Hkv=None, seed=0, views=None):
    Hkv = (2 if G == 4 else 1) if Hkv is None else Hkv
    probe = ap.Probe(kv_len, q_len, bs=bs, Hq=G * Hkv, Hkv=Hkv, device=DEV, seed=seed, seq_shift=1)
    for s in range(probe.C):
        q, k, v = probe.inputs(s)
        if views is not None:
            q, k, v = views(q, k, v)
        out = _op().causal_attention_prefill(q, k, v)
        probe.read(s, out)
    torch.cuda.synchronize()
    pairs = ap.check(probe, lambda b, h, r0, r1: ap.causal_mask(q_len, kv_len, r0, r1, DEV))
    assert pairs == bs * G * Hkv * sum(kv_len - q_len + i + 1 for i in range(q_len))


# `key <= lim` on the diagonal tile, `key0 > wave_hi` (a wave skips the tiles above its last row) and `key0 + FT_KB - 1 >
# wave_lo` (mask or ft_scale_unmasked): lengths on both sides of the 32-row wave, the 64-key tile and the 128-row workgroup
# (`row_ok`, `wave_on`, n_tiles of a partial last block); 300 and 1000 are several workgroups with C = 3 and 8
@pytest.mark.parametrize("G", [4, 8])
@pytest.mark.parametrize("S", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300, 1000])
def test_dense_prompt(S, G):
    dense_read_out(S, S, G, seed=S + G)


# n_tiles = 65 and a last workgroup of one row (`wave_on` false for waves 1 .. 3)
def test_dense_prompt_4097():
    dense_read_out(4097, 4097, 4, Hkv=1, seed=1)            # C = 33


# `off = kv_len - q_len` moves the diagonal inside the tile: `lim = off + qi`, `wave_lo` / `wave_hi` and
# `n_tiles = (off + min(q0 + PF_QB, q_len) - 1) / FT_KB + 1` at off = 1, 63, 64, 65 and off not a multiple of anything
@pytest.mark.parametrize("G", [4, 8])
@pytest.mark.parametrize("past, new", [(1, 1), (63, 65), (64, 64), (65, 130), (333, 200), (3000, 130)])
def test_dense_continuation(past, new, G):
    dense_read_out(new, past + new, G, seed=past + G)


# `hk = hq / G` for a G that is no power of two, and G = 1
@pytest.mark.parametrize("G", [1, 7])
def test_dense_any_group_size(G):
    dense_read_out(300, 300, G, Hkv=2, seed=G)


# `bh = blockIdx.x % nbh`, `b = bh / Hq`: the sequences hold different inputs and probe different classes
@pytest.mark.parametrize("q_len, kv_len", [(300, 300), (130, 195)])
def test_dense_two_sequences(q_len, kv_len):
    dense_read_out(q_len, kv_len, 4, bs=2, seed=5)          # the second sequence probes other classes (seq_shift)


# the qsb / qsh / qss, ksb .. vss strides of ft_load_q and ft_load_tile
def test_dense_on_strided_views():
    """The views of test_continuation_on_strided_views: K a slice of a larger cache buffer, Q and V transpose views of a fused
    QKV output."""
    past, new, Hq, Hkv, bs = 333, 200, 8, 2, 2
    L = past + new

    def views(q, k, v):
        buf = torch.full((bs, Hkv, L + 517, 128), 64.0, dtype=torch.bfloat16, device=DEV)       # rows >= L: never read
        buf[:, :, :L] = k
        qkv = torch.full((bs, L, (Hq + 2 * Hkv) * 128), 1.0, dtype=torch.bfloat16, device=DEV)
        qkv[:, past:, :Hq * 128] = q.transpose(1, 2).reshape(bs, new, Hq * 128)
        qkv[..., (Hq + Hkv) * 128:] = v.transpose(1, 2).reshape(bs, L, Hkv * 128)
        k2 = buf[:, :, :L]
        v2 = qkv[..., (Hq + Hkv) * 128:].view(bs, L, Hkv, 128).transpose(1, 2)
        q2 = qkv[:, past:, :Hq * 128].view(bs, new, Hq, 128).transpose(1, 2)
        assert not k2.is_contiguous() and not v2.is_contiguous() and not q2.is_contiguous()
        return q2, k2, v2

    dense_read_out(new, L, 4, bs=bs, Hkv=Hkv, seed=9, views=views)


# ------------------------------------------------------------------------------------------------------------ sparse
def _pad(lists, n=None):
    n = max(len(x) for x in lists) if n is None else n
    return torch.tensor([list(x) + [PAD] * (n - len(x)) for x in lists], dtype=torch.int64)


def sparse_read_out(L, heads, seed=0, slab=512):
    """heads: per sequence, per query head (slash list, vertical list); all heads over one KV head."""
    bs, Hq = len(heads), len(heads[0])
    ns, nv = (max(len(h[i]) for seq in heads for h in seq) for i in (0, 1))
    si = torch.stack([_pad([h[0] for h in seq], ns) for seq in heads])
    vi = torch.stack([_pad([h[1] for h in seq], nv) for seq in heads])
    probe = ap.Probe(L, bs=bs, Hq=Hq, Hkv=1, device=DEV, seed=seed, seq_shift=1)
    si_dev, vi_dev = si.to(DEV), vi.to(DEV)
    for s in range(probe.C):
        q, k, v = probe.inputs(s)
        probe.read(s, _op().sparse_prefill_attention(q, k, v, vi_dev, si_dev))
    torch.cuda.synchronize()
    return ap.check(probe, lambda b, h, r0, r1: window_mask(L, vi[b, h], si[b, h], rows=torch.arange(r0, r1)), slab=slab)


def _groups(L, starred=False):
    fam = ap.sparse_families(L, starred)
    fam += fam[:(-len(fam)) % 4]
    return [fam[i:i + 4] for i in range(0, len(fam), 4)]


def _cases():
    out = []
    for L in (2, 63, 64, 65, 130, 1000):
        out += [pytest.param(L, False, g, id=f"{L}-" + "+".join(f[0] for f in _groups(L)[g])) for g in range(len(_groups(L)))]
    out += [pytest.param(4113, True, g, id="4113-" + "+".join(f[0] for f in _groups(4113, True)[g]))
            for g in range(len(_groups(4113, True)))]
    return out


@pytest.mark.parametrize("L, starred, group", _cases())
def test_sparse_families(L, starred, group):
    """Hq = 4 over one KV head, a different (slash, vertical) family per head."""
    fam = _groups(L, starred)[group]
    pairs = sparse_read_out(L, [[(s, v) for _, s, v in fam]], seed=L + group)
    if all(name == "nothing" for name, _, _ in fam):
        assert pairs == 0


def test_sparse_empty_rows_are_zero_bits():
    """No valid offset and no valid column in any head: every row of the output is +0."""
    L = 130
    lists = [[-1, L] + ap.BIG, [-7], [L + 5, PAD], ap.BIG]
    vi = si = _pad(lists).unsqueeze(0).to(DEV)
    probe = ap.Probe(L, bs=1, Hq=4, Hkv=1, device=DEV)
    q, k, v = probe.inputs(0)
    out = torch.full((1, L, 4, 128), 3.0, dtype=torch.bfloat16, device=DEV)
    _op().sparse_prefill_attention(q, k, v, vi, si, out=out)
    torch.cuda.synchronize()
    assert not bool(out.view(torch.int16).any())


def test_sparse_two_sequences():
    """bs = 2: other lists, and other probed classes, in the second sequence."""
    L = 1000
    fam = {n: (s, v) for n, s, v in ap.sparse_families(L)}
    a = [fam[n] for n in ("run65", "cover-mixed", "dup-63-64", "v-late")]
    b = [fam[n] for n in ("edge-blast", "v129", "no-s0", "cover-s63")]
    sparse_read_out(L, [a, b], seed=2)


def test_sparse_default_sizes_scaled():
    """L = 8,192 (C = 64), MInference's default sizes scaled: 30 sinks + 470 random columns, offsets 0 .. 99 + 2,900 random;
    the full read-out, compared in slabs of rows on the device."""
    L, Hq = 8192, 4
    g = torch.Generator().manual_seed(8192)
    heads = [((list(range(100)) + (torch.randperm(L - 100, generator=g)[:2900] + 100).tolist()),
              (list(range(30)) + (torch.randperm(L - 30, generator=g)[:470] + 30).tolist())) for _ in range(Hq)]
    assert sparse_read_out(L, [heads], seed=4, slab=512) > 0
