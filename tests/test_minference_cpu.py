"""CPU: the MInference sparse prefill's C ABI (part 6 of include/shadowkv_hip.h) is declared, bound and refuses bad arguments on
the host before any launch (-1 = SKV_ERR_ARG, -2 = SKV_ERR_UNSUPPORTED); DecoderLM's pattern handling; the vectorised window
mask the GPU tests use against a brute-force reading of the definition."""
import json
import os
import re

import pytest
import torch

from minference_ref import block_coverage, brute_mask, window_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("skv_vs_estimate", "skv_vs_sparse_attention", "skv_vs_estimate_workspace_bytes", "skv_vs_attention_workspace_bytes")


def test_exports_are_declared_and_bound():
    from shadowkv_amd import _lib
    text = open(os.path.join(ROOT, "include", "shadowkv_hip.h")).read()
    part6 = text[text.index("part 6"):]
    for name in NAMES:
        assert re.search(r"SKV_EXPORT\s+(int|long long)\s+" + name + r"\s*\(", part6), name
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib(), name) is not None
    assert _lib.lib().skv_abi_version() == 1


def test_workspace_sizes():
    from shadowkv_amd import _lib
    L = _lib.lib()
    assert L.skv_vs_estimate_workspace_bytes(1, 32, 124928) == 32 * 61 * 128 * 4
    assert L.skv_vs_attention_workspace_bytes(1, 32, 124928) == 32 * 3904 * 4
    assert L.skv_vs_attention_workspace_bytes(1, 32, 124928) < 64 * 2 ** 20
    assert L.skv_vs_estimate_workspace_bytes(0, 32, 100) == 0 and L.skv_vs_attention_workspace_bytes(1, 1, 0) == 0


P = 0x1000                                          # a non-null, aligned pointer that is never dereferenced on the host


def _strides(H, n, d=128):
    return (H * n * d, n * d, d)


def _est(**kw):
    from shadowkv_amd import _lib
    a = dict(q=P, k=P, c=P, d=P, ws=P, bs=1, hq=8, hkv=2, q_len=100, kv_len=100, hd=128,
             qs=_strides(8, 100), ks=_strides(2, 100))
    a.update(kw)
    return _lib.lib().skv_vs_estimate(a["q"], a["k"], a["c"], a["d"], a["ws"], a["bs"], a["hq"], a["hkv"], a["q_len"],
                                       a["kv_len"], a["hd"], *a["qs"], *a["ks"], 0)


def _attn(**kw):
    from shadowkv_amd import _lib
    a = dict(q=P, k=P, v=P, out=P, vi=P, si=P, ws=P, bs=1, hq=8, hkv=2, q_len=100, kv_len=100, hd=128, nv=10, ns=10,
             qs=_strides(8, 100), ks=_strides(2, 100), vs=_strides(2, 100))
    a.update(kw)
    return _lib.lib().skv_vs_sparse_attention(a["q"], a["k"], a["v"], a["out"], a["vi"], a["si"], a["ws"], a["bs"], a["hq"],
                                               a["hkv"], a["q_len"], a["kv_len"], a["hd"], a["nv"], a["ns"], *a["qs"],
                                               *a["ks"], *a["vs"], 0.088, 0)


def test_estimate_refuses_bad_arguments_before_any_launch():
    for name in ("q", "k", "c", "d", "ws"):
        assert _est(**{name: 0}) == -1, name
    assert _est(bs=0) == -1
    assert _est(hq=0) == -1 and _est(hkv=0) == -1
    assert _est(q_len=0, kv_len=0) == -1
    assert _est(kv_len=101) == -1                       # kv_len != q_len
    assert _est(kv_len=99) == -1
    assert _est(hq=6, hkv=4) == -1                      # Hq % Hkv
    assert _est(qs=(8 * 100 * 128, 100 * 128, 132)) == -1
    assert _est(ks=(2 * 100 * 128 + 4, 100 * 128, 128)) == -1
    assert _est(q=P + 8) == -1                          # 16-byte alignment
    assert _est(c=P + 2) == -1                          # 4-byte alignment of the f32 outputs
    assert _est(hd=64, qs=_strides(8, 100, 64), ks=_strides(2, 100, 64)) == -2
    assert _est(hd=256) == -2


def test_sparse_attention_refuses_bad_arguments_before_any_launch():
    for name in ("q", "k", "v", "out", "vi", "si", "ws"):
        assert _attn(**{name: 0}) == -1, name
    assert _attn(bs=0) == -1
    assert _attn(q_len=0, kv_len=0) == -1
    assert _attn(nv=0) == -1 and _attn(ns=0) == -1 and _attn(ns=-3) == -1
    assert _attn(kv_len=120) == -1                      # kv_len != q_len
    assert _attn(hq=6, hkv=4) == -1
    assert _attn(vs=(2 * 100 * 128, 100 * 128 + 2, 128)) == -1
    assert _attn(v=P + 8) == -1 and _attn(out=P + 4) == -1
    assert _attn(vi=P + 2) == -1
    assert _attn(hd=64, qs=_strides(8, 100, 64), ks=_strides(2, 100, 64), vs=_strides(2, 100, 64)) == -2


# ------------------------------------------------------------------------------------------------------ pattern handling
def _cfg(layers=2, heads=8):
    from shadowkv_amd import llama
    return llama.ModelConfig(name="tiny", hidden_size=128 * heads, intermediate_size=2048, num_hidden_layers=layers,
                             num_attention_heads=heads, num_key_value_heads=2, vocab_size=2000)


def _model(pattern, minference=True, layers=2):
    from shadowkv_amd import llama
    return llama.DecoderLM(cfg=_cfg(layers), device="cpu", max_length=256, attn_mode="full", max_new_tokens=16,
                           minference=minference, minference_pattern=pattern)


LAYERS = [{"0": ["stream_llm", 100, 800, 0.5], "3": ["vertical_and_slash", 500, 2000, 0.9]},
          {"7": ["vertical_and_slash", 64, 128, 0.1]}]


def test_json_file_and_list_give_the_same_pattern(tmp_path):
    path = tmp_path / "pattern.json"
    path.write_text(json.dumps(LAYERS))
    a = _model(str(path)).minference_parttern
    b = _model(LAYERS).minference_parttern
    c = _model([{int(h): tuple(e) for h, e in layer.items()} for layer in LAYERS]).minference_parttern
    assert a == b == c
    assert a[0][0] == ("stream_llm", 100, 800, 0.5) and a[0][3] == ("vertical_and_slash", 500, 2000, 0.9)
    assert a[1][7] == ("vertical_and_slash", 64, 128, 0.1)


def test_missing_heads_get_the_default():
    from shadowkv_amd.llama import MINFERENCE_DEFAULT
    assert MINFERENCE_DEFAULT == ("vertical_and_slash", 1000, 6096, 1)
    p = _model(LAYERS).minference_parttern
    assert len(p) == 2 and all(sorted(layer) == list(range(8)) for layer in p)
    assert p[0][1] == MINFERENCE_DEFAULT and p[1][0] == MINFERENCE_DEFAULT
    none = _model(None).minference_parttern
    assert none == [{h: MINFERENCE_DEFAULT for h in range(8)}] * 2
    off = _model(None, minference=False)
    assert off.minference is False and off.minference_parttern is None


@pytest.mark.parametrize("bad, what", [
    ([{"0": ["no_such_type", 10, 10, 1]}, {}], "unknown pattern type"),
    ([{"2": ["block_sparse", 100, 100, 1]}, {}], "block_sparse"),
    ([{}, {"8": ["stream_llm", 10, 10, 1]}], "outside"),
    ([{"-1": ["stream_llm", 10, 10, 1]}, {}], "outside"),
    ([{"x": ["stream_llm", 10, 10, 1]}, {}], "not an integer"),
    ([{}], "layers"),
    ([{}, {}, {}], "layers"),
    ([{"0": ["stream_llm", 0, 10, 1]}, {}], "positive integer"),
    ([{"0": ["vertical_and_slash", 10, 2.5, 1]}, {}], "positive integer"),
    ([{"0": ["stream_llm", 10, 10]}, {}], "expected"),
    ({"0": {}}, "list"),
])
def test_bad_patterns_raise_at_construction(bad, what):
    with pytest.raises(ValueError, match=what):
        _model(bad)


def test_block_sparse_message_names_layer_and_head():
    with pytest.raises(ValueError, match=r"layer 1, head 5: 'block_sparse'"):
        _model([{}, {5: ("block_sparse", 100, 100, 1)}])


# ------------------------------------------------------------------------------------------------------ window mask
def _case(L, nv, ns, seed, dup=False):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-3, L + 40, (nv,), generator=g)          # some entries outside [0, L): ignored
    s = torch.randint(-3, L + 70, (ns,), generator=g)           # offsets >= e_b of a block contribute nothing there
    if dup:
        v = torch.cat([v, v[: nv // 2]])
        s = torch.cat([s, s[: ns // 2], s[:3]])
    return v[torch.randperm(v.numel(), generator=g)], s[torch.randperm(s.numel(), generator=g)]


@pytest.mark.parametrize("L", [1, 2, 5, 63, 64, 65, 127, 130, 200, 257])
@pytest.mark.parametrize("dup", [False, True])
def test_window_mask_matches_brute_force(L, dup):
    for seed in range(3):
        v, s = _case(L, max(1, L // 10), max(1, L // 8), 100 * L + seed, dup)
        assert torch.equal(window_mask(L, v, s), brute_mask(L, v, s)), (L, seed)


def test_window_mask_special_sets():
    L = 200
    full = window_mask(L, [], torch.arange(L))
    assert torch.equal(full, torch.ones(L, L, dtype=torch.bool).tril())    # every offset: dense causal
    diag = window_mask(L, [], [0])
    for i in range(L):                                                     # offset 0: the row's own 64-key block
        b0 = 64 * (i // 64)
        assert diag[i].nonzero().flatten().tolist() == list(range(b0, i + 1))
    # offsets >= e_b contribute nothing to block b; an offset in (e_b - 64, e_b) gives the window [0, 64)
    cov = block_coverage(L, [100])
    assert not cov[0].any() and cov[1].nonzero().flatten().tolist() == list(range(64))
    assert cov[2].nonzero().flatten().tolist() == list(range(28, 92))
    assert cov[3].nonzero().flatten().tolist() == list(range(92, 156))
    sinks = window_mask(L, [0, 0, 3], [])
    assert sinks[:, 0].all() and sinks[3:, 3].all() and int(sinks.sum()) == L + (L - 3)
    assert torch.equal(window_mask(L, [5, 7], [1, 2], rows=[70, 199]), brute_mask(L, [5, 7], [1, 2])[[70, 199]])
