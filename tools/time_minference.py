"""Times the MInference vertical + slash sparse prefill at Llama-3.1-8B head shapes (32 query / 8 KV
heads, D = 128), bs 1, Gaussian bf16, every shape warmed first, interleaved rounds in one process, medians of HIP events.

(a) the index estimate (tensor_op.vertical_slash_scores) and estimate + top-k + sorted index lists
    (tensor_op.vertical_slash_indices, MInference's default sizes 1,000 / 6,096) per layer;
(b) tensor_op.sparse_prefill_attention against the dense causal kernel (skv_prefill_attention) on the same data, for three
    STATED index sets (random Gaussian q / k give diffuse attention, so an estimated set would keep almost every key):
      full       slash = every offset (dense causal coverage);
      structured slash = offsets 0 .. 4095 + 2,000 distinct random offsets, vertical = the 30 sinks + 970 random columns;
      stream     stream_llm 128 / 4096 (vertical 0 .. 127, slash 0 .. 4095);
    every head gets the same lists; attended (query, key) pairs are counted from the lists (the section 9 mask) and the time
    per attended pair is reported next to the dense kernel's on the causal pairs;
(c) DecoderLM.batch_prefill of one --e2e-len prompt on the 32-layer shapes (random weights, ShadowKV cache): dense, the
    default vertical_and_slash pattern (the density it chose is counted for heads 0 and 31 of layers 0 and 31), and
    stream_llm 128 / 4096 on every head.

    python tools/time_minference.py [--lengths 32768 124928] [--rounds 5] [--no-e2e] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shadowkv_amd import llama, tensor_op  # noqa: E402

DEV = "cuda:0"
HQ, HKV, D = 32, 8, 128


def time_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def attended_pairs(L, vertical, slash, chunk=64):
    """(query, key) pairs the section 9 mask keeps for one head: vertical / slash 1-D integer lists (entries outside [0, L)
    ignored).  Windows per 64-row block through a difference array, chunk blocks at a time, on the GPU."""
    n_blk = (L + 63) // 64
    s = torch.unique(slash[(slash >= 0) & (slash < L)].to(DEV, torch.int64))
    vert = torch.zeros(L, dtype=torch.int32, device=DEV)
    v = vertical[(vertical >= 0) & (vertical < L)].to(DEV, torch.int64)
    vert[v] = 1
    total = 0
    for b0 in range(0, n_blk, chunk):
        blocks = torch.arange(b0, min(n_blk, b0 + chunk), device=DEV)
        e = 64 * (blocks + 1)
        diff = torch.zeros(blocks.numel(), L + 65, dtype=torch.int32, device=DEV)
        hi = torch.clamp(e.view(-1, 1) - s.view(1, -1), min=64)
        on = (s.view(1, -1) < e.view(-1, 1)).int()
        diff.scatter_add_(1, hi - 64, on)
        diff.scatter_add_(1, hi, -on)
        keep = ((diff.cumsum(1)[:, :L] > 0).int() | vert.view(1, -1)).cumsum(1)          # keys kept at or below j
        rows = (64 * blocks.view(-1, 1) + torch.arange(64, device=DEV).view(1, -1)).clamp(max=L - 1)
        valid = (64 * blocks.view(-1, 1) + torch.arange(64, device=DEV).view(1, -1)) < L
        total += int((keep.gather(1, rows) * valid).sum())
        del diff, keep
    return total


def index_sets(L, seed):
    g = torch.Generator().manual_seed(seed)
    full_s = torch.arange(L)
    full_v = torch.zeros(1, dtype=torch.int64)
    st_s = torch.cat([torch.arange(4096), 4096 + torch.randperm(L - 4096, generator=g)[:2000]])
    st_v = torch.cat([torch.arange(30), 30 + torch.randperm(L - 30, generator=g)[:970]])
    return {"full": (full_v, full_s), "structured": (st_v, st_s),
            "stream_128_4096": (torch.arange(128), torch.arange(4096))}


def kernel_rows(lengths, rounds):
    rows = []
    for L in lengths:
        g = torch.Generator(device=DEV).manual_seed(L)
        q = torch.randn(1, HQ, L, D, device=DEV, generator=g).bfloat16()
        k = torch.randn(1, HKV, L, D, device=DEV, generator=g).bfloat16()
        v = torch.randn(1, HKV, L, D, device=DEV, generator=g).bfloat16()
        out = torch.empty(1, L, HQ, D, device=DEV, dtype=torch.bfloat16)
        sets = index_sets(L, L)
        lists = {}
        for name, (vi, si) in sets.items():
            vi = torch.sort(vi.to(torch.int32)).values.to(DEV).view(1, 1, -1).expand(1, HQ, -1).contiguous()
            si = torch.sort(si.to(torch.int32)).values.to(DEV).view(1, 1, -1).expand(1, HQ, -1).contiguous()
            lists[name] = (vi, si)
        legs = {"dense": lambda: tensor_op.causal_attention_prefill(q, k, v, out=out),
                "estimate": lambda: tensor_op.vertical_slash_scores(q, k),
                "estimate_topk_indices": lambda: tensor_op.vertical_slash_indices(q, k, 1000, 6096)}
        for name, (vi, si) in lists.items():
            legs["sparse_" + name] = (lambda vi=vi, si=si: tensor_op.sparse_prefill_attention(q, k, v, vi, si, out=out,
                                                                                                sorted=True))
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        ms = {n: [] for n in legs}
        for _ in range(rounds):
            for n, fn in legs.items():
                ms[n].append(time_call(fn))
        causal = L * (L + 1) // 2
        row = {"L": L, "heads": [HQ, HKV], "causal_pairs_per_head": causal}
        for n, xs in ms.items():
            row[n] = {"ms_median": round(statistics.median(xs), 4), "ms_min": round(min(xs), 4), "rounds": len(xs)}
        dense_ms = row["dense"]["ms_median"]
        row["dense"]["ps_per_pair"] = round(dense_ms * 1e9 / (HQ * causal), 3)
        row["dense"]["tflops_median"] = round(4 * D * HQ * causal / dense_ms / 1e9, 1)
        for name, (vi, si) in sets.items():
            pairs = attended_pairs(L, vi, si)
            leg = row["sparse_" + name]
            leg["pairs_per_head"] = pairs
            leg["density"] = round(pairs / causal, 4)
            leg["ps_per_pair"] = round(leg["ms_median"] * 1e9 / (HQ * pairs), 3)
            leg["tflops_on_pairs"] = round(4 * D * HQ * pairs / leg["ms_median"] / 1e9, 1)
            leg["rate_vs_dense"] = round(leg["tflops_on_pairs"] / row["dense"]["tflops_median"], 3)
            leg["time_vs_dense"] = round(leg["ms_median"] / dense_ms, 3)
        row["estimate_share_of_structured"] = round(row["estimate_topk_indices"]["ms_median"] /
                                                    row["sparse_structured"]["ms_median"], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del q, k, v, out, legs, lists
        torch.cuda.empty_cache()
    return rows


def e2e_rows(n):
    m = llama.DecoderLM(cfg=llama.LLAMA_3_1_8B, batch_size=1, max_length=n, device=DEV, seed=1)
    ids = torch.randint(0, m.vocab_size, (1, n), generator=torch.Generator().manual_seed(0)).to(DEV)
    stream = [{h: ("stream_llm", 128, 4096, 1) for h in range(HQ)} for _ in range(m.num_layers)]
    legs = {"dense": (False, None), "vertical_and_slash_default": (True, llama.load_minference_pattern(None, m.num_layers, HQ)),
            "stream_llm_128_4096": (True, llama.load_minference_pattern(stream, m.num_layers, HQ))}
    res = {"prompt": n, "layers": m.num_layers, "model": "llama-3.1-8b shapes, random weights, ShadowKV cache"}
    captured = {}
    orig = tensor_op.minference_index_sets

    def spy(q, k, pat):
        vi, si = orig(q, k, pat)
        captured.setdefault("layers", []).append((vi[0, [0, HQ - 1]].cpu(), si[0, [0, HQ - 1]].cpu()))
        return vi, si

    ms = {name: [] for name in legs}
    try:
        tensor_op.minference_index_sets = spy
        for rnd in range(2):                               # a warm round, then a timed one
            for name, (on, pat) in legs.items():
                m.minference, m.minference_parttern = on, pat
                captured.clear()
                t = time_call(lambda: m.batch_prefill(ids))
                if rnd:
                    ms[name].append(t)
                if rnd and name == "vertical_and_slash_default":
                    lay = captured["layers"]
                    dens = []
                    for vi, si in (lay[0], lay[-1]):
                        for h in range(2):
                            dens.append(attended_pairs(n, vi[h], si[h]) / (n * (n + 1) // 2))
                    res["default_pattern_density_l0_l31_h0_h31"] = [round(x, 4) for x in dens]
    finally:
        tensor_op.minference_index_sets = orig
        m.minference, m.minference_parttern = False, None
    res["batch_prefill_ms"] = {name: round(xs[0], 1) for name, xs in ms.items()}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", type=int, nargs="*", default=[32768, 124928])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--e2e-len", type=int, default=124928)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "kernel": kernel_rows(a.lengths, a.rounds)}
    if not a.no_e2e:
        res["e2e"] = e2e_rows(a.e2e_len)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
