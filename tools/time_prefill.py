"""Times the prefill: the causal attention kernel alone against SDPA, and DecoderLM.batch_prefill end to end, split into parts.

Kernel: tensor_op.causal_attention_prefill at Llama-3.1-8B head shapes (32 query / 8 KV heads, D = 128), bs 1, Gaussian bf16
data, causal FLOPs 4 bs Hq D sum_i (kv_len - q_len + i + 1).  Interleaved rounds in one process against
F.scaled_dot_product_attention(is_causal=True) on the same data with K / V expanded to 32 heads, restricted to the fused
backends (the math backend would materialise S x S scores); HIP events, every shape warmed first.

End to end: the 32-layer Llama-3.1-8B shapes (random weights) on the ShadowKV cache, one prompt of --e2e-len tokens through
batch_prefill; attention, get_svd and prefill_kv_cache are bracketed by events, the rest (dense GEMMs, norms, RoPE, embedding,
lm_head) is the remainder.

    python tools/time_prefill.py [--lengths 4096 32768 124928] [--rounds 5] [--no-sdpa] [--no-e2e] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shadowkv_amd import llama, tensor_op  # noqa: E402

DEV = "cuda:0"


def causal_flops(bs, hq, d, q_len, kv_len):
    off = kv_len - q_len
    return 4 * bs * hq * d * (q_len * (off + 1) + q_len * (q_len - 1) // 2)


def sdpa_fn():
    try:
        from torch.nn.attention import SDPBackend, sdpa_kernel
    except ImportError:
        return None
    backends = [SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION]

    def run(q, k, v):
        with sdpa_kernel(backends):
            return F.scaled_dot_product_attention(q, k, v, is_causal=True)
    return run


def time_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_rows(lengths, rounds, use_sdpa):
    rows = []
    sdpa = sdpa_fn() if use_sdpa else None
    for S in lengths:
        g = torch.Generator(device=DEV).manual_seed(S)
        q = torch.randn(1, 32, S, 128, device=DEV, generator=g).bfloat16()
        k = torch.randn(1, 8, S, 128, device=DEV, generator=g).bfloat16()
        v = torch.randn(1, 8, S, 128, device=DEV, generator=g).bfloat16()
        out = torch.empty(1, S, 32, 128, device=DEV, dtype=torch.bfloat16)
        ours = lambda: tensor_op.causal_attention_prefill(q, k, v, out=out)  # noqa: E731
        legs = {"skv_prefill_attention": ours}
        note = None
        if sdpa is not None:
            ke, ve = k.repeat_interleave(4, dim=1), v.repeat_interleave(4, dim=1)
            try:
                sdpa(q, ke, ve)
                legs["sdpa"] = lambda: sdpa(q, ke, ve)
            except RuntimeError as e:          # no fused backend for this shape / build
                note = f"sdpa unavailable: {str(e).splitlines()[0][:160]}"
        for fn in legs.values():               # warm every leg at this shape
            fn()
        torch.cuda.synchronize()
        ms = {n: [] for n in legs}
        for _ in range(rounds):                # interleaved rounds
            for n, fn in legs.items():
                ms[n].append(time_call(fn))
        fl = causal_flops(1, 32, 128, S, S)
        row = {"S": S, "causal_flop": fl}
        for n, xs in ms.items():
            med = statistics.median(xs)
            row[n] = {"ms_median": round(med, 4), "ms_min": round(min(xs), 4), "tflops_median": round(fl / med / 1e9, 1),
                      "tflops_best": round(fl / min(xs) / 1e9, 1), "rounds": len(xs)}
        if note:
            row["note"] = note
        print(json.dumps(row), flush=True)
        rows.append(row)
        del q, k, v, out, legs
        torch.cuda.empty_cache()
    return rows


def e2e_row(n):
    m = llama.DecoderLM(cfg=llama.LLAMA_3_1_8B, batch_size=1, max_length=n, device=DEV, seed=1)
    c = m.kv_cache
    spans = {"attention": [], "get_svd": [], "prefill_kv_cache": []}

    def bracket(name, fn):
        def wrapped(*a, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn(*a, **kw)
            e.record()
            spans[name].append((s, e))
            return r
        return wrapped

    orig_attn = tensor_op.causal_attention_prefill
    ids = torch.randint(0, m.vocab_size, (1, n), generator=torch.Generator().manual_seed(0)).to(DEV)
    try:
        tensor_op.causal_attention_prefill = bracket("attention", orig_attn)
        c.get_svd = bracket("get_svd", c.get_svd)
        c.prefill_kv_cache = bracket("prefill_kv_cache", c.prefill_kv_cache)
        res = {}
        for leg in ("warm", "timed"):
            for v in spans.values():
                v.clear()
            total = time_call(lambda: m.batch_prefill(ids))
            torch.cuda.synchronize()
            res = {k: round(sum(s.elapsed_time(e) for s, e in v), 1) for k, v in spans.items()}
            res["total"] = round(total, 1)
        res["dense_and_rest"] = round(res["total"] - res["attention"] - res["get_svd"] - res["prefill_kv_cache"], 1)
    finally:
        tensor_op.causal_attention_prefill = orig_attn
    row = {"e2e_prefill_ms": res, "prompt": n, "layers": m.num_layers, "model": "llama-3.1-8b shapes, random weights",
           "attention_tflops": round(32 * causal_flops(1, 32, 128, n, n) / res["attention"] / 1e9, 1)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", type=int, nargs="*", default=[4096, 32768, 124928])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-sdpa", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--e2e-len", type=int, default=124928)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "kernel": kernel_rows(a.lengths, a.rounds, not a.no_sdpa)}
    if not a.no_e2e:
        res["e2e"] = e2e_row(a.e2e_len)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
