#!/usr/bin/env python3
"""The fetch launch and tokens/s of batched decode with the V offload table in bf16 and in FP8 (e4m3), in
one process on one box: Llama-3.1-8B shapes, 122 K synthetic context, budget 2048, in-place layout, V in pinned host memory,
eager decode_step on a synthetic query walk.  Two models with the same weights and the same context are built per batch size,
one per v_dtype, and timed in turns (bf16, fp8, bf16, fp8, ...).  Reported per batch size and v_dtype:
  * tokens/s (sequences x steps / s, per-step host sync as the benchmark), one figure per turn;
  * the fetch launch (K rebuild || V landing) through cache.fetch_events: mean and median per launch, and summed per step;
  * the last step's logits of the FP8-V model against the bf16-V model over the same tokens and queries: max |d| / max |logit|.
usage: tools/time_v_fetch.py [--batch 8,24] [--steps K] [--warmup W] [--turns T] [--layers L] [--out FILE]   (FILE is appended to)
A batch whose two tables do not fit the host's available memory is replaced by the largest one that does; the line says so."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from shadowkv_amd import llama  # noqa: E402

CTX, DEV = 122 * 1024, "cuda:0"


def mem_available():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return 0


def table_bytes(cfg, layers, batch, elem):
    return layers * batch * cfg.num_key_value_heads * (CTX // 8) * 1024 * elem


def reset(model):
    c = model.kv_cache
    c.kv_offset, c.gen_offset = CTX, 0                  # back to the state right after the prefill


def decode(model, steps, warmup, seed, tokens_in=None, keep=None):
    """steps of decode_step on the query walk of `seed`; returns (tokens/s over the last `steps`, the tokens fed)"""
    c = model.kv_cache
    reset(model)
    slack = c.k_cache_buffer.shape[-2] - c.sparse_end
    walk = llama.QueryWalk(model, step=0.3, seed=seed)
    tok = torch.randint(0, model.vocab_size, (model.batch_size, 1), device=model.device,
                        generator=torch.Generator(device=model.device).manual_seed(1))
    fed, t0 = [], None
    for i in range(warmup + steps):
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if c.gen_offset >= slack:
            reset(model)
        if tokens_in is not None:
            tok = tokens_in[i]
        fed.append(tok)
        walk.advance()
        tok = model.decode_step(tok, temperature=0.0 if keep is not None else 0.6, q_table=walk.qb)
        tok[:, -1].tolist()                             # per-step host sync, as the benchmark
    torch.cuda.synchronize()
    return steps * model.batch_size / (time.perf_counter() - t0), fed


def fetch_times(model, steps, seed):
    """ms of every fetch launch of `steps` steps (after 2 unrecorded ones)"""
    decode(model, 2, 0, seed)
    model.kv_cache.fetch_events = []
    decode(model, steps, 0, seed + 1)
    torch.cuda.synchronize()
    ev, model.kv_cache.fetch_events = model.kv_cache.fetch_events, None
    return [a.elapsed_time(b) for a, b, _ in ev]


def tap(model):
    box, orig = {}, model.forward_fused

    def ff(*args, **kw):
        box["logits"] = orig(*args, **kw)
        return box["logits"]
    model.forward_fused = ff
    return box


def one_batch(a, batch):
    cfg = llama.LLAMA_3_1_8B
    layers = a.layers or cfg.num_hidden_layers
    note, avail = "", mem_available()
    while batch > 1 and table_bytes(cfg, layers, batch, 3) > 0.85 * avail:     # bf16 (2 B) + fp8 (1 B) tables side by side
        batch -= 1
    if batch != a.want:
        note = (f" (bs {a.want} asked: its two tables need {table_bytes(cfg, layers, a.want, 3) / 1e9:.1f} GB of pinned host memory, "
                f"{avail / 1e9:.1f} GB are available; bs {batch} is the largest batch that fits both)")
    models = {}
    for v_dtype in ("bf16", "fp8_e4m3"):
        m = llama.DecoderLM(cfg=cfg, batch_size=batch, max_length=CTX, device=DEV, sparse_budget=2048, rank=160, chunk_size=8,
                            num_layers=a.layers, chunk_layout="inplace", overlap_attention=True, v_dtype=v_dtype,
                            max_new_tokens=max(1024, 8 * (a.warmup + a.steps) + 256))
        llama.build_synthetic_context(m, CTX, seed=4321)
        models[v_dtype] = m
    tps = {k: [] for k in models}
    for t in range(a.turns):
        for k, m in models.items():
            tps[k].append(decode(m, a.steps, a.warmup, 4242 + t)[0])
    fetch = {k: fetch_times(m, a.fetch_steps, 777) for k, m in models.items()}
    boxes = {k: tap(m) for k, m in models.items()}
    _, fed = decode(models["bf16"], a.logit_steps, 0, 99, keep=True)
    decode(models["fp8_e4m3"], a.logit_steps, 0, 99, tokens_in=fed, keep=True)
    la, lb = boxes["fp8_e4m3"]["logits"].float(), boxes["bf16"]["logits"].float()
    dev = float((la - lb).abs().max() / lb.abs().max())
    L = models["bf16"].num_layers
    lines = [f"# tools/time_v_fetch.py on {torch.cuda.get_device_name(0)}: Llama-3.1-8B shapes, 122 K synthetic context, budget 2048, "
             f"in-place layout, V in pinned host memory, eager decode_step, bs {batch}{note}, {L} layers, {a.turns} turns of {a.steps} "
             f"steps after {a.warmup} warm-up steps per v_dtype, taken in turns"]
    for k, m in models.items():
        f = fetch[k]
        c = m.kv_cache
        lines.append(f"bs {batch:2d} v_dtype {k:<9} tokens/s {' '.join(f'{x:8.2f}' for x in tps[k])}  (median {statistics.median(tps[k]):8.2f})  "
                     f"fetch launch: mean {statistics.mean(f):7.3f} ms  median {statistics.median(f):7.3f} ms  per step ({L} layers) "
                     f"{statistics.mean(f) * L:8.3f} ms  over {len(f)} launches  table {c.v_cache_cpu.numel() * c.v_cache_cpu.element_size() / 1e9:6.2f} GB pinned"
                     + (f"  v_scale {c.v_scale.numel() * 4 / 1e9:5.2f} GB HBM" if c.v_scale is not None else ""))
    lines.append(f"bs {batch:2d} fp8 : bf16  tokens/s (medians) {statistics.median(tps['fp8_e4m3']) / statistics.median(tps['bf16']):.3f}   "
                 f"fetch launch (means) {statistics.mean(fetch['fp8_e4m3']) / statistics.mean(fetch['bf16']):.3f}")
    lines.append(f"bs {batch:2d} logits of step {a.logit_steps} (same tokens, same queries), FP8-V model against bf16-V model: "
                 f"max |d| / max |logit| = {dev:.3e}")
    del models, boxes
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="8,24")
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--turns", type=int, default=2)
    ap.add_argument("--fetch-steps", type=int, default=6, dest="fetch_steps")
    ap.add_argument("--logit-steps", type=int, default=6, dest="logit_steps")
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for b in [int(x) for x in a.batch.split(",")]:
        a.want = b
        lines = one_batch(a, b)
        print("\n".join(lines), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        import gc
        gc.collect()


if __name__ == "__main__":
    main()
