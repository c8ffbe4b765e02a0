#!/usr/bin/env python3
"""tokens/s of the headline configuration (Llama-3.1-8B shapes, 122 K synthetic context, budget 2048, hipGraph, in-place
layout with overlap_attention, bs 1) with bf16 weights and with weight-only FP8 weights, on one box in one process: the bf16
model is built and timed, then quantised in place (DecoderLM.quantize_weights) and timed again over the SAME context and
query walk.  usage: tools/fp8_e2e.py [--steps K] [--warmup W] [--layers L] [--batch B] [--weight-dtype D] [--out FILE]
(FILE is appended to).  --weight-dtype {fp8_e4m3,mxfp4} (bs 1): the format the second measurement quantises to (default
fp8_e4m3); given explicitly it also appends the relative deviation of one probe step's logits from the bf16 model's (same
token, same synthetic queries, same context - a random-weight figure, not an accuracy measurement).
--batch B (B > 1): the batched headline configuration (in-place layout, V in pinned host memory, eager decode_step - a captured
graph at bs > 1 is not part of the FP8 rows work) as a triple over one context, measured one after the other: the bf16 model, the
FP8 model with the dequantising fallback, the FP8 model with fp8_rows="native" (skv_linear_rows_fp8).
--weight-dtype mxfp4 --batch B: the same triple for MXFP4 weights - bf16, the MXFP4 model with the dequantising fallback, the
MXFP4 model with mxfp4_rows="native" (skv_linear_rows_mxfp4); --mxfp4-rows {both,fallback,native} picks
which of the two MXFP4 measurements run (the fallback dequantises every matrix on every step: it is the slow one).
--landmark-dtype fp8_e4m3 (any --batch): bf16 weights throughout, ONE model and context; the cache's landmark
table is swapped between the bf16 means and their FP8 quantisation (table + row scales) and the two are timed alternately,
--repeats times each (bs 1: captured graph with early fetch + near staging; bs > 1: eager decode_step), then a short probe run
per dtype over the same query walk reports how many of the selected chunks the two share per step."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from shadowkv_amd import llama  # noqa: E402


def run(model, ctx, steps, warmup, seed=4242):
    c = model.kv_cache
    c.kv_offset, c.gen_offset = ctx, 0                  # back to the state right after the prefill
    table = llama.make_walk_table(model, warmup + steps + 6, step=0.3, seed=seed)
    dec = llama.GraphDecoder(model, temperature=0.6, walk_table=table, ring_slack=True)
    dec.token.copy_(torch.randint(0, model.vocab_size, (1, 1), device=model.device, generator=torch.Generator(device=model.device).manual_seed(1)))
    dec.capture()
    for _ in range(warmup):
        dec.step()[:, -1].tolist()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        dec.step()[:, -1].tolist()                      # per-step host sync, as the benchmark
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def probe_logits(model, ctx, seed=77):
    """The logits of ONE fused decode step right after the prefill state: a fixed token, a fixed synthetic query table."""
    c = model.kv_cache
    c.kv_offset, c.gen_offset = ctx, 0
    table = llama.make_walk_table(model, 1, step=0.3, seed=seed)
    tok = torch.tensor([[17]], device=model.device)
    row = c.sparse_end + c.gen_offset
    lg = model.forward_fused(tok, model.get_ctx(tok), torch.tensor([row], device=model.device), kv_len=row + 1, q_table=table[0])
    torch.cuda.synchronize()
    return lg[:, -1].float().clone()


def run_eager(model, ctx, steps, warmup, seed=4242):
    """sequences x steps / s of decode_step on a synthetic query walk (bench.py's --mode eager loop)"""
    c = model.kv_cache
    c.kv_offset, c.gen_offset = ctx, 0
    slack = c.k_cache_buffer.shape[-2] - c.sparse_end
    walk = llama.QueryWalk(model, step=0.3, seed=seed)
    tok = torch.randint(0, model.vocab_size, (model.batch_size, 1), device=model.device,
                        generator=torch.Generator(device=model.device).manual_seed(1))
    t0 = None
    for i in range(warmup + steps):
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if c.gen_offset >= slack:                       # generated-row slack exhausted: rewind the bookkeeping (as bench.py)
            c.kv_offset, c.gen_offset = ctx, 0
        walk.advance()
        tok = model.decode_step(tok, temperature=0.6, q_table=walk.qb)
        tok[:, -1].tolist()                             # per-step host sync, as the benchmark
    torch.cuda.synchronize()
    return steps * model.batch_size / (time.perf_counter() - t0)


def batched(a, wd="fp8_e4m3"):
    from shadowkv_amd import tensor_op
    mx = wd == "mxfp4"
    tag, attr = ("mxfp4", "mxfp4_rows") if mx else ("fp8", "fp8_rows")
    modes = ("fallback", "native") if not mx or a.mxfp4_rows == "both" else (a.mxfp4_rows,)
    calls = lambda: (getattr(tensor_op, tag + "_native_calls"), getattr(tensor_op, tag + "_fallback_calls"))
    ctx, dev = 122 * 1024, "cuda:0"
    model = llama.DecoderLM(cfg=llama.LLAMA_3_1_8B, batch_size=a.batch, max_length=ctx, device=dev, sparse_budget=2048, rank=160,
                            chunk_size=8, num_layers=a.layers, chunk_layout="inplace", overlap_attention=True,
                            max_new_tokens=max(1024, 8 * (a.warmup + a.steps) + 256))
    llama.build_synthetic_context(model, ctx, seed=4321)
    res = {"bf16": (run_eager(model, ctx, a.steps, a.warmup), model.weight_bytes(), 0, 0)}
    model.quantize_weights(dtype=wd)
    torch.cuda.empty_cache()
    for mode in modes:
        setattr(model, attr, mode)
        n0, f0 = calls()
        tps = run_eager(model, ctx, a.steps, a.warmup)
        res[f"{tag} {mode}"] = (tps, model.weight_bytes(), calls()[0] - n0, calls()[1] - f0)
    lines = [f"# tools/fp8_e2e.py --batch {a.batch} on {torch.cuda.get_device_name(0)}: 122 K synthetic context, budget 2048, in-place + "
             f"overlap_attention, V in pinned host memory, eager decode_step, {model.num_layers} layers, {a.steps} steps after {a.warmup} warm-up steps"]
    for k, (tps, nbytes, nat, fb) in res.items():
        lines.append(f"bs {a.batch:2d} {k:<14} {tps:8.2f} tokens/s  weights {nbytes / 1e9:6.2f} GB  native {'MXFP4' if mx else 'FP8'} launches {nat}  "
                     f"dequantising fallbacks {fb}")
    ratios = [f"{tag} {m} : bf16 {res[f'{tag} {m}'][0] / res['bf16'][0]:.3f}" for m in modes]
    if len(modes) == 2:
        ratios.append(f"{tag} native : {tag} fallback {res[f'{tag} native'][0] / res[f'{tag} fallback'][0]:.3f}")
    lines.append(f"bs {a.batch:2d} tokens/s ratios: " + "   ".join(ratios))
    return lines


def selected_sets(model, ctx, steps, seed=99):
    """bool [steps, L, bs, kv, n_chunks]: the chunks in the resident set after each eager step of a fixed query walk (with
    resident_sets == select_sets that IS the step's selection; it depends on the walk and the landmarks only)"""
    c = model.kv_cache
    c.kv_offset, c.gen_offset = ctx, 0
    walk = llama.QueryWalk(model, step=0.3, seed=seed)
    tok = torch.full((model.batch_size, 1), 17, device=model.device)
    out = []
    for _ in range(steps):
        walk.advance()
        tok = model.decode_step(tok, temperature=0.0, q_table=walk.qb)
        ids = c.position_ids.clamp_min(0)
        out.append(torch.zeros(*ids.shape[:-1], c.v_cache_cpu.shape[-2], dtype=torch.bool, device=ids.device).scatter_(-1, ids, True))
    torch.cuda.synchronize()
    return torch.stack(out)


def landmark_ab(a):
    from shadowkv_amd import tensor_op
    ctx, dev, bs = 122 * 1024, "cuda:0", a.batch
    model = llama.DecoderLM(cfg=llama.LLAMA_3_1_8B, batch_size=bs, max_length=ctx, device=dev, sparse_budget=2048, rank=160,
                            chunk_size=8, num_layers=a.layers, chunk_layout="inplace", overlap_attention=True,
                            max_new_tokens=max(1024, 8 * (a.warmup + a.steps) + 256))
    llama.build_synthetic_context(model, ctx, seed=4321)
    c = model.kv_cache
    if bs == 1:
        c.enable_early_fetch(near=True)
    lm = c.k_landmark
    table = torch.zeros(lm.shape, dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)
    scale = torch.ones(lm.shape[:-1], dtype=torch.float32, device=dev)
    for l in range(lm.shape[0]):
        tensor_op.quantize_v_rows(lm[l], table[l].view(bs, lm.shape[2], -1), scale[l])
    torch.cuda.synchronize()
    forms = {"bf16": (lm, None), a.landmark_dtype: (table, scale)}

    def use(dt):
        c.k_landmark, c.k_landmark_scale = forms[dt]
        c.landmark_dtype = dt

    tps = {dt: [] for dt in forms}
    for _ in range(a.repeats):
        for dt in forms:
            use(dt)
            tps[dt].append(run(model, ctx, a.steps, a.warmup) if bs == 1 else run_eager(model, ctx, a.steps, a.warmup))
    sets = {}
    for dt in forms:
        use(dt)
        sets[dt] = selected_sets(model, ctx, 8)
    S = c.select_sets
    both = (sets["bf16"] & sets[a.landmark_dtype]).sum(-1).float() / S                 # [steps, L, bs, kv]
    lines = [f"# tools/fp8_e2e.py --landmark-dtype {a.landmark_dtype} --batch {bs} on {torch.cuda.get_device_name(0)}: 122 K synthetic context, "
             f"budget 2048, in-place + overlap_attention, {'hipGraph, early fetch + near staging' if bs == 1 else 'eager decode_step'}, "
             f"{model.num_layers} layers, {a.steps} steps after {a.warmup} warm-up steps, {a.repeats} alternating repeats"]
    for dt, v in tps.items():
        v = sorted(v)
        lines.append(f"bs {bs:2d} landmark_dtype {dt:<9} {v[len(v) // 2]:8.2f} tokens/s (median; all: {' '.join(f'{x:.2f}' for x in v)})  "
                     f"landmark table {forms[dt][0][0].numel() * forms[dt][0].element_size() / 1e6:7.1f} MB per layer")
    med = {dt: sorted(v)[len(v) // 2] for dt, v in tps.items()}
    lines.append(f"bs {bs:2d} fp8 : bf16 landmarks tokens/s ratio {med[a.landmark_dtype] / med['bf16']:.3f}")
    lines.append(f"bs {bs:2d} selected chunks shared by the two, per step (mean over layers and heads): "
                 + " ".join(f"{100 * float(x):.1f}%" for x in both.mean(dim=(1, 2, 3))) + f"   min over (step, layer, head) {100 * float(both.min()):.1f}%")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--weight-dtype", dest="weight_dtype", choices=("fp8_e4m3", "mxfp4"), default=None)
    ap.add_argument("--mxfp4-rows", dest="mxfp4_rows", choices=("both", "fallback", "native"), default="both")
    ap.add_argument("--landmark-dtype", dest="landmark_dtype", choices=("fp8_e4m3",), default=None)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.landmark_dtype:
        lines = landmark_ab(a)
        print("\n".join(lines))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    wd = a.weight_dtype or "fp8_e4m3"
    if a.batch > 1:
        lines = batched(a, wd)
        print("\n".join(lines))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    ctx, dev = 122 * 1024, "cuda:0"
    model = llama.DecoderLM(cfg=llama.LLAMA_3_1_8B, batch_size=1, max_length=ctx, device=dev, sparse_budget=2048, rank=160,
                            chunk_size=8, num_layers=a.layers, chunk_layout="inplace", overlap_attention=True,
                            max_new_tokens=max(1024, 8 * (a.warmup + a.steps) + 256))
    llama.build_synthetic_context(model, ctx, seed=4321)
    model.kv_cache.enable_early_fetch(near=True)        # the headline's default for G <= 4
    res = {}
    res["bf16"] = (run(model, ctx, a.steps, a.warmup), model.weight_bytes(), model.kv_proj_split_launches > 0)
    ref = probe_logits(model, ctx) if a.weight_dtype else None
    model.quantize_weights(dtype=wd)
    torch.cuda.empty_cache()
    res[wd] = (run(model, ctx, a.steps, a.warmup), model.weight_bytes(), False)
    lines = [f"# tools/fp8_e2e.py on {torch.cuda.get_device_name(0)}: 122 K synthetic context, budget 2048, hipGraph, in-place + "
             f"overlap_attention, bs 1, {model.num_layers} layers, {a.steps} steps after {a.warmup} warm-up steps"]
    for k, (tps, nbytes, split) in res.items():
        lines.append(f"weight_dtype {k:<9} {tps:8.2f} tokens/s  {1e6 / tps / model.num_layers:7.2f} us/layer  weights {nbytes / 1e9:6.2f} GB"
                     f"  qkv {'split (q launch + k/v role)' if split else 'one launch'}")
    lines.append(f"{'fp8' if wd == 'fp8_e4m3' else wd} : bf16 tokens/s ratio {res[wd][0] / res['bf16'][0]:.3f}")
    if ref is not None:
        got = probe_logits(model, ctx)
        lines.append(f"probe step (token 17, fixed synthetic queries): |logits_{wd} - logits_bf16| / |logits_bf16| = "
                     f"{float((got - ref).norm() / ref.norm()):.3e}  (random weights: not an accuracy measurement)")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
