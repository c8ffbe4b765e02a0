#!/usr/bin/env python3
"""Back-to-back timing of the decode step's dense kernels over 32 layers of distinct weights (HBM-cold, like the step)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from shadowkv_amd import tensor_op, llama
dev = "cuda:0"


def _fixture(reps):
    """The five launches of a decode step's dense half (fn(w, w_scale): bf16 with None, FP8 or MXFP4 by the pair), the graph
    builder and the timer that --fp8 and --mxfp4 share: (g, shapes, graph_of, timed)."""
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(0)
    flush = torch.zeros(1 << 30, dtype=torch.uint8, device=dev)
    x = torch.randn(1, 1, 4096, device=dev, generator=g).bfloat16()
    res = torch.randn(1, 1, 4096, device=dev, generator=g).bfloat16()
    xi = torch.randn(1, 1, 14336, device=dev, generator=g).bfloat16()
    nw = torch.ones(4096, device=dev, dtype=torch.bfloat16)
    cs = llama.build_cos_sin_cache(llama.LLAMA_3_1_8B, 4096, torch.device(dev), torch.bfloat16)
    pos = torch.tensor([[100]], device=dev); row = torch.tensor([5], device=dev)
    kc = torch.zeros(1, 8, 64, 128, device=dev, dtype=torch.bfloat16); vc = torch.zeros_like(kc)
    rm = torch.zeros(1, 128256 // 16, dtype=torch.int16, device=dev)

    shapes = [
        ("qkv 6144x4096 (norm+rope+push)", 6144, 4096,
         lambda w, sc: tensor_op.norm_qkv_rope_update(x, res, nw, 1e-5, w, None, cs, pos, row, kc, vc, 32, 8, w_scale=sc)),
        ("o 4096x4096", 4096, 4096, lambda w, sc: tensor_op.linear_decode(x, w, w_scale=sc)),
        ("gate/up 28672x4096 (norm+silu)", 28672, 4096,
         lambda w, sc: tensor_op.norm_linear_decode(x, res, nw, 1e-5, w, fuse_silu_mul=True, w_scale=sc)),
        ("down 4096x14336 (+residual)", 4096, 14336, lambda w, sc: tensor_op.linear_decode(xi, w, bias=res, w_scale=sc)),
        ("lm_head 128256x4096 (norm+keys)", 128256, 4096,
         lambda w, sc: tensor_op.norm_linear_decode(x, res, nw, 1e-5, w, range_max=rm, w_scale=sc)),
    ]

    def graph_of(fn):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            flush.add_(1)
            if fn is not None:
                fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            for _ in range(reps):
                flush.add_(1)
                if fn is not None:
                    fn()
        gr.replay(); torch.cuda.synchronize()
        return gr

    def timed(gr):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); gr.replay(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps           # us per iteration

    return g, shapes, graph_of, timed


def fp8_mode(out_path=None, rounds=7, reps=24):
    """--fp8 [FILE]: every FP8 launch against the bf16 launch of the same shape (skv_gemv.hip, unchanged), HBM-cold.
    Per shape three captured graphs of `reps` iterations: [flush], [flush, FP8 launch], [flush, bf16 launch] - the flush
    rewrites a 1 GiB buffer (four times L2 + the 256 MiB last-level cache), so every launch reads its weights from HBM.  The
    graphs are replayed in interleaved rounds; a launch's time is (its graph - the flush graph) / reps within the round, the
    reported figure the median over the rounds.  bytes: the weights (+ 4 N of scales); the activations are noise next to them."""
    g, shapes, graph_of, timed = _fixture(reps)

    def weights(n, k):
        w = (torch.randn(n, k, device=dev, generator=g) * 0.02).bfloat16()
        return (w,) + tensor_op.quantize_fp8_rows(w)

    lines = [f"# tools/time_gemv.py --fp8 on {torch.cuda.get_device_name(0)}: HBM-cold launches (1 GiB flush before each), "
             f"median of {rounds} interleaved rounds of {reps} launches; us per launch, TB/s over the weight bytes",
             f"{'shape':<34} {'fp8 us':>8} {'TB/s':>6} {'bf16 us':>8} {'TB/s':>6} {'bf16/fp8':>9} {'flush us':>9}"]
    worst = None
    for name, n, k, fn in shapes:
        wb, w8, sc = weights(n, k)
        g0, g8, gb = graph_of(None), graph_of(lambda: fn(w8, sc)), graph_of(lambda: fn(wb, None))
        t8, tb, tf = [], [], []
        for _ in range(rounds):
            f = timed(g0); a = timed(g8); b = timed(gb)
            tf.append(f); t8.append(a - f); tb.append(b - f)
        med = lambda v: sorted(v)[len(v) // 2]
        u8, ub = med(t8), med(tb)
        b8, bb = n * k + 4 * n, 2 * n * k
        lines.append(f"{name:<34} {u8:8.2f} {b8 / u8 * 1e-6:6.2f} {ub:8.2f} {bb / ub * 1e-6:6.2f} {ub / u8:9.2f} {med(tf):9.1f}")
        print(lines[-1], flush=True)
        worst = ub / u8 if worst is None else min(worst, ub / u8)
        del wb, w8, sc, g0, g8, gb
    lines.append(f"# smallest bf16 : fp8 time ratio {worst:.2f} ({'every FP8 launch is no slower' if worst >= 1 else 'AN FP8 LAUNCH IS SLOWER'} "
                 "than its bf16 counterpart)")
    print(lines[-1])
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def mxfp4_mode(out_path=None, rounds=7, reps=24):
    """--mxfp4 [FILE]: the method of --fp8 with three launches per shape - bf16, FP8 and MXFP4 - in interleaved rounds of one
    process: per shape four captured graphs of `reps` iterations ([flush], [flush, launch] per format), a launch's time is
    (its graph - the flush graph) / reps within the round, the reported figure the median over the rounds.  bytes: the weights
    (+ 4 N of FP8 row scales; + N K / 32 of MXFP4 block scales).  Acceptance: no MXFP4 launch slower than the FP8 launch of
    the same shape; the margin is the spread (max - min) of that FP8 launch's rounds."""
    g, shapes, graph_of, timed = _fixture(reps)
    lines = [f"# tools/time_gemv.py --mxfp4 on {torch.cuda.get_device_name(0)}: HBM-cold launches (1 GiB flush before each), "
             f"median of {rounds} interleaved rounds of {reps} launches; us per launch, TB/s over the weight bytes",
             f"{'shape':<34} {'bf16 us':>8} {'TB/s':>6} {'fp8 us':>8} {'TB/s':>6} {'mxfp4 us':>9} {'TB/s':>6} {'fp8 spread':>11} "
             f"{'bf16/mx':>8} {'fp8/mx':>7}  verdict"]
    med = lambda v: sorted(v)[len(v) // 2]
    slower = []
    for name, n, k, fn in shapes:
        wb = (torch.randn(n, k, device=dev, generator=g) * 0.02).bfloat16()
        w8, s8 = tensor_op.quantize_fp8_rows(wb)
        w4, s4 = tensor_op.quantize_mxfp4_rows(wb)
        g0, gb = graph_of(None), graph_of(lambda: fn(wb, None))
        g8, g4 = graph_of(lambda: fn(w8, s8)), graph_of(lambda: fn(w4, s4))
        tb, t8, t4 = [], [], []
        for _ in range(rounds):
            f = timed(g0); b = timed(gb); a = timed(g8); c = timed(g4)
            tb.append(b - f); t8.append(a - f); t4.append(c - f)
        ub, u8, u4, spread = med(tb), med(t8), med(t4), max(t8) - min(t8)
        bb, b8, b4 = 2 * n * k, n * k + 4 * n, n * k // 2 + n * k // 32
        ok = u4 <= u8 + spread
        if not ok:
            slower.append(name)
        lines.append(f"{name:<34} {ub:8.2f} {bb / ub * 1e-6:6.2f} {u8:8.2f} {b8 / u8 * 1e-6:6.2f} {u4:9.2f} {b4 / u4 * 1e-6:6.2f} "
                     f"{spread:11.2f} {ub / u4:8.2f} {u8 / u4:7.2f}  {'no slower than FP8' if ok else 'SLOWER THAN FP8'}")
        print(lines[-1], flush=True)
        del wb, w8, s8, w4, s4, g0, gb, g8, g4
    lines.append("# " + ("every MXFP4 launch is no slower than the FP8 launch of its shape" if not slower else
                         "MXFP4 LAUNCHES SLOWER THAN FP8 beyond the FP8 rounds' spread: " + "; ".join(slower)))
    print(lines[-1])
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if "--fp8" in sys.argv:
    i = sys.argv.index("--fp8")
    fp8_mode(sys.argv[i + 1] if len(sys.argv) > i + 1 else None)
    sys.exit(0)
if "--mxfp4" in sys.argv:
    i = sys.argv.index("--mxfp4")
    mxfp4_mode(sys.argv[i + 1] if len(sys.argv) > i + 1 else None)
    sys.exit(0)
L = 32
g = torch.Generator(device=dev).manual_seed(0)
def w(n, k): return [(torch.randn(n, k, device=dev, generator=g) * 0.02).bfloat16() for _ in range(L)]
wqkv, wo, wgu, wd = w(6144, 4096), w(4096, 4096), w(28672, 4096), w(4096, 14336)
x = torch.randn(1, 1, 4096, device=dev, generator=g).bfloat16(); res = torch.randn(1, 1, 4096, device=dev, generator=g).bfloat16()
xi = torch.randn(1, 1, 14336, device=dev, generator=g).bfloat16()
nw = torch.ones(4096, device=dev, dtype=torch.bfloat16)
cs = llama.build_cos_sin_cache(llama.LLAMA_3_1_8B, 4096, torch.device(dev), torch.bfloat16)
pos = torch.tensor([[100]], device=dev); row = torch.tensor([5], device=dev)
kc = torch.zeros(1, 8, 64, 128, device=dev, dtype=torch.bfloat16); vc = torch.zeros_like(kc)
def t(name, fn, mb):
    s_ = torch.cuda.Stream()
    with torch.cuda.stream(s_):
        for l in range(L): fn(l)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s_):          # captured: no host launch gaps, like the decode step
        for l in range(L): fn(l)
    gr.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        gr.replay()
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (5 * L)
    print(f"{name:<34} {us:7.2f} us  {mb / us * 1e-0:7.1f} GB/s" .replace("GB/s", "MB/us = %.2f TB/s" % (mb / us)))
t("qkv (norm + gemv + rope/append)", lambda l: tensor_op.norm_qkv_rope_update(x, res, nw, 1e-5, wqkv[l], None, cs, pos, row, kc, vc, 32, 8), 50.33)
t("qkv plain gemv", lambda l: tensor_op.linear_decode(x, wqkv[l]), 50.33)
t("o gemv", lambda l: tensor_op.linear_decode(x, wo[l]), 33.55)
t("gate/up (norm + gemv + silu)", lambda l: tensor_op.norm_linear_decode(x, res, nw, 1e-5, wgu[l], fuse_silu_mul=True), 234.9)
t("gate/up plain gemv + silu", lambda l: tensor_op.linear_decode(x, wgu[l], fuse_silu_mul=True), 234.9)
t("down gemv", lambda l: tensor_op.linear_decode(xi, wd[l]), 117.4)
