"""Event-timed small-M projection kernel (skv_linear_rows_bf16) at the decode shapes, cycling 8 weight copies.
--fp8 [FILE]: the FP8 rows kernel (skv_linear_rows_fp8) against the bf16 launch and the dequantising fallback, HBM-cold.
--mxfp4 [FILE]: the MXFP4 rows kernel (skv_linear_rows_mxfp4) against the FP8 rows launch, the bf16 launch and its fallback."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shadowkv_amd import _lib


def fp8_mode(out_path=None, rounds=7, reps=24):
    """Per layer shape and M in {8, 16, 24, 32}, in ONE process: the FP8 launch, the unchanged skv_linear_rows_bf16 launch on the
    dequantised matrix and the current fallback (dequantise + F.linear).  The method of tools/time_gemv.py --fp8: per launch a
    captured graph of `reps` iterations [flush, launch] next to a graph of [flush] alone - the flush rewrites a 1 GiB buffer, so
    every launch reads its weights from HBM - replayed in interleaved rounds; a launch's time is (its graph - the flush graph)
    / reps within the round, the reported figure the median over the rounds.  TB/s: over the FP8 bytes (+ 4 N of scales).
    Acceptance: no FP8 launch slower than the bf16 launch of the same shape and M."""
    from shadowkv_amd import tensor_op
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    flush = torch.zeros(1 << 30, dtype=torch.uint8, device=dev)
    shapes = [("qkv 6144x4096", 6144, 4096, False), ("o 4096x4096", 4096, 4096, False),
              ("gate/up 28672x4096 (silu)", 28672, 4096, True), ("down 4096x14336", 4096, 14336, False)]

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

    med = lambda v: sorted(v)[len(v) // 2]
    lines = [f"# tools/time_rows_gemm.py --fp8 on {torch.cuda.get_device_name(0)}: HBM-cold launches (1 GiB flush before each), "
             f"median of {rounds} interleaved rounds of {reps} launches; us per launch, TB/s over the FP8 weight bytes",
             f"{'shape':<26} {'M':>3} {'fp8 us':>8} {'TB/s':>6} {'bf16 us':>8} {'fallback us':>12} {'bf16/fp8':>9} {'fallback/fp8':>13}"]
    losers = []
    for name, n, k, silu in shapes:
        wb = (torch.randn(n, k, device=dev, generator=g) * 0.02).bfloat16()
        w8, sc = tensor_op.quantize_fp8_rows(wb)
        wd = tensor_op.dequantize_fp8_rows(w8, sc)        # the matrix the bf16 launch reads: the same numbers, rounded to bf16
        del wb
        g0 = graph_of(None)
        for M in (8, 16, 24, 32):
            x = torch.randn(M, 1, k, device=dev, generator=g).bfloat16()
            y = torch.empty(M, 1, n // 2 if silu else n, device=dev, dtype=torch.bfloat16)
            g8 = graph_of(lambda: tensor_op.linear_decode(x, w8, fuse_silu_mul=silu, out=y, w_scale=sc, fp8_rows="native"))
            gb = graph_of(lambda: tensor_op.linear_decode(x, wd, fuse_silu_mul=silu, out=y))
            gf = graph_of(lambda: tensor_op.linear_decode(x, w8, fuse_silu_mul=silu, out=y, w_scale=sc))
            t8, tb, tf = [], [], []
            for _ in range(rounds):
                f = timed(g0); a = timed(g8); b = timed(gb); c = timed(gf)
                t8.append(a - f); tb.append(b - f); tf.append(c - f)
            u8, ub, uf = med(t8), med(tb), med(tf)
            lines.append(f"{name:<26} {M:3d} {u8:8.2f} {(n * k + 4 * n) / u8 * 1e-6:6.2f} {ub:8.2f} {uf:12.2f} {ub / u8:9.2f} {uf / u8:13.2f}")
            print(lines[-1], flush=True)
            if ub < u8:
                losers.append(f"{name} M {M} ({u8:.2f} us against {ub:.2f} us)")
            del g8, gb, gf
        del w8, sc, wd, g0
    lines.append("# acceptance: " + ("every FP8 launch is no slower than the bf16 launch of the same shape and M" if not losers
                                     else "AN FP8 LAUNCH IS SLOWER THAN ITS bf16 COUNTERPART: " + "; ".join(losers)))
    print(lines[-1])
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def mxfp4_mode(out_path=None, rounds=7, reps=24):
    """--mxfp4 [FILE]: the method of --fp8 in ONE process, per layer shape and M in {8, 16, 24, 32}: the MXFP4 rows launch, the FP8
    rows launch, the skv_linear_rows_bf16 launch on the dequantised matrix - captured graphs of `reps` iterations [flush, launch]
    next to a graph of [flush] alone, replayed in interleaved rounds, a launch's time (its graph - the flush graph) / reps within
    the round - and the current MXFP4 fallback (dequantise + F.linear), which builds a host constant and is therefore timed
    eagerly the same way ([flush, call] x reps between two events, minus [flush] x reps).  The reported figure is the median
    over the rounds.  TB/s: over the MXFP4 bytes (nibbles + N K / 32 scale bytes).
    Acceptance (DESIGN.md sections 12 / 12.1): no MXFP4 launch slower than the FP8 launch of the same shape and M; the margin
    is the spread (max - min) of that FP8 launch's rounds."""
    from shadowkv_amd import tensor_op
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    flush = torch.zeros(1 << 30, dtype=torch.uint8, device=dev)
    shapes = [("qkv 6144x4096", 6144, 4096, False), ("o 4096x4096", 4096, 4096, False),
              ("gate/up 28672x4096 (silu)", 28672, 4096, True), ("down 4096x14336", 4096, 14336, False)]

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

    def timed_eager(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            flush.add_(1)
            if fn is not None:
                fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    med = lambda v: sorted(v)[len(v) // 2]
    lines = [f"# tools/time_rows_gemm.py --mxfp4 on {torch.cuda.get_device_name(0)}: HBM-cold launches (1 GiB flush before each), "
             f"median of {rounds} interleaved rounds of {reps} launches; us per launch, TB/s over the MXFP4 weight bytes",
             f"{'shape':<26} {'M':>3} {'mxfp4 us':>9} {'TB/s':>6} {'fp8 us':>8} {'fp8 spread':>11} {'bf16 us':>8} {'fallback us':>12} "
             f"{'fp8/mx':>7} {'bf16/mx':>8} {'fallback/mx':>12}  verdict"]
    losers = []
    for name, n, k, silu in shapes:
        wb = (torch.randn(n, k, device=dev, generator=g) * 0.02).bfloat16()
        w4, s4 = tensor_op.quantize_mxfp4_rows(wb)
        w8, s8 = tensor_op.quantize_fp8_rows(wb)
        wd = tensor_op.dequantize_mxfp4_rows(w4, s4)      # the matrix the bf16 launch reads: the MXFP4 numbers, exact in bf16
        del wb
        g0 = graph_of(None)
        for M in (8, 16, 24, 32):
            x = torch.randn(M, 1, k, device=dev, generator=g).bfloat16()
            y = torch.empty(M, 1, n // 2 if silu else n, device=dev, dtype=torch.bfloat16)
            g4 = graph_of(lambda: tensor_op.linear_decode(x, w4, fuse_silu_mul=silu, out=y, w_scale=s4, mxfp4_rows="native"))
            g8 = graph_of(lambda: tensor_op.linear_decode(x, w8, fuse_silu_mul=silu, out=y, w_scale=s8, fp8_rows="native"))
            gb = graph_of(lambda: tensor_op.linear_decode(x, wd, fuse_silu_mul=silu, out=y))
            fallback = lambda: tensor_op.linear_decode(x, w4, fuse_silu_mul=silu, out=y, w_scale=s4)
            fallback(); timed_eager(None)
            t4, t8, tb, tf = [], [], [], []
            for _ in range(rounds):
                f = timed(g0); a = timed(g4); b = timed(g8); c = timed(gb)
                t4.append(a - f); t8.append(b - f); tb.append(c - f)
                fe = timed_eager(None); tf.append(timed_eager(fallback) - fe)
            u4, u8, ub, uf, spread = med(t4), med(t8), med(tb), med(tf), max(t8) - min(t8)
            ok = u4 <= u8 + spread
            lines.append(f"{name:<26} {M:3d} {u4:9.2f} {(n * k // 2 + n * k // 32) / u4 * 1e-6:6.2f} {u8:8.2f} {spread:11.2f} {ub:8.2f} "
                         f"{uf:12.2f} {u8 / u4:7.2f} {ub / u4:8.2f} {uf / u4:12.2f}  {'no slower than FP8' if ok else 'SLOWER THAN FP8'}")
            print(lines[-1], flush=True)
            if not ok:
                losers.append(f"{name} M {M} ({u4:.2f} us against {u8:.2f} us, spread {spread:.2f})")
            del g4, g8, gb
        del w4, s4, w8, s8, wd, g0
    lines.append("# acceptance: " + ("every MXFP4 rows launch is no slower than the FP8 rows launch of the same shape and M" if not losers
                                     else "MXFP4 ROWS LAUNCHES SLOWER THAN FP8 beyond the FP8 rounds' spread: " + "; ".join(losers)))
    print(lines[-1])
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if "--mxfp4" in sys.argv:
    i = sys.argv.index("--mxfp4")
    mxfp4_mode(sys.argv[i + 1] if len(sys.argv) > i + 1 else None)
    sys.exit(0)
if "--fp8" in sys.argv:
    i = sys.argv.index("--fp8")
    fp8_mode(sys.argv[i + 1] if len(sys.argv) > i + 1 else None)
    sys.exit(0)
L = _lib.lib(); dev = "cuda:0"
M = int(sys.argv[1]) if len(sys.argv) > 1 else 8
for (N, K, silu) in ((6144, 4096, 0), (4096, 4096, 0), (28672, 4096, 1), (4096, 14336, 0)):
    ws = [torch.randn(N, K, device=dev).bfloat16() for _ in range(8)]
    x = torch.randn(M, K, device=dev).bfloat16()
    y = torch.empty(M, N // 2 if silu else N, device=dev, dtype=torch.bfloat16)
    st = torch.cuda.current_stream().cuda_stream
    def run():
        for w in ws:
            L.skv_linear_rows_bf16(w.data_ptr(), x.data_ptr(), 0, y.data_ptr(), M, N, K, silu, st)
    run(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); [run() for _ in range(10)]; e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / 80
    print(f"M={M} N={N} K={K} silu={silu}: {us:.2f} us  {N*K*2/us*1e-6:.2f} TB/s", flush=True)
