#!/usr/bin/env python3
"""Bit identity of the decode GEMV entries and the small-M rows entries between two builds of the library.

    SKV_LIB_PATH=<library A> python tools/gemv_ab_bits.py --dump a.pt      (one fresh process per library)
    python tools/gemv_ab_bits.py --dump b.pt
    python tools/gemv_ab_bits.py --compare a.pt b.pt

--dump runs every public GEMV entry of the three formats (skv_gemv.hip, skv_gemv_fp8.hip, skv_gemv_mxfp4.hip) on seeded inputs -
the shapes of the exact tests and the Llama-3.1-8B shapes - and the three rows entries (skv_rows_gemm.hip, skv_rows_gemm_fp8.hip,
skv_rows_gemm_mxfp4.hip) on Gaussian data, and stores every output tensor as raw 16-bit words; --compare is torch.equal."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import torch

DEV = "cuda:0"
# the rows entries: token rows, plain N (with and without bias), the SiLU pair N, K per format, the Llama-3.1-8B projections
ROWS_M, ROWS_N, ROWS_SILU_N = (2, 8, 9, 16, 17, 32), (48, 6160, 16400), 2 * 1003
ROWS_K = {"bf16": (96, 288, 1056, 8224), "fp8": (192, 576, 2112, 8256), "mxfp4": (384, 1152, 4224, 8320)}
ROWS_LLAMA = ((6144, 4096, 0), (4096, 4096, 0), (28672, 4096, 1), (4096, 14336, 0))       # (N, K, silu) at M = 8 and 24
# per format: elements of a k-step, then (waves per workgroup, k-steps in flight) of every branch of skv_rows_pick
ROWS_SHAPES = {"bf16": (32, {"g1 paired": (8, 8), "g1": (8, 8), "g1 two tiles": (8, 8), "g2 1/2x8": (8, 4), "g2 2/2x8": (8, 4),
                             "g2 2/1x8": (8, 4), "g2 2/4x4": (4, 4)}),
               "fp8": (64, {"g1 paired": (8, 8), "g1": (8, 4), "g1 two tiles": (8, 4), "g2 1/2x8": (8, 4), "g2 2/2x8": (8, 4),
                            "g2 2/1x8": (8, 4), "g2 2/4x4": (4, 2)}),
               "mxfp4": (128, {"g1 paired": (8, 4), "g1": (8, 4), "g1 two tiles": (8, 2), "g2 1/2x8": (8, 2), "g2 2/2x8": (8, 2),
                               "g2 2/1x8": (8, 2), "g2 2/4x4": (4, 2)})}


def rows_coverage(fmt):
    """The small rows shapes reach all seven branches, and in either generation a wave that runs unrolled batches, one that runs
    single-step tails and a K with fewer k-steps than waves (the order of the f32 sums differs between those paths)."""
    from dense_ref import expected_branch
    step, shapes = ROWS_SHAPES[fmt]
    reached = set()
    for M in ROWS_M:
        for N in ROWS_N + (ROWS_SILU_N,):
            for K in ROWS_K[fmt]:
                b = expected_branch(M, N, K)
                nwv, u = shapes[b]
                S = K // step
                per = -(-S // nwv)
                last = S - per * ((S - 1) // per)                       # steps of the last wave that has any
                reached |= {b, (b[:2], "batch") if per >= u else None, (b[:2], "tail") if per % u or last % u else None,
                            (b[:2], "fewer steps than waves") if S < nwv else None}
    want = set(shapes) | {(g, c) for g in ("g1", "g2") for c in ("batch", "tail", "fewer steps than waves")}
    assert reached - {None} == want, (fmt, want - reached)


def dump(path):
    from shadowkv_amd import _lib, tensor_op
    L, p, st = _lib.lib(), _lib.ptr, _lib.current_stream_handle()
    g = torch.Generator(device=DEV).manual_seed(7)
    out = {}

    def rnd(*shape, s=1.0):
        return (torch.randn(*shape, device=DEV, generator=g) * s).bfloat16()

    def buf(n):
        return torch.full((n + 8,), 1000.0, dtype=torch.bfloat16, device=DEV)

    def keep(name, rc, *ts):
        assert rc == 0, (name, rc)
        torch.cuda.synchronize()
        for i, t in enumerate(ts):
            out[f"{name}/{i}"] = t.view(torch.int16).cpu().clone()

    def both(N, K):
        w = rnd(N, K, s=0.02)
        w8, sc = tensor_op.quantize_fp8_rows(w)
        return w, w8, sc

    def mx(w):
        return tensor_op.quantize_mxfp4_rows(w)

    # plain / bias / SiLU pair (no norm): the shapes of the exact tests, then O, down and gate/up of Llama-3.1-8B
    # (the last seven: the MXFP4 exact tests' shapes - their K set at N = 37, the four-rows-per-wave instance, the odd SiLU pair)
    for N, K in [(1, 512), (7, 520), (9, 1024), (20, 1040), (4101, 13696), (8193, 1000), (8208, 1024), (8209, 512), (4096, 4096),
                 (4096, 14336), (2006, 13696), (28672, 4096), (37, 1024), (37, 2048), (37, 2080), (37, 13696), (8200, 2048),
                 (8200, 2080), (22, 2080)]:
        w, w8, sc = both(N, K)
        x, b = rnd(K), rnd(N)
        is_mx = K % 32 == 0 and K >= 1024
        if is_mx:
            w4, s4 = mx(w)
        for bias in (None, b):
            y = buf(N)
            keep(f"gemv_bf16 {N}x{K} bias {bias is not None}", L.skv_gemv_bf16(p(w), p(x), p(bias), p(y), N, K, 0, st), y)
            if K % 16 == 0 and K >= 1024:
                y = buf(N)
                keep(f"gemv_fp8 {N}x{K} bias {bias is not None}", L.skv_gemv_fp8(p(w8), p(sc), p(x), p(bias), p(y), N, K, 0, st), y)
            if is_mx:
                y = buf(N)
                keep(f"gemv_mxfp4 {N}x{K} bias {bias is not None}", L.skv_gemv_mxfp4(p(w4), p(s4), p(x), p(bias), p(y), N, K, 0, st), y)
        if N % 2 == 0:
            y = buf(N // 2)
            keep(f"gemv_bf16 silu {N}x{K}", L.skv_gemv_bf16(p(w), p(x), 0, p(y), N, K, 1, st), y)
            if K % 16 == 0 and K >= 1024:
                y = buf(N // 2)
                keep(f"gemv_fp8 silu {N}x{K}", L.skv_gemv_fp8(p(w8), p(sc), p(x), 0, p(y), N, K, 1, st), y)
            if is_mx:
                y = buf(N // 2)
                keep(f"gemv_mxfp4 silu {N}x{K}", L.skv_gemv_mxfp4(p(w4), p(s4), p(x), 0, p(y), N, K, 1, st), y)
    # norm prologue: plain / bias / SiLU pair, with and without a residual; range keys (lm_head)
    K = 4096
    x, res, nw = rnd(K), rnd(K), (1 + 0.1 * torch.randn(K, device=DEV, generator=g)).bfloat16()
    for N in (1, 17, 20, 37, 4101, 8193, 2 * 1003, 6144, 28672):
        w, w8, sc = both(N, K)
        w4, s4 = mx(w)
        b = rnd(N)
        for r in (res, None):
            for bias in (None, b):
                for silu in ((0, 1) if N % 2 == 0 and bias is None else (0,)):
                    No = N // 2 if silu else N
                    tag = f"{N}x{K} residual {r is not None} bias {bias is not None} silu {silu}"
                    y, h = buf(No), buf(K)
                    keep("norm_gemv_bf16 " + tag, L.skv_norm_gemv_bf16(p(w), p(x), p(r), p(nw), 1e-5, p(h), p(bias), p(y), N, K, silu, st), y, h)
                    y, h = buf(No), buf(K)
                    keep("norm_gemv_fp8 " + tag,
                         L.skv_norm_gemv_fp8(p(w8), p(sc), p(x), p(r), p(nw), 1e-5, p(h), p(bias), p(y), N, K, silu, st), y, h)
                    y, h = buf(No), buf(K)
                    keep("norm_gemv_mxfp4 " + tag,
                         L.skv_norm_gemv_mxfp4(p(w4), p(s4), p(x), p(r), p(nw), 1e-5, p(h), p(bias), p(y), N, K, silu, st), y, h)
    for N in (16, 48, 32000, 128256):
        w, w8, sc = both(N, K)
        w4, s4 = mx(w)
        b = rnd(N)
        for bias in (None, b):
            y, h, keys = buf(N), buf(K), torch.full((N // 16 + 8,), -1, dtype=torch.int16, device=DEV)
            keep(f"rangemax_bf16 {N} bias {bias is not None}",
                 L.skv_norm_gemv_rangemax_bf16(p(w), p(x), p(res), p(nw), 1e-5, p(h), p(bias), p(y), N, K, p(keys), st), y, h, keys)
            y, h, keys = buf(N), buf(K), torch.full((N // 16 + 8,), -1, dtype=torch.int16, device=DEV)
            keep(f"rangemax_fp8 {N} bias {bias is not None}",
                 L.skv_norm_gemv_rangemax_fp8(p(w8), p(sc), p(x), p(res), p(nw), 1e-5, p(h), p(bias), p(y), N, K, p(keys), st), y, h, keys)
            y, h, keys = buf(N), buf(K), torch.full((N // 16 + 8,), -1, dtype=torch.int16, device=DEV)
            keep(f"rangemax_mxfp4 {N} bias {bias is not None}",
                 L.skv_norm_gemv_rangemax_mxfp4(p(w4), p(s4), p(x), p(res), p(nw), 1e-5, p(h), p(bias), p(y), N, K, p(keys), st), y, h, keys)
        del w, w8, sc, w4, s4
    # QKV epilogue (norm K = 4096, plain K = 1040 and bf16 K = 520), NeoX and GLM; the q-only launch
    ROWS, CS = 12, 40
    for Hq, Hkv, glm in ((32, 8, False), (4, 1, False), (32, 4, True), (2, 1, True)):
        N = (Hq + 2 * Hkv) * 128
        cs = (torch.rand(CS, 64 if glm else 128, device=DEV, generator=g) * 2 - 1).bfloat16()
        pos, row, ov = torch.tensor([17], device=DEV), torch.tensor([5], device=DEV), rnd(Hq * 128)
        for Kq in (4096, 1040, 520):
            w, w8, sc = both(N, Kq)
            w4, s4 = mx(w) if Kq == 4096 else (None, None)        # (1040 is off MXFP4's k-step: its QKV launch runs with the norm only)
            xq, b = rnd(Kq), rnd(N)
            norm = Kq == 4096
            for bias in (None, b):
                for override in (None, ov):
                    for fmt in {4096: ("bf16", "fp8", "mxfp4"), 1040: ("bf16", "fp8"), 520: ("bf16",)}[Kq]:
                        q, h = buf(Hq * 128), buf(Kq)
                        kc = torch.zeros(1, Hkv, ROWS, 128, device=DEV, dtype=torch.bfloat16)
                        vc = torch.zeros_like(kc)
                        tail = (p(res) if norm else 0, p(nw) if norm else 0, 1e-5, p(h) if norm else 0, p(bias), p(cs), p(pos), p(row),
                                p(override), p(q), p(kc), p(vc), Kq, Hq, Hkv, 128, cs.stride(0), CS, kc.stride(1), ROWS, 2 if glm else 1, st)
                        rc = L.skv_qkv_gemv_rope_update(p(w), p(xq), *tail) if fmt == "bf16" else \
                            L.skv_qkv_gemv_rope_update_fp8(p(w8), p(sc), p(xq), *tail) if fmt == "fp8" else \
                            L.skv_qkv_gemv_rope_update_mxfp4(p(w4), p(s4), p(xq), *tail)
                        keep(f"qkv_{fmt} Hq {Hq} Hkv {Hkv} glm {glm} K {Kq} bias {bias is not None} override {override is not None}",
                             rc, q, h, kc, vc)
                    if norm:
                        q, h = buf(Hq * 128), buf(Kq)
                        keep(f"q_only Hq {Hq} Hkv {Hkv} glm {glm} bias {bias is not None} override {override is not None}",
                             L.skv_q_gemv_rope(p(w), p(xq), p(res), p(nw), 1e-5, p(h), p(bias), p(cs), p(pos), p(override), p(q), Kq, Hq, Hkv,
                                               128, cs.stride(0), CS, 2 if glm else 1, st), q, h)
    # near-pull launches: gate/up (list 0) and down (list 1) in front of an early state after one selection step
    from test_gpu_kv_cache import _headline_cache
    for fmt in ("bf16", "fp8", "mxfp4"):
        c, cs, gc = _headline_cache(8, False, L=16384, seed=41)
        c.near_lists = 2
        c.enable_early_fetch(near=True)
        qq = (torch.randn(1, 32, 1, 128, device=DEV, generator=gc) * 1.5).bfloat16()
        c.select_fetch_attend_inplace(0, qq, cs, kv_len=c.sparse_end + 2)
        torch.cuda.synchronize()
        gs = torch.Generator(device=DEV).manual_seed(9)
        for N, Kd in ((18, 4096), (28672, 4096)):
            w = (torch.randn(N, Kd, device=DEV, generator=gs) * 0.02).bfloat16()
            w8, sc = tensor_op.quantize_fp8_rows(w)
            w4, s4 = mx(w) if fmt == "mxfp4" else (None, None)
            y, h = buf(N // 2), buf(Kd)
            a = c.near_pull_args(0)
            rc = L.skv_norm_gemv_near_pull_bf16(p(w), p(x), p(res), p(nw), 1e-5, p(h), p(y), N, Kd, *a, st) if fmt == "bf16" else \
                L.skv_norm_gemv_near_pull_fp8(p(w8), p(sc), p(x), p(res), p(nw), 1e-5, p(h), p(y), N, Kd, *a, st) if fmt == "fp8" else \
                L.skv_norm_gemv_near_pull_mxfp4(p(w4), p(s4), p(x), p(res), p(nw), 1e-5, p(h), p(y), N, Kd, *a, st)
            keep(f"near gate/up {fmt} {N}", rc, y, h, c.near_published_ids(0).to(torch.int32).view(torch.int16))
        for N, Kd in ((9, 1056 if fmt == "mxfp4" else 1040), (4096, 14336)):       # (1040 is off MXFP4's k-step)
            w = (torch.randn(N, Kd, device=DEV, generator=gs) * 0.02).bfloat16()
            w8, sc = tensor_op.quantize_fp8_rows(w)
            w4, s4 = mx(w) if fmt == "mxfp4" else (None, None)
            xd, b = (torch.randn(Kd, device=DEV, generator=gs)).bfloat16(), (torch.randn(N, device=DEV, generator=gs)).bfloat16()
            y = buf(N)
            a = c.near_pull_args(0, 1)
            rc = L.skv_gemv_near_pull_bf16(p(w), p(xd), p(b), p(y), N, Kd, *a, st) if fmt == "bf16" else \
                L.skv_gemv_near_pull_fp8(p(w8), p(sc), p(xd), p(b), p(y), N, Kd, *a, st) if fmt == "fp8" else \
                L.skv_gemv_near_pull_mxfp4(p(w4), p(s4), p(xd), p(b), p(y), N, Kd, *a, st)
            keep(f"near down {fmt} {N}", rc, y, c.near_published_ids(0).to(torch.int32).view(torch.int16))
        del c
    # the rows entries: Gaussian weights and activations (the integer banks of the exact tests are blind to the summation order)
    for fmt in ("bf16", "fp8", "mxfp4"):
        rows_coverage(fmt)
        cases = [(M, N, K, N == ROWS_SILU_N) for N in ROWS_N + (ROWS_SILU_N,) for K in ROWS_K[fmt] for M in ROWS_M]
        cases += [(M, N, K, bool(silu)) for N, K, silu in ROWS_LLAMA for M in (8, 24)]
        w = None
        for M, N, K, silu in cases:
            if w is None or w.shape != (N, K):
                w, w8, sc = both(N, K)
                w4, s4 = mx(w) if fmt == "mxfp4" else (None, None)
                xr, b = rnd(max(ROWS_M), K), rnd(N)
            xm = xr[:M].contiguous()
            for bias in ((None,) if silu else (None, b)):
                No = N // 2 if silu else N
                y = buf(M * No)
                rc = L.skv_linear_rows_bf16(p(w), p(xm), p(bias), p(y), M, N, K, int(silu), st) if fmt == "bf16" else \
                    L.skv_linear_rows_fp8(p(w8), p(sc), p(xm), p(bias), p(y), M, N, K, int(silu), st) if fmt == "fp8" else \
                    L.skv_linear_rows_mxfp4(p(w4), p(s4), p(xm), p(bias), p(y), M, N, K, int(silu), st)
                keep(f"rows_{fmt} M {M} {N}x{K} silu {int(silu)} bias {bias is not None}", rc, y)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(out, path)
    print(f"{len(out)} tensors from {_lib.LIB_PATH} -> {path}")


def compare(a_path, b_path):
    a, b = torch.load(a_path), torch.load(b_path)
    assert a.keys() == b.keys(), "the two dumps hold different entries"
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    for k in bad:
        print(f"DIFFERENT  {k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} words")
    groups = {}
    for k in a:
        groups.setdefault(k.split(" ")[0], []).append(k)
    for name, ks in groups.items():
        print(f"{name:<22} {len(ks):4d} tensors  {'EQUAL' if not any(k in bad for k in ks) else 'DIFFERENT'}")
    print(f"{len(a) - len(bad)} of {len(a)} tensors bit-identical")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
