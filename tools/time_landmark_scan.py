#!/usr/bin/env python3
"""The landmark scan over a bf16 and over an FP8 (e4m3) landmark table, timed alternately in one process.

One 122 K synthetic context per landmark dtype (build_synthetic_context, Llama-3.1-8B shapes, bs 1, a few layers); the scan's
inputs at blocks = 8 / 64 / 192 (bs 1 / 8 / 24 at 8 KV heads) are that context's landmark tables put side by side.  Every timed
launch reads another table of a ring of at least 1 GB of bf16 tables (the FP8 ring has the same number of tables), as the
layers of a decode step do: nothing is served from the 256 MB Infinity Cache.  Two forms: the scan alone (skv_score_landmarks
/ _fp8: logits [B][G][N] + partials) and the launch of the fused selection (skv_score_landmarks_fused / _fp8: keys + slot-major
logits + partials).  Per (form, blocks): `--rounds` rounds, each timing the bf16 ring and then the FP8 ring with device events;
median and minimum us per launch over the rounds, the spread of the bf16 rounds ((max - min) / median), and algorithmic GB/s:
B * N * 256 bytes for bf16 against B * N * (128 + 4) for FP8 (bytes + scales).

usage: tools/time_landmark_scan.py [--blocks 8,64,192] [--rounds 9] [--passes 4] [--layers 2] [--forms plain,fused] [--out FILE]
(FILE is appended to).  Kernel time: run it under `rocprofv3 --kernel-trace --stats` with --rounds 1 --passes 1, in a run of its
own."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from shadowkv_amd import _lib, llama  # noqa: E402

CTX, DEV = 122 * 1024, "cuda:0"
ALPHA = 1.0 / math.sqrt(128)


def scan_bytes(blocks, n, fp8):
    """what the scan must read of the landmark table (the q rows and the outputs are three orders of magnitude below)"""
    return blocks * n * (128 + 4) if fp8 else blocks * n * 256


def build(landmark_dtype, layers):
    m = llama.DecoderLM(cfg=llama.LLAMA_3_1_8B, batch_size=1, max_length=CTX, device=DEV, sparse_budget=2048, rank=160, chunk_size=8,
                        num_layers=layers, chunk_layout="inplace", overlap_attention=True, landmark_dtype=landmark_dtype)
    q = llama.build_synthetic_context(m, CTX, seed=4321)
    c = m.kv_cache
    return c.k_landmark.clone(), None if c.k_landmark_scale is None else c.k_landmark_scale.clone(), c.k_landmark_idx.clone(), q


def ring(lm, scale, idx, blocks, count):
    """`count` inputs of `blocks` blocks: the layers' tables [L][1][8][N][128] side by side, starting at another layer each"""
    L, reps = lm.shape[0], blocks // 8
    out = []
    for j in range(count):
        pick = [(j + i) % L for i in range(reps)]
        t = torch.cat([lm[p][0] for p in pick]).contiguous()
        s = None if scale is None else torch.cat([scale[p][0] for p in pick]).contiguous()
        out.append((t, s, torch.cat([idx[p][0] for p in pick]).contiguous()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="8,64,192")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--passes", type=int, default=4, help="passes over the ring per timed window")
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--forms", default="plain,fused")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    G = 4
    src = {}
    for dt in ("bf16", "fp8_e4m3"):
        src[dt] = build(dt, a.layers)
        torch.cuda.empty_cache()
    n = src["bf16"][0].shape[-2]
    assert src["fp8_e4m3"][0].shape[-2] == n and src["fp8_e4m3"][0].element_size() == 1
    q1 = src["bf16"][3].view(8, G, 128)
    st = torch.cuda.current_stream().cuda_stream
    lines = [f"# tools/time_landmark_scan.py on {torch.cuda.get_device_name(0)}: 122 K synthetic context ({n} landmarks per KV head, G = {G}), "
             f"{a.rounds} alternating rounds x {a.passes} passes over a ring of tables >= 1 GB (bf16), device events"]
    for form in a.forms.split(","):
        for blocks in (int(b) for b in a.blocks.split(",")):
            count = max(2, -(-(1 << 30) // scan_bytes(blocks, n, False)))
            q = q1.repeat(blocks // 8, 1, 1).contiguous()
            T = (n + 255) // 256
            D = torch.empty(blocks, G, n, device=DEV, dtype=torch.bfloat16)
            pm, ps = torch.empty(blocks, T, G, device=DEV), torch.empty(blocks, T, G, device=DEV)
            ws = torch.empty(L.skv_select_workspace_bytes(blocks, G, n), dtype=torch.uint8, device=DEV)
            state = torch.zeros(L.skv_select_state_bytes(blocks, G), dtype=torch.uint8, device=DEV)
            rings = {dt: ring(src[dt][0], src[dt][1], src[dt][2], blocks, count) for dt in src}

            def launch(dt, t, s, idx):
                lm = (t.data_ptr(),) if s is None else (t.data_ptr(), s.data_ptr())
                sfx = "" if s is None else "_fp8"
                if form == "fused":
                    rc = getattr(L, "skv_score_landmarks_fused" + sfx)(q.data_ptr(), *lm, idx.data_ptr(), ws.data_ptr(), blocks, G, n, ALPHA,
                                                                        state.data_ptr(), 0, 0, 0, st)
                else:
                    rc = getattr(L, "skv_score_landmarks" + sfx)(q.data_ptr(), *lm, D.data_ptr(), pm.data_ptr(), ps.data_ptr(), blocks, G,
                                                                  n, ALPHA, st)
                _lib.check(rc, "scan " + dt)

            def window(dt):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.passes):
                    for t, s, idx in rings[dt]:
                        launch(dt, t, s, idx)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e3 / (a.passes * count)

            for dt in rings:                                   # warm-up: code objects, clocks
                window(dt)
            us = {dt: [] for dt in rings}
            for _ in range(a.rounds):
                for dt in rings:
                    us[dt].append(window(dt))
            med = {dt: statistics.median(v) for dt, v in us.items()}
            spread = (max(us["bf16"]) - min(us["bf16"])) / med["bf16"]
            for dt in rings:
                nbytes = scan_bytes(blocks, n, dt != "bf16")
                lines.append(f"{form:<5} blocks {blocks:3d} (bs {blocks // 8:2d}) {dt:<8} median {med[dt]:8.2f} us  min {min(us[dt]):8.2f} us  "
                             f"{nbytes / 1e6:7.1f} MB  {nbytes / med[dt] * 1e-3:7.1f} GB/s algorithmic  ({count} tables in the ring)")
            lines.append(f"{form:<5} blocks {blocks:3d} fp8 : bf16 time {med['fp8_e4m3'] / med['bf16']:.3f}   spread of the bf16 rounds "
                         f"{100 * spread:.1f} %")
            del rings
            torch.cuda.empty_cache()
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
