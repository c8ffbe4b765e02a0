// The frame the small-M projection kernels share: skv_rows_gemm_kernel / skv_rows_gemm2_kernel (skv_rows_gemm.hip, bf16
// weights) and their FP8 siblings (skv_rows_gemm_fp8.hip, e4m3 weights + a row scale) differ only in how a wave streams and
// multiplies its K slice.  Everything around that stream is stated here once: which weight row and which token row a lane
// loads, a wave's K slice, the hand-off of the partial tiles to LDS, the wave-ordered reduction, the epilogue, and on the
// host the branch tree that picks a kernel instance.
//
// Lane layout of v_mfma_f32_16x16x32_bf16, both operands: lane (a = lane & 15, g = lane >> 4) holds row / token a and the
// g-th quarter of the k-step; of D it holds D[rows 4 g .. 4 g + 3][token a].
// Template parameters: SILU_PAIR: W = [gate; up] (2 I rows), a tile is 8 gate rows (a < 8) + the matching 8 up rows and
// y[m][i] = bf16(silu(gate_i)) * up_i; MT token tiles of 16; RT tiles of 16 weight rows per wave (first generation: 1);
// NWV waves per workgroup, K split NWV ways.
#pragma once
#include "skv_common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ int skv_rows_a(int lane) { return lane & 15; }
__device__ __forceinline__ int skv_rows_g(int lane) { return lane >> 4; }

// the weight row lane column a streams for tile `tile`; a row past a ragged last tile is clamped: computed and discarded.
// Returned as the size_t the row offset is computed in: with an int return hipcc takes the clamp as a 32-bit min ahead of the
// k-loops and the plain second-generation instances hold 2 to 4 more VGPRs (profiles/rows_frame_refactor.txt section 2).
template <bool SILU_PAIR>
__device__ __forceinline__ size_t skv_rows_weight_row(int tile, int a, int N, int I) {
    if (SILU_PAIR) {
        int idx = tile * 8 + (a & 7);
        if (idx >= I) idx = I - 1;
        return (size_t)(a < 8 ? idx : I + idx);
    }
    int row = tile * 16 + a;
    if (row >= N) row = N - 1;
    return (size_t)row;
}
// the token row of lane column a in token tile t; columns >= M compute a duplicate that is never stored
__device__ __forceinline__ int skv_rows_token(int t, int a, int M) { return min(16 * t + a, M - 1); }

// wave `wave` of NWV runs the k-steps [s0, s1) of S
template <int NWV>
__device__ __forceinline__ void skv_rows_k_slice(int S, int wave, int& s0, int& s1) {
    const int per = (S + NWV - 1) / NWV;
    s0 = wave * per;
    s1 = min(S, s0 + per);
}

// acc[r][t]: the wave's partial tile of row tile r and token tile t -> LDS -> the workgroup's outputs.  An output unit o is a
// row, or a (gate, up) pair, of one token: the NWV partial sums in wave order, the row scale (SCALED: one f32 multiply after
// the reduction), then bias / SiLU * mul with one bf16 rounding per tensor.  ONE_PASS (the first generation): the workgroup's
// threads cover every unit of M <= 32 token rows at once, no loop.  The second generation loops even where one pass would
// do (2/1x8): without the loop those launches measured slower (profiles/rows_frame_refactor.txt section 4, job B).
template <bool SILU_PAIR, bool SCALED, bool ONE_PASS, int NWV, int MT, int RT>
__device__ __forceinline__ void skv_rows_epilogue(const f32x4 (&acc)[RT][MT], int tid, int a, int g, const float* __restrict__ scale,
                                                  const bf16_t* __restrict__ bias, bf16_t* __restrict__ Y, int N, int M, int I) {
    static_assert(!ONE_PASS || RT * 16 * 32 <= NWV * 64, "one pass: a thread per output unit of 32 token rows");
    __shared__ float s_red[NWV][MT][RT][16][17];
    const int wave = tid >> 6;
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) s_red[wave][t][r][4 * g + i][a] = acc[r][t][i];
    __syncthreads();
    constexpr int UNITS = SILU_PAIR ? 8 : 16;
    const auto output = [&](int o) {
        const int tok = o / (RT * UNITS), j = o % (RT * UNITS), r = j / UNITS, i = j % UNITS;
        const int n = (blockIdx.x * RT + r) * UNITS + i;
        if (SILU_PAIR) {
            if (n < I) {
                float gs = 0.f, us = 0.f;
#pragma unroll
                for (int w = 0; w < NWV; ++w) {
                    gs += s_red[w][tok >> 4][r][i][tok & 15];
                    us += s_red[w][tok >> 4][r][i + 8][tok & 15];
                }
                if constexpr (SCALED) {
                    gs = scale[n] * gs;
                    us = scale[I + n] * us;
                }
                const float gg = bfr(gs), uu = bfr(us);  // the projection outputs are bf16 tensors
                Y[(size_t)tok * I + n] = f2bf(bfr(gg / (1.0f + __expf(-gg))) * uu);
            }
        } else if (n < N) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < NWV; ++w) t += s_red[w][tok >> 4][r][i][tok & 15];
            if constexpr (SCALED) t *= scale[n];
            Y[(size_t)tok * N + n] = f2bf(bias ? bfr(t) + bf2f(bias[n]) : t);
        }
    };
    if constexpr (ONE_PASS) {
        if (tid < RT * UNITS * M) output(tid);
    } else {
        for (int o = tid; o < RT * UNITS * M; o += NWV * 64) output(o);
    }
}

// Host.  L is the format's launcher: it holds the launch's arguments; gen1<SILU_PAIR, PAIRX, MT>(grid, I) and
// gen2<SILU_PAIR, MT, RT, NWV>(grid, I) start its kernels with the k-steps in flight (U) the format chose for that shape.
template <bool SILU_PAIR, bool PAIRX, int MT, class L>
static void skv_rows_launch1(const L& l, int N, int I) {
    l.template gen1<SILU_PAIR, PAIRX, MT>(SILU_PAIR ? (I + 7) / 8 : (N + 15) / 16, I);
}
template <bool SILU_PAIR, int MT, int RT, int NWV, class L>
static void skv_rows_launch2(const L& l, int N, int I) {
    const int tiles = SILU_PAIR ? (I + 7) / 8 : (N + 15) / 16;
    l.template gen2<SILU_PAIR, MT, RT, NWV>((tiles + RT - 1) / RT, I);
}

// Kernel and shape per (token rows, projection), measured on MI355X with bf16 weights, HBM-cold (tools/time_rows_gemm.py, us;
// g1 = first-generation kernel, RTxNW = second generation with RT row tiles per wave and NW waves per workgroup):
//     rows   QKV 6144x4096        O 4096x4096        gate/up 28672x4096        down 4096x14336
//      8     g1 15.6 | 2x8 15.2   g1  9.3 | 1x8 10.1  g1 52.3 | 4x4 59.9        g1 29.4 | 1x8 32.0      -> g1 (paired operand)
//     16     g1 18.9 | 2x8 16.6   g1 10.6 | 1x8 11.8  g1 63.7 | 4x4 62.9        g1 33.5 | 1x8 36.7      -> g1, QKV 2x8
//     24     g1 25.1 | 2x8 19.4   g1 13.6 | 1x8 13.9  g1 85.6 | 4x4 59.9        g1 45.6 | 1x8 42.8      -> 2x8, g1, 4x4, 1x8
//     32     g1 28.6 | 2x8 20.7   g1 15.6 | 1x8 15.0  g1 96.5 | 4x4 62.3        g1 50.6 | 1x8 47.4
// (fewer, fatter workgroups lose where the projection has only 256 row tiles; the token operand's distinct cache lines,
// not the weight stream, set the pace of the first generation from 17 rows on.)
// For FP8 weights these thresholds are a STARTING POINT, NOT A RESULT: an entry changes for that format only with numbers
// from tools/time_rows_gemm.py --fp8 (profiles/fp8_rows_timing.txt).
template <bool SILU_PAIR, class L>
static void skv_rows_pick(const L& l, int M, int N, int K, int I) {
    const bool mid = N >= 6144 && N < 16384;
    if (M <= 8) return skv_rows_launch1<SILU_PAIR, true, 1>(l, N, I);
    if (M <= 16) {
        if (mid) return skv_rows_launch2<SILU_PAIR, 1, 2, 8>(l, N, I);
        return skv_rows_launch1<SILU_PAIR, false, 1>(l, N, I);
    }
    if (N >= 16384) return skv_rows_launch2<SILU_PAIR, 2, 4, 4>(l, N, I);
    if (mid) return skv_rows_launch2<SILU_PAIR, 2, 2, 8>(l, N, I);
    if (K >= 8192) return skv_rows_launch2<SILU_PAIR, 2, 1, 8>(l, N, I);
    return skv_rows_launch1<SILU_PAIR, false, 2>(l, N, I);
}
// The format checks its own arguments (pointers, M, K, the SiLU form) before this; a SiLU launch has no bias.
template <class L>
static int skv_rows_dispatch(const L& l, int M, int N, int K, bool fuse_silu_mul) {
    if (fuse_silu_mul) skv_rows_pick<true>(l, M, N, K, N / 2);
    else skv_rows_pick<false>(l, M, N, K, 0);
    return hipGetLastError() == hipSuccess ? SKV_OK : SKV_ERR_LAUNCH;
}
