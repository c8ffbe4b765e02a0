// Weight-only FP8 sibling of skv_rows_gemm.hip: the dense projections of a decode step with 2..32 token rows, the weights as OCP
// e4m3fn bytes with one f32 scale per output row,
//     Y[m][n] = scale[n] * sum_k e4m3(W8[n][k]) * X[m][k] (+ bias[n]),   W8 [N][K] bytes row-major, X [M][K], Y [M][N] bf16, M <= 32
// and the gate/up variant (W8 = [gate; up], 2I rows): Y[m][i] = bf16(silu(t_g)) * t_u, each row with its own scale.
// Contract per output: f32 accumulation, the split-K partials summed in wave order, then ONE f32 multiply
// by scale[n]; t then takes exactly the epilogue of skv_linear_rows_bf16.  Activations stay bf16: e4m3 -> bf16 is exact, the
// multiply is v_mfma_f32_16x16x32_bf16.
//
// Structure, tile shapes and the (SILU_PAIR, MT, RT, NWV) family are those of skv_rows_gemm.hip; only the weight operand changes.
// A 16-byte load now holds 16 weights, so a k-step is 64 elements and feeds TWO MFMAs:
//     A operand (weights): lane (a = lane & 15, g = lane >> 4) loads 16 B = W8[row a][64 s + 16 g .. +16]  (nontemporal);
//                          bytes 0..7 -> 8 bf16 for the first MFMA, bytes 8..15 for the second (4 + 4 v_cvt_scalef32_pk_bf16_fp8,
//                          scale 1.0: two bytes -> one packed bf16 pair, straight into the operand registers)
//     B operand (tokens) : lane (a, g) reads the 32 bytes X[token min(a, M-1)][64 s + 16 g .. +16] as two 16-byte vectors, the
//                          first for the first MFMA, the second for the second (the k order inside an MFMA is free as long as
//                          both operands agree: lane group g owns k = 16 g .. 16 g + 15 of the step, split 8 | 8)
//     D                  : lane holds D[rows 4 g .. 4 g + 3][token a]
// Per 16 B of weights: 8 conversions and 2 * MT MFMAs.
#include "../../include/shadowkv_hip.h"
#include "skv_common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#ifndef RG8_WAVES
#define RG8_WAVES 8
#endif
#ifndef RG8_U
#define RG8_U 8
#endif
// RG8_WAVES: waves per 16-row tile (K split);  RG8_U: k-steps (16-B weight loads) in flight per wave of the first generation

// eight e4m3 bytes (two words) -> the 8 bf16 of one MFMA operand, element order = byte order.  gfx950 decodes OCP e4m3fn.
__device__ __forceinline__ bf16x8 e4m3x8_to_bf16(uint32_t w0, uint32_t w1) {
    u32x4 r;
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true));
    return __builtin_bit_cast(bf16x8, r);
}
__device__ __forceinline__ f32x4 mfma_bf16(bf16x8 w, const u32x4& x, f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, __builtin_bit_cast(bf16x8, x), acc, 0, 0, 0);
}

// PAIRX (M <= 8): token columns 8..15 of the MFMA are never stored, so their lanes (a >= 8) load the SECOND 16-byte vector of
// token a - 8 (same k-step) and hand it over with one DPP row rotate: one token-operand load serves both MFMAs of a k-step.
// MT = 2 (17 <= M <= 32): two token tiles per weight load, as in skv_rows_gemm_kernel.
template <bool SILU_PAIR, bool PAIRX, int MT, int U>
__global__ __launch_bounds__(RG8_WAVES * 64) void skv_rows_gemm_fp8_kernel(const uint8_t* __restrict__ W, const float* __restrict__ scale,
                                                                           const bf16_t* __restrict__ X,
                                                                           const bf16_t* __restrict__ bias, bf16_t* __restrict__ Y,
                                                                           int N, int K, int M, int I /* SILU_PAIR: rows of one half */) {
    static_assert(!(PAIRX && MT > 1), "the paired token operand serves one tile of <= 8 tokens");
    __shared__ float s_red[RG8_WAVES][MT][16][17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = lane & 15, g = lane >> 4;
    int row;
    if (SILU_PAIR) {  // tile = 8 gate rows (a < 8) + the matching 8 up rows
        int idx = blockIdx.x * 8 + (a & 7);
        if (idx >= I) idx = I - 1;  // clamp: computed and discarded
        row = a < 8 ? idx : I + idx;
    } else {
        row = blockIdx.x * 16 + a;
        if (row >= N) row = N - 1;
    }
    const uint8_t* wp = W + (size_t)row * K + 16 * g;
    const int tokl = PAIRX ? (a & 7) : a;
    const bf16_t* xp[MT];                                               // batches (PAIRX: lanes a >= 8 at the second vector)
    const bf16_t* xs[MT];                                               // single steps: every lane both vectors of its token
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int tok = min(16 * t + tokl, M - 1);                       // columns >= M: a duplicate, never stored
        xs[t] = X + (size_t)tok * K + 16 * g;
        xp[t] = xs[t] + (PAIRX ? (a >> 3) * 8 : 0);
    }
    const int S = K / 64, per = (S + RG8_WAVES - 1) / RG8_WAVES;
    const int s0 = wave * per, s1 = min(S, s0 + per);
    f32x4 acc0[MT], acc1[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        acc0[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        acc1[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    int s = s0;
    for (; s + U <= s1; s += U) {
        u32x4 wv[U], xv[MT][U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            wv[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + (size_t)(s + u) * 64));
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                xv[t][u][0] = *reinterpret_cast<const u32x4*>(xp[t] + (size_t)(s + u) * 64);
                if (!PAIRX) xv[t][u][1] = *reinterpret_cast<const u32x4*>(xp[t] + (size_t)(s + u) * 64 + 8);
            }
        }
        // every load of the batch is issued before the first conversion: the fence of skv_rows_gemm2_kernel keeps the compiler from
        // sinking a load to its use, the scheduling barrier keeps the machine scheduler from weaving loads into the conversions
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (PAIRX) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    xv[0][u][1][j] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)xv[0][u][0][j], 0x128 /*row_ror:8*/, 0xf, 0xf, false);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bf16x8 w0 = e4m3x8_to_bf16(wv[u][0], wv[u][1]), w1 = e4m3x8_to_bf16(wv[u][2], wv[u][3]);
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                acc0[t] = mfma_bf16(w0, xv[t][u][0], acc0[t]);
                acc1[t] = mfma_bf16(w1, xv[t][u][1], acc1[t]);
            }
        }
    }
    for (; s < s1; ++s) {
        const u32x4 wv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + (size_t)s * 64));
        u32x4 xv[MT][2];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            xv[t][0] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)s * 64);
            xv[t][1] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)s * 64 + 8);
        }
        const bf16x8 w0 = e4m3x8_to_bf16(wv[0], wv[1]), w1 = e4m3x8_to_bf16(wv[2], wv[3]);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            acc0[t] = mfma_bf16(w0, xv[t][0], acc0[t]);
            acc1[t] = mfma_bf16(w1, xv[t][1], acc1[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_red[wave][t][4 * g + r][a] = acc0[t][r] + acc1[t][r];
    __syncthreads();
    if (SILU_PAIR) {
        if (tid < 8 * M) {
            const int tok = tid >> 3, i = tid & 7, idx = blockIdx.x * 8 + i;
            if (idx < I) {
                float gs = 0.f, us = 0.f;
#pragma unroll
                for (int w = 0; w < RG8_WAVES; ++w) {
                    gs += s_red[w][tok >> 4][i][tok & 15];
                    us += s_red[w][tok >> 4][i + 8][tok & 15];
                }
                const float gg = bfr(scale[idx] * gs), uu = bfr(scale[I + idx] * us);  // the projection outputs are bf16 tensors
                Y[(size_t)tok * I + idx] = f2bf(bfr(gg / (1.0f + __expf(-gg))) * uu);
            }
        }
    } else if (tid < 16 * M) {
        const int tok = tid >> 4, r = tid & 15, n = blockIdx.x * 16 + r;
        if (n < N) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < RG8_WAVES; ++w) t += s_red[w][tok >> 4][r][tok & 15];
            t *= scale[n];                       // the row's scale: one f32 multiply after the reduction
            Y[(size_t)tok * N + n] = f2bf(bias ? bfr(t) + bf2f(bias[n]) : t);
        }
    }
}

// Second generation (skv_rows_gemm2_kernel): a wave walks RT tiles of 16 weight rows over its K slice, so one token-operand load
// (32 bytes here) per k-step serves 2 * RT (x MT) MFMAs.  U k-steps in flight: RT * U weight loads of 1 KB per wave.
template <bool SILU_PAIR, int MT, int RT, int NWV, int U>
__global__ __launch_bounds__(NWV * 64) void skv_rows_gemm2_fp8_kernel(const uint8_t* __restrict__ W, const float* __restrict__ scale,
                                                                      const bf16_t* __restrict__ X, const bf16_t* __restrict__ bias,
                                                                      bf16_t* __restrict__ Y, int N, int K, int M,
                                                                      int I /* SILU_PAIR: rows of one half */) {
    __shared__ float s_red[NWV][MT][RT][16][17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = lane & 15, g = lane >> 4;
    const uint8_t* wp[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        int row;
        if (SILU_PAIR) {  // tile = 8 gate rows (a < 8) + the matching 8 up rows
            int idx = (blockIdx.x * RT + r) * 8 + (a & 7);
            if (idx >= I) idx = I - 1;  // clamp: computed and discarded
            row = a < 8 ? idx : I + idx;
        } else {
            row = (blockIdx.x * RT + r) * 16 + a;
            if (row >= N) row = N - 1;
        }
        wp[r] = W + (size_t)row * K + 16 * g;
    }
    const bf16_t* xs[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) xs[t] = X + (size_t)min(16 * t + a, M - 1) * K + 16 * g;   // columns >= M: a duplicate, never stored
    const int S = K / 64, per = (S + NWV - 1) / NWV;
    const int s0 = wave * per, s1 = min(S, s0 + per);
    f32x4 acc[RT][MT];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[r][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int s = s0;
    for (; s + U <= s1; s += U) {
        u32x4 wv[RT][U], xv[MT][U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int r = 0; r < RT; ++r)
                wv[r][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)(s + u) * 64));
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                xv[t][u][0] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)(s + u) * 64);
                xv[t][u][1] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)(s + u) * 64 + 8);
            }
        }
        // every load of the batch is issued before the first conversion (fence + scheduling barrier, as in the first generation)
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < RT; ++r) {
                    const bf16x8 w = e4m3x8_to_bf16(wv[r][u][2 * h], wv[r][u][2 * h + 1]);
#pragma unroll
                    for (int t = 0; t < MT; ++t) acc[r][t] = mfma_bf16(w, xv[t][u][h], acc[r][t]);
                }
    }
    for (; s < s1; ++s) {
        u32x4 xv[MT][2];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            xv[t][0] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)s * 64);
            xv[t][1] = *reinterpret_cast<const u32x4*>(xs[t] + (size_t)s * 64 + 8);
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const u32x4 wv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)s * 64));
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bf16x8 w = e4m3x8_to_bf16(wv[2 * h], wv[2 * h + 1]);
#pragma unroll
                for (int t = 0; t < MT; ++t) acc[r][t] = mfma_bf16(w, xv[t][h], acc[r][t]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) s_red[wave][t][r][4 * g + i][a] = acc[r][t][i];
    __syncthreads();
    if (SILU_PAIR) {
        for (int o = tid; o < RT * 8 * M; o += NWV * 64) {
            const int tok = o / (RT * 8), j = o % (RT * 8), r = j >> 3, i = j & 7, idx = (blockIdx.x * RT + r) * 8 + i;
            if (idx < I) {
                float gs = 0.f, us = 0.f;
#pragma unroll
                for (int w = 0; w < NWV; ++w) {
                    gs += s_red[w][tok >> 4][r][i][tok & 15];
                    us += s_red[w][tok >> 4][r][i + 8][tok & 15];
                }
                const float gg = bfr(scale[idx] * gs), uu = bfr(scale[I + idx] * us);  // the projection outputs are bf16 tensors
                Y[(size_t)tok * I + idx] = f2bf(bfr(gg / (1.0f + __expf(-gg))) * uu);
            }
        }
    } else {
        for (int o = tid; o < RT * 16 * M; o += NWV * 64) {
            const int tok = o / (RT * 16), j = o % (RT * 16), r = j >> 4, rr = j & 15, n = (blockIdx.x * RT + r) * 16 + rr;
            if (n < N) {
                float t = 0.f;
#pragma unroll
                for (int w = 0; w < NWV; ++w) t += s_red[w][tok >> 4][r][rr][tok & 15];
                t *= scale[n];                   // the row's scale: one f32 multiply after the reduction
                Y[(size_t)tok * N + n] = f2bf(bias ? bfr(t) + bf2f(bias[n]) : t);
            }
        }
    }
}

template <bool SILU_PAIR, int MT, int RT, int NWV, int U = 4>
static void launch_rows2_fp8(const void* W, const void* scale, const void* X, const void* bias, void* Y, int M, int N, int K, int I,
                             hipStream_t st) {
    const int tiles = SILU_PAIR ? (I + 7) / 8 : (N + 15) / 16;
    hipLaunchKernelGGL((skv_rows_gemm2_fp8_kernel<SILU_PAIR, MT, RT, NWV, U>), dim3((tiles + RT - 1) / RT), dim3(NWV * 64), 0, st,
                       (const uint8_t*)W, (const float*)scale, (const bf16_t*)X, (const bf16_t*)bias, (bf16_t*)Y, N, K, M, I);
}

template <bool SILU_PAIR, bool PAIRX, int MT, int U = RG8_U>
static void launch_rows1_fp8(const void* W, const void* scale, const void* X, const void* bias, void* Y, int M, int N, int K, int I,
                             hipStream_t st) {
    hipLaunchKernelGGL((skv_rows_gemm_fp8_kernel<SILU_PAIR, PAIRX, MT, U>), dim3(SILU_PAIR ? (I + 7) / 8 : (N + 15) / 16),
                       dim3(RG8_WAVES * 64), 0, st, (const uint8_t*)W, (const float*)scale, (const bf16_t*)X, (const bf16_t*)bias,
                       (bf16_t*)Y, N, K, M, I);
}

// Kernel and shape per (token rows, projection).  The thresholds are those of launch_rows (skv_rows_gemm.hip), which were
// measured for bf16 WEIGHTS: for this kernel they are a STARTING POINT, NOT A RESULT - nothing here has been timed with FP8
// weights yet.  An entry changes only with numbers from tools/time_rows_gemm.py --fp8 (profiles/fp8_rows_timing.txt).
//     rows <= 8            -> first generation, paired token operand
//     rows <= 16           -> first generation; 6144 <= N < 16384: 2x8
//     rows <= 32           -> N >= 16384: 4x4; 6144 <= N < 16384: 2x8; K >= 8192: 1x8; else first generation, two token tiles
// k-steps in flight per wave (weight loads of 16 B per lane; every k-step adds 2 * MT token loads): 8 with the paired token
// operand, 4 in the other first-generation shapes (two workgroups fit a CU's registers; 8 steps leave room for one), 4 in the
// second generation, 2 in its 4x4 shape (16 loads per step pair).  Like the thresholds: chosen from the register counts, not timed.
template <bool SILU_PAIR>
static void launch_rows_fp8(const void* W, const void* scale, const void* X, const void* bias, void* Y, int M, int N, int K, int I,
                            hipStream_t st) {
    const bool mid = N >= 6144 && N < 16384;
    if (M <= 8) return launch_rows1_fp8<SILU_PAIR, true, 1>(W, scale, X, bias, Y, M, N, K, I, st);
    if (M <= 16) {
        if (mid) return launch_rows2_fp8<SILU_PAIR, 1, 2, 8>(W, scale, X, bias, Y, M, N, K, I, st);
        return launch_rows1_fp8<SILU_PAIR, false, 1, 4>(W, scale, X, bias, Y, M, N, K, I, st);
    }
    if (N >= 16384) return launch_rows2_fp8<SILU_PAIR, 2, 4, 4, 2>(W, scale, X, bias, Y, M, N, K, I, st);
    if (mid) return launch_rows2_fp8<SILU_PAIR, 2, 2, 8>(W, scale, X, bias, Y, M, N, K, I, st);
    if (K >= 8192) return launch_rows2_fp8<SILU_PAIR, 2, 1, 8>(W, scale, X, bias, Y, M, N, K, I, st);
    return launch_rows1_fp8<SILU_PAIR, false, 2, 4>(W, scale, X, bias, Y, M, N, K, I, st);
}

extern "C" int skv_linear_rows_fp8(const void* W8, const void* scale, const void* X, const void* bias, void* Y, int M, int N, int K,
                                   int fuse_silu_mul, skv_stream_t stream) {
    // every argument check on the host, before any HIP call
    if (!W8 || !scale || !X || !Y || M < 1 || N < 1) return SKV_ERR_ARG;
    if (fuse_silu_mul && (N % 2 || bias)) return SKV_ERR_ARG;
    if (M > 32 || K % 64 || K < 64) return SKV_ERR_UNSUPPORTED;
    if (fuse_silu_mul) launch_rows_fp8<true>(W8, scale, X, nullptr, Y, M, N, K, N / 2, (hipStream_t)stream);
    else launch_rows_fp8<false>(W8, scale, X, bias, Y, M, N, K, 0, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? SKV_OK : SKV_ERR_LAUNCH;
}
