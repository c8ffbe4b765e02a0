// Weight-only MXFP4 GEMV for the decode step's dense projections (one token): the kernels of skv_gemv.hip with the weights as
// OCP MX e2m1 nibbles and one e8m0 scale byte per 32 consecutive elements of a row,
//     W[n][k] = 2^(scale[n][k / 32] - 127) * e2m1(nibble[n][k]),
//     W4 [N][K / 2] bytes row-major, element 2i in the low nibble of byte i, element 2i + 1 in the high nibble;
//     scale [N][K / 32] bytes row-major;  x / bias / y bf16.
// Contract per output row: t = sum_k f32(2^s(n, k / 32) * e2m1(n, k)) * f32(x[k]) - the block scale is applied to the WEIGHT
// (exact: 2 significant bits times a power of two; it is what v_cvt_scalef32_pk_f32_fp4 returns), f32 accumulation in
// explicit FMAs, no multiply after the reduction - and t then takes exactly the epilogue of the bf16 kernel (plain, bias,
// SiLU pair, QKV, range keys).  Stated for scale bytes 27..227 (what quantize_mxfp4_rows emits).
//
// K % 32 == 0, K >= 1024 (a partial last 2048-element step is handled after the main loop; the NORM variant needs K == 4096).
// Same structure as skv_gemv_fp8_kernel: a wave owns R weight rows; each wave-instruction reads 1 KiB of a row (64 lanes x
// 16 B, coalesced, non-temporal), R x 4 row segments are in flight per wave before the first use.  A 16-byte load holds 32
// weights = exactly one MX block: a k-step is 2048 elements, a lane owns elements 32 lane .. 32 lane + 31 of it, reads them
// from x as four 16-byte vectors and has ONE scale byte per load; the 64 scale bytes of a row and k-step are contiguous (one
// coalesced byte load per lane).  The f32 scale operand is byte << 23, built once per load.  Per 16 B of weights:
// 16 v_cvt_scalef32_pk_f32_fp4 + 16 packed FMAs.
//
// This file holds the MXFP4 weight stream (prefetch, main loop, K tail) and the MXFP4 entries.  The frame around the stream is
// skv_gemv_frame.h, the norm prologue skv_norm_prologue_4096 (skv_kvproj.h): h and xn are bit-identical to skv_add_rmsnorm,
// only the pickup of xn from LDS differs (vectors 256 u + 4 lane .. + 3 for step u); near_pull_of is in skv_launch.h.
#include "../../include/shadowkv_hip.h"
#include "skv_gemv_frame.h"

// byte B of a 32-bit word as two f32 = scale * e2m1 (low nibble first: element order = nibble order)
template <int B>
__device__ __forceinline__ f32x2 e2m1_pair(uint32_t w, float scale) {
    return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, B);
}
// the f32 2^(byte - 127) of an e8m0 scale byte (bytes 1..254; the contract is 27..227)
__device__ __forceinline__ float e8m0_f32(uint32_t byte) { return __uint_as_float(byte << 23); }

// the 32 elements of one lane and one k-step: 4 weight words (8 nibbles each) against 16 bf16 pairs
template <int R>
__device__ __forceinline__ void mxfp4_fma32(f32x2 (&acc)[R][4], const u32x4 (&w)[R], const uint8_t (&sb)[R], const f32x2 (&xx)[16]) {
    float s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = e8m0_f32(sb[r]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            acc[r][j] = __builtin_elementwise_fma(e2m1_pair<0>(w[r][j], s[r]), xx[4 * j], acc[r][j]);
            acc[r][j] = __builtin_elementwise_fma(e2m1_pair<1>(w[r][j], s[r]), xx[4 * j + 1], acc[r][j]);
            acc[r][j] = __builtin_elementwise_fma(e2m1_pair<2>(w[r][j], s[r]), xx[4 * j + 2], acc[r][j]);
            acc[r][j] = __builtin_elementwise_fma(e2m1_pair<3>(w[r][j], s[r]), xx[4 * j + 3], acc[r][j]);
        }
    }
}
__device__ __forceinline__ void bf16x32_to_f32(f32x2 (&xx)[16], const u32x4 (&v)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) xx[4 * q + j] = (f32x2){bf_lo(v[q][j]), bf_hi(v[q][j])};
}

// Template parameters as in skv_gemv_kernel (skv_gemv_frame.h).
template <int R, bool SILU_PAIR, bool NORM, bool QKV, bool RMAX = false, bool NEARP = false>
__global__ __launch_bounds__(256) void skv_gemv_mxfp4_kernel(const uint8_t* __restrict__ W, const uint8_t* __restrict__ scale,
                                                             const bf16_t* __restrict__ x, const bf16_t* __restrict__ bias,
                                                             bf16_t* __restrict__ y, int N, int K, int I /* SILU_PAIR: rows of one half */,
                                                             const bf16_t* __restrict__ residual, const bf16_t* __restrict__ w_norm,
                                                             bf16_t* __restrict__ h_out, float eps, QkvEpilogue qe,
                                                             uint16_t* __restrict__ range_max = nullptr, NearPull np = NearPull{}) {
    int bx = blockIdx.x;
    if (skv_gemv_near_pull_block<NEARP>(np, bx)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ksteps = NORM ? 2 : K / 2048;  // 64 lanes x 32 elements per step (NORM: K == 4096, static trip count)
    int rows[R];
    const int unit0 = (bx * 4 + wave) * (SILU_PAIR ? R / 2 : R);
    skv_gemv_wave_rows<R, SILU_PAIR, QKV>(rows, unit0, I, qe.glm);
    const int limit = SILU_PAIR ? I : N;      // units of the launch
    if (!NORM && unit0 >= limit) return;   // (NORM: every wave takes part in the block-wide prologue first)
    const uint8_t *wp[R], *sp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = skv_gemv_stream_row<R, SILU_PAIR>(rows, r, unit0, limit, I);
        wp[r] = W + (size_t)row * (K / 2) + 16 * lane;      // a k-step is 1 KiB of a row's nibbles
        sp[r] = scale + (size_t)row * (K / 32) + lane;      // and 64 scale bytes
    }
    const bf16_t* xp = x + 32 * lane;
    // NORM: both k-steps of the weights and scales do not depend on the norm prologue: they are in flight before it
    u32x4 wpre[NORM ? 2 : 1][NORM ? R : 1];
    uint8_t spre[NORM ? 2 : 1][NORM ? R : 1];
    if (NORM) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                wpre[u][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)u * 1024));
                spre[u][r] = sp[r][u * 64];
            }
    }
    f32x2 xn[NORM ? 2 : 1][16];
    if (NORM) {
        __shared__ u32x4 s_xn[512];
        __shared__ float s_ss[4];
        skv_norm_prologue_4096<false>(x, residual, w_norm, bx == 0 ? h_out : nullptr, K, eps, tid, s_xn, s_ss);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const u32x4 v[4] = {s_xn[u * 256 + 4 * lane], s_xn[u * 256 + 4 * lane + 1], s_xn[u * 256 + 4 * lane + 2],
                                s_xn[u * 256 + 4 * lane + 3]};
            bf16x32_to_f32(xn[u], v);
        }
        if (unit0 >= limit) return;
    }
    f32x2 acc[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[r][j] = (f32x2){0.f, 0.f};

    if constexpr (NORM) {
#pragma unroll
        for (int u = 0; u < 2; ++u) mxfp4_fma32<R>(acc, wpre[u], spre[u], xn[u]);
    } else {
        for (int ks = 0; ks < ksteps; ks += 4) {
            u32x4 wv[4][R], xv[4][4];
            uint8_t sv[4][R];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (ks + u < ksteps) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) xv[u][q] = *reinterpret_cast<const u32x4*>(xp + (size_t)(ks + u) * 2048 + 8 * q);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        wv[u][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)(ks + u) * 1024));
                        sv[u][r] = sp[r][(size_t)(ks + u) * 64];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (ks + u < ksteps) {
                    f32x2 xx[16];
                    bf16x32_to_f32(xx, xv[u]);
                    mxfp4_fma32<R>(acc, wv[u], sv[u], xx);
                }
            }
        }
        // K % 2048 != 0 (K = 1024: this step only; GLM-4: 13696 = 6 x 2048 + 1408): the last partial step, lanes below the
        // tail only - a lane's 32 elements are one whole block, so the tail is K % 2048 / 32 lanes
        const int tail_lanes = (K % 2048) / 32;
        if (lane < tail_lanes) {
            u32x4 xt[4], wt[R];
            uint8_t st[R];
#pragma unroll
            for (int q = 0; q < 4; ++q) xt[q] = *reinterpret_cast<const u32x4*>(xp + (size_t)ksteps * 2048 + 8 * q);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                wt[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)ksteps * 1024));
                st[r] = sp[r][(size_t)ksteps * 64];
            }
            f32x2 xx[16];
            bf16x32_to_f32(xx, xt);
            mxfp4_fma32<R>(acc, wt, st, xx);
        }
    }
    float tot[R];
#pragma unroll
    for (int r = 0; r < R; ++r) tot[r] = skv_gemv_row_total(acc[r]);   // (no multiply after the reduction: the scales are in the weights)
    skv_gemv_epilogue<R, SILU_PAIR, QKV, RMAX>(rows, tot, unit0, bx, tid, N, I, bias, y, qe, range_max, x);
}

// the MXFP4 format of the host entries (skv_gemv_frame.h)
struct GemvMxfp4 : GemvArgs {
    static constexpr int K_STEP = 32, K_MIN = 1024;
    static constexpr bool SCALED = true;
    static constexpr bool Q_ROWS_ALONE = false;
    static constexpr bool NEAR_ROLE_ARGS_FIRST = false;      // a near-pull entry checks the GEMV's own arguments first, then the role's
    static constexpr bool QKV_REFUSES_NO_HEADS = true;     // the QKV entry with no heads: SKV_ERR_ARG from the entry itself
    const uint8_t* W;
    const uint8_t* scale;
    GemvMxfp4(const GemvArgs& a, const void* w, const void* s) : GemvArgs(a), W((const uint8_t*)w), scale((const uint8_t*)s) {}
    template <int R, bool SILU, bool NORM, bool QKV, bool RMAX, bool NEARP>
    void launch(int grid, int I, uint16_t* range_max, const NearPull& near) const {
        hipLaunchKernelGGL((skv_gemv_mxfp4_kernel<R, SILU, NORM, QKV, RMAX, NEARP>), dim3(grid), dim3(256), 0, st, W, scale, x, bias, y, N, K, I,
                           residual, w_norm, h_out, eps, qe, range_max, near);
    }
};

extern "C" int skv_gemv_mxfp4(const void* W4, const void* scale_e8m0, const void* x, const void* bias, void* y, int N, int K,
        int fuse_silu_mul, skv_stream_t stream) {
    return skv_gemv_entry<GemvMxfp4>(W4, scale_e8m0, x, bias, y, N, K, fuse_silu_mul, stream);
}

extern "C" int skv_norm_gemv_mxfp4(const void* W4, const void* scale_e8m0, const void* x, const void* residual, const void* norm_weight,
        float eps, void* h_out, const void* bias, void* y, int N, int K, int fuse_silu_mul, skv_stream_t stream) {
    return skv_norm_gemv_entry<GemvMxfp4>(W4, scale_e8m0, x, residual, norm_weight, eps, h_out, bias, y, N, K, fuse_silu_mul, stream);
}

extern "C" int skv_norm_gemv_rangemax_mxfp4(const void* W4, const void* scale_e8m0, const void* x, const void* residual,
        const void* norm_weight, float eps, void* h_out, const void* bias, void* y, int N, int K, void* range_max, skv_stream_t stream) {
    return skv_norm_gemv_rangemax_entry<GemvMxfp4>(W4, scale_e8m0, x, residual, norm_weight, eps, h_out, bias, y, N, K, range_max, stream);
}

extern "C" int skv_qkv_gemv_rope_update_mxfp4(const void* Wqkv4, const void* scale_e8m0, const void* x, const void* residual,
        const void* norm_weight, float eps, void* h_out, const void* bias, const void* cos_sin, const int64_t* pos, const int64_t* row_idx,
        const void* q_override, void* q_out, void* k_cache, void* v_cache, int K, int q_heads, int kv_heads, int head_dim,
        long long cos_sin_stride, int cos_sin_rows, long long cache_stride_h, int cache_rows, int rope_mode, skv_stream_t stream) {
    return skv_qkv_gemv_rope_update_entry<GemvMxfp4>(Wqkv4, scale_e8m0, x, residual, norm_weight, eps, h_out, bias, cos_sin, pos, row_idx,
                                                    q_override, q_out, k_cache, v_cache, K, q_heads, kv_heads, head_dim, cos_sin_stride,
                                                    cos_sin_rows, cache_stride_h, cache_rows, rope_mode, stream);
}

extern "C" int skv_norm_gemv_near_pull_mxfp4(const void* W4, const void* scale_e8m0, const void* x, const void* residual,
        const void* norm_weight, float eps, void* h_out, void* y, int N, int K, void* early_state, int blocks, int groups, int n_landmarks,
        int n_chunks, int early_max, const void* v_host, long long host_block_stride, int pull_parts, int active_lists, skv_stream_t stream) {
    return skv_norm_gemv_near_pull_entry<GemvMxfp4>(W4, scale_e8m0, x, residual, norm_weight, eps, h_out, y, N, K, early_state, blocks, groups,
                                                   n_landmarks, n_chunks, early_max, v_host, host_block_stride, pull_parts, active_lists,
                                                   stream);
}

extern "C" int skv_gemv_near_pull_mxfp4(const void* W4, const void* scale_e8m0, const void* x, const void* bias, void* y, int N, int K,
        void* early_state, int blocks, int groups, int n_landmarks, int n_chunks, int early_max, const void* v_host,
        long long host_block_stride, int pull_parts, int list, skv_stream_t stream) {
    return skv_gemv_near_pull_entry<GemvMxfp4>(W4, scale_e8m0, x, bias, y, N, K, early_state, blocks, groups, n_landmarks, n_chunks, early_max,
                                              v_host, host_block_stride, pull_parts, list, stream);
}
