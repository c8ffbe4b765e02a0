// Weight-only FP8 GEMV for the decode step's dense projections (one token): the kernels of skv_gemv.hip with the weights as
// OCP e4m3fn bytes and one f32 scale per output row,
//     W[n][k] = scale[n] * e4m3(byte[n][k]),   byte [N][K] row-major (K contiguous), x / bias / y bf16.
// Contract per output row: t = scale[n] * sum_k f32(e4m3(byte[n][k])) * f32(x[k]) - f32 accumulation, ONE f32 multiply after
// the reduction - and t then takes exactly the epilogue of the bf16 kernel (plain, bias, SiLU pair, QKV, range keys).
//
// K % 16 == 0, K >= 1024 (a partial last 1024-element step is handled after the main loop; the NORM variant needs K == 4096).
// Same structure as skv_gemv_kernel: a wave owns R weight rows; each wave-instruction reads 1 KiB of a row (64 lanes x 16 B,
// coalesced, non-temporal), R x 4 row segments are in flight per wave before the first use.  A 16-byte load now holds 16
// weights: a k-step is 1024 elements, a lane owns elements 16 lane .. 16 lane + 15 of it and reads them from x as two 16-byte
// vectors.  Per 16 B of weights: 8 v_cvt_pk_f32_fp8 (gfx950 decodes OCP e4m3fn, not MI300's fnuz) + 8 packed FMAs.
//
// This file holds the FP8 weight stream (prefetch, main loop, K tail, the row scale) and the FP8 entries.  The frame around
// the stream - near-pull role, row ownership, row total, epilogue, the launch branch tree - is skv_gemv_frame.h, shared with
// skv_gemv.hip; the norm prologue is skv_norm_prologue_4096 (skv_kvproj.h): h and xn are bit-identical to skv_add_rmsnorm, only
// the pickup of xn from LDS differs from the bf16 kernel's (vectors 128 u + 2 lane, 128 u + 2 lane + 1 for step u);
// near_pull_of is in skv_launch.h.
#include "../../include/shadowkv_hip.h"
#include "skv_gemv_frame.h"

// bytes 0, 1 / bytes 2, 3 of a 32-bit word as two f32 (element order = byte order)
__device__ __forceinline__ f32x2 e4m3_lo(uint32_t w) { return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false); }
__device__ __forceinline__ f32x2 e4m3_hi(uint32_t w) { return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true); }

// the 16 elements of one lane and one k-step: 4 weight words against 8 bf16 pairs
template <int R>
__device__ __forceinline__ void fp8_fma16(f32x2 (&acc)[R][4], const u32x4 (&w)[R], const f32x2 (&xx)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            acc[r][j] = __builtin_elementwise_fma(e4m3_lo(w[r][j]), xx[2 * j], acc[r][j]);
            acc[r][j] = __builtin_elementwise_fma(e4m3_hi(w[r][j]), xx[2 * j + 1], acc[r][j]);
        }
    }
}
__device__ __forceinline__ void bf16x16_to_f32(f32x2 (&xx)[8], const u32x4& a, const u32x4& b) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        xx[j] = (f32x2){bf_lo(a[j]), bf_hi(a[j])};
        xx[4 + j] = (f32x2){bf_lo(b[j]), bf_hi(b[j])};
    }
}

// Template parameters as in skv_gemv_kernel (skv_gemv_frame.h).
template <int R, bool SILU_PAIR, bool NORM, bool QKV, bool RMAX = false, bool NEARP = false>
__global__ __launch_bounds__(256) void skv_gemv_fp8_kernel(const uint8_t* __restrict__ W, const float* __restrict__ scale,
                                                           const bf16_t* __restrict__ x, const bf16_t* __restrict__ bias,
                                                           bf16_t* __restrict__ y, int N, int K, int I /* SILU_PAIR: rows of one half */,
                                                           const bf16_t* __restrict__ residual, const bf16_t* __restrict__ w_norm,
                                                           bf16_t* __restrict__ h_out, float eps, QkvEpilogue qe,
                                                           uint16_t* __restrict__ range_max = nullptr, NearPull np = NearPull{}) {
    int bx = blockIdx.x;
    if (skv_gemv_near_pull_block<NEARP>(np, bx)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ksteps = NORM ? 4 : K / 1024;  // 64 lanes x 16 elements per step (NORM: K == 4096, static trip count)
    int rows[R];
    const int unit0 = (bx * 4 + wave) * (SILU_PAIR ? R / 2 : R);
    skv_gemv_wave_rows<R, SILU_PAIR, QKV>(rows, unit0, I, qe.glm);
    const int limit = SILU_PAIR ? I : N;      // units of the launch
    if (!NORM && unit0 >= limit) return;   // (NORM: every wave takes part in the block-wide prologue first)
    const uint8_t* wp[R];
    float sc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = skv_gemv_stream_row<R, SILU_PAIR>(rows, r, unit0, limit, I);
        wp[r] = W + (size_t)row * K + 16 * lane;
        sc[r] = scale[row];
    }
    const bf16_t* xp = x + 16 * lane;
    // NORM: all four k-steps of the weights do not depend on the norm prologue: they are in flight before it
    u32x4 wpre[NORM ? R : 1][4];
    if (NORM) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < R; ++r)
                wpre[r][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)u * 1024));
    }
    f32x2 xn[NORM ? 4 : 1][8];
    if (NORM) {
        __shared__ u32x4 s_xn[512];
        __shared__ float s_ss[4];
        skv_norm_prologue_4096<false>(x, residual, w_norm, bx == 0 ? h_out : nullptr, K, eps, tid, s_xn, s_ss);
#pragma unroll
        for (int u = 0; u < 4; ++u) bf16x16_to_f32(xn[u], s_xn[u * 128 + 2 * lane], s_xn[u * 128 + 2 * lane + 1]);
        if (unit0 >= limit) return;
    }
    f32x2 acc[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[r][j] = (f32x2){0.f, 0.f};

    if constexpr (NORM) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            u32x4 w[R];
#pragma unroll
            for (int r = 0; r < R; ++r) w[r] = wpre[r][u];
            fp8_fma16<R>(acc, w, xn[u]);
        }
    } else {
        for (int ks = 0; ks < ksteps; ks += 4) {
            u32x4 wv[4][R], xv[4][2];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (ks + u < ksteps) {
                    xv[u][0] = *reinterpret_cast<const u32x4*>(xp + (size_t)(ks + u) * 1024);
                    xv[u][1] = *reinterpret_cast<const u32x4*>(xp + (size_t)(ks + u) * 1024 + 8);
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        wv[u][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)(ks + u) * 1024));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (ks + u < ksteps) {
                    f32x2 xx[8];
                    bf16x16_to_f32(xx, xv[u][0], xv[u][1]);
                    fp8_fma16<R>(acc, wv[u], xx);
                }
            }
        }
        // K % 1024 != 0 (GLM-4: 13696 = 13 x 1024 + 384): the last partial step, lanes below the tail only
        const int tail_lanes = (K % 1024) / 16;
        if (lane < tail_lanes) {
            f32x2 xx[8];
            bf16x16_to_f32(xx, *reinterpret_cast<const u32x4*>(xp + (size_t)ksteps * 1024),
                           *reinterpret_cast<const u32x4*>(xp + (size_t)ksteps * 1024 + 8));
            u32x4 wt[R];
#pragma unroll
            for (int r = 0; r < R; ++r) wt[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)ksteps * 1024));
            fp8_fma16<R>(acc, wt, xx);
        }
    }
    float tot[R];
#pragma unroll
    for (int r = 0; r < R; ++r) tot[r] = sc[r] * skv_gemv_row_total(acc[r]);   // the row's scale: one f32 multiply after the reduction
    skv_gemv_epilogue<R, SILU_PAIR, QKV, RMAX>(rows, tot, unit0, bx, tid, N, I, bias, y, qe, range_max, x);
}

// the FP8 format of the host entries (skv_gemv_frame.h)
struct GemvFp8 : GemvArgs {
    static constexpr int K_STEP = 16, K_MIN = 1024;
    static constexpr bool SCALED = true;
    static constexpr bool Q_ROWS_ALONE = false;
    static constexpr bool NEAR_ROLE_ARGS_FIRST = false;      // a near-pull entry checks the GEMV's own arguments first, then the role's
    static constexpr bool QKV_REFUSES_NO_HEADS = true;     // the QKV entry with no heads: SKV_ERR_ARG from the entry itself
    const uint8_t* W;
    const float* scale;
    GemvFp8(const GemvArgs& a, const void* w, const void* s) : GemvArgs(a), W((const uint8_t*)w), scale((const float*)s) {}
    template <int R, bool SILU, bool NORM, bool QKV, bool RMAX, bool NEARP>
    void launch(int grid, int I, uint16_t* range_max, const NearPull& near) const {
        hipLaunchKernelGGL((skv_gemv_fp8_kernel<R, SILU, NORM, QKV, RMAX, NEARP>), dim3(grid), dim3(256), 0, st, W, scale, x, bias, y, N, K, I,
                           residual, w_norm, h_out, eps, qe, range_max, near);
    }
};

extern "C" int skv_gemv_fp8(const void* W8, const void* scale, const void* x, const void* bias, void* y, int N, int K,
        int fuse_silu_mul, skv_stream_t stream) {
    return skv_gemv_entry<GemvFp8>(W8, scale, x, bias, y, N, K, fuse_silu_mul, stream);
}

extern "C" int skv_norm_gemv_fp8(const void* W8, const void* scale, const void* x, const void* residual, const void* norm_weight,
        float eps, void* h_out, const void* bias, void* y, int N, int K, int fuse_silu_mul, skv_stream_t stream) {
    return skv_norm_gemv_entry<GemvFp8>(W8, scale, x, residual, norm_weight, eps, h_out, bias, y, N, K, fuse_silu_mul, stream);
}

extern "C" int skv_norm_gemv_rangemax_fp8(const void* W8, const void* scale, const void* x, const void* residual,
        const void* norm_weight, float eps, void* h_out, const void* bias, void* y, int N, int K, void* range_max, skv_stream_t stream) {
    return skv_norm_gemv_rangemax_entry<GemvFp8>(W8, scale, x, residual, norm_weight, eps, h_out, bias, y, N, K, range_max, stream);
}

extern "C" int skv_qkv_gemv_rope_update_fp8(const void* Wqkv8, const void* scale, const void* x, const void* residual,
        const void* norm_weight, float eps, void* h_out, const void* bias, const void* cos_sin, const int64_t* pos, const int64_t* row_idx,
        const void* q_override, void* q_out, void* k_cache, void* v_cache, int K, int q_heads, int kv_heads, int head_dim,
        long long cos_sin_stride, int cos_sin_rows, long long cache_stride_h, int cache_rows, int rope_mode, skv_stream_t stream) {
    return skv_qkv_gemv_rope_update_entry<GemvFp8>(Wqkv8, scale, x, residual, norm_weight, eps, h_out, bias, cos_sin, pos, row_idx,
                                                    q_override, q_out, k_cache, v_cache, K, q_heads, kv_heads, head_dim, cos_sin_stride,
                                                    cos_sin_rows, cache_stride_h, cache_rows, rope_mode, stream);
}

extern "C" int skv_norm_gemv_near_pull_fp8(const void* W8, const void* scale, const void* x, const void* residual,
        const void* norm_weight, float eps, void* h_out, void* y, int N, int K, void* early_state, int blocks, int groups, int n_landmarks,
        int n_chunks, int early_max, const void* v_host, long long host_block_stride, int pull_parts, int active_lists, skv_stream_t stream) {
    return skv_norm_gemv_near_pull_entry<GemvFp8>(W8, scale, x, residual, norm_weight, eps, h_out, y, N, K, early_state, blocks, groups,
                                                   n_landmarks, n_chunks, early_max, v_host, host_block_stride, pull_parts, active_lists,
                                                   stream);
}

extern "C" int skv_gemv_near_pull_fp8(const void* W8, const void* scale, const void* x, const void* bias, void* y, int N, int K,
        void* early_state, int blocks, int groups, int n_landmarks, int n_chunks, int early_max, const void* v_host,
        long long host_block_stride, int pull_parts, int list, skv_stream_t stream) {
    return skv_gemv_near_pull_entry<GemvFp8>(W8, scale, x, bias, y, N, K, early_state, blocks, groups, n_landmarks, n_chunks, early_max,
                                              v_host, host_block_stride, pull_parts, list, stream);
}
