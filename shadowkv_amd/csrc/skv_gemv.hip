// bf16 GEMV for the decode step's dense projections (q_len == 1, one token per sequence):
//     y[n] = sum_k W[n][k] * x[k] (+ bias[n]),   W [N][K] row-major (K contiguous), f32 accumulation, bf16 out
// and the gate/up variant with the activation fused in the epilogue (W = [gate; up], 2I rows):
//     y[i] = bf16(silu(W[i].x)) * (W[I+i].x)
// Replaces F.linear -> hipBLASLt for M = 1 (at bs = 1 the
// 15 GB of weights are the largest HBM term of a decode step; the library kernels run them at 2.2-4.7 TB/s).
//
// K % 8 == 0, K >= 512 (a partial last 512-element step is handled after the main loop).
// HBM-bound streaming: a wave owns R weight rows; each wave-instruction reads 1 KiB of a row (64 lanes x
// 16 B, coalesced), x (<= 28 KB) comes from L2.  Per 16 B of weights: 8 conversions + 4 packed FMAs, far below the
// VALU roof.  Rows are reduced over the 64 lanes with a DPP butterfly + two cross-row shuffles; lane 0 writes.
//
// What a launch that fits the chip in one round of workgroups (q, O, down) is bound by is not HBM but the number of
// dependent memory round trips of a wave, so the points where loads are ISSUED are chosen to leave none the result does
// not need (the order of every accumulator's FMAs - k-steps ascending, tail last - and the reduction tree are untouched):
//   * without the norm prologue the stream is a software pipeline: the next group of k-steps (x and weights, 8 KB of
//     weights per wave) is requested before the FMAs of the current one, so two groups are in flight at every moment;
//   * with it, the prologue's x / residual / w_norm vectors are requested BEFORE the weight prefetch: the memory counter
//     retires in order, so the prologue waits for its own L2-resident vectors only and computes while the weights fly;
//   * the epilogue's operands (bias; QKV: position, cache row, cos / sin, q_override) are requested in front of the stream,
//     not after the reduction.
// Registers: the two-row instances stay within 128 VGPRs (four waves per SIMD), the four-row ones within 168 (three);
// __launch_bounds__ states those budgets, and scalar row bases + one 32-bit lane offset keep the addresses out of them.
//
// This file holds the bf16 weight stream (prefetch, main loop, K tail) and the bf16 entries.  The frame around the stream -
// near-pull role, row ownership, row total, epilogue, the launch branch tree - is skv_gemv_frame.h, shared with
// skv_gemv_fp8.hip; the norm prologue is skv_norm_prologue_4096 (skv_kvproj.h); near_pull_of is in skv_launch.h.
#include "../../include/shadowkv_hip.h"
#include "skv_gemv_frame.h"

#ifndef SKV_GEMV_PRE_R2
#define SKV_GEMV_PRE_R2 4      // k-steps of weights a two-row wave of the NORM variant requests before its norm prologue.  8 (all up
                               // front) lost in round 5 (142 VGPRs; 228.8-230.1 tokens/s against 230.3-231.3) while the prologue still
                               // waited for those weights; now that it does not, 8 does not fit: with the prologue's operands held
                               // across the prefetch the q instance needs scratch at its 128 VGPRs and the build refuses it
#endif

// NORM variant (K == 4096): x is the pre-norm hidden state; every BLOCK recomputes h = x + residual (bf16), the
// RMS statistics and xn = bf16(h * rstd * w_norm) cooperatively (skv_norm_prologue_4096), so "residual add + RMSNorm +
// projection" is one launch; block 0 stores h (the new residual stream).  Bit-identical to the separate launch.
// QKV, N = Hq * 128: the q rows alone (skv_q_gemv_rope) - the k / v rows are then the role of a later launch (skv_kvproj.h).
// The other template parameters: skv_gemv_frame.h.
template <int R, bool SILU_PAIR, bool NORM, bool QKV, bool RMAX = false, bool NEARP = false>
__global__ __launch_bounds__(256, R <= 2 ? 4 : 3) void skv_gemv_kernel(const bf16_t* __restrict__ W, const bf16_t* __restrict__ x,
                                                       const bf16_t* __restrict__ bias, bf16_t* __restrict__ y, int N,
                                                       int K, int I /* SILU_PAIR: rows of one half */,
                                                       const bf16_t* __restrict__ residual,
                                                       const bf16_t* __restrict__ w_norm, bf16_t* __restrict__ h_out,
                                                       float eps, QkvEpilogue qe, uint16_t* __restrict__ range_max = nullptr,
                                                       NearPull np = NearPull{}) {
    int bx = blockIdx.x;
    if (skv_gemv_near_pull_block<NEARP>(np, bx)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform by construction; said so, the row bases are scalars
    const int ksteps = NORM ? 8 : K / 512;  // 64 lanes x 8 elements per step (NORM: K == 4096, static trip count)
    int rows[R];
    const int unit0 = (bx * 4 + wave) * (SILU_PAIR ? R / 2 : R);
    skv_gemv_wave_rows<R, SILU_PAIR, QKV>(rows, unit0, I, qe.glm);
    const int limit = SILU_PAIR ? I : N;      // units of the launch
    if (!NORM && unit0 >= limit) return;   // (NORM: every wave takes part in the block-wide prologue first)
    // addresses: a scalar base (the row is the wave's) + a 32-bit element offset per lane - one address register for all rows and x
    const bf16_t* wrow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) wrow[r] = W + (size_t)skv_gemv_stream_row<R, SILU_PAIR>(rows, r, unit0, limit, I) * K;
    uint32_t kbytes = 0;                         // bytes of the row behind the stream (uniform)
    auto wload = [&](int r, int ks) {            // ks: k-steps from there, a constant at every call - the instruction's immediate offset
        return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(wrow[r]) + (kbytes + 16u * lane) + 1024 * ks));
    };
    auto xload = [&](int ks) { return *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(x) + (kbytes + 16u * lane) + 1024 * ks); };
    // Order of the requests: the norm prologue's operands and the epilogue's first, the weights behind them.  The memory counter
    // retires in order, so the prologue waits for its own (L2-resident) vectors only and computes while the weights fly, and
    // the epilogue's operands - position -> cos / sin is a dependent pair - are back long before the reduction ends.
    NormOperands nin;
    if (NORM) nin = skv_norm_prologue_load<false>(x, residual, w_norm, tid);
    int erows[R];            // (a wave past the end of the launch - it stays for the prologue's barriers - fetches for unit 0)
    const int eunit = unit0 < limit ? unit0 : 0;
#pragma unroll
    for (int r = 0; r < R; ++r) erows[r] = unit0 < limit ? rows[r] : 0;
    QkvOperands<R> eop{};
    eop = skv_gemv_epilogue_fetch<R, SILU_PAIR, QKV>(erows, eunit, N, bias, qe, x);
    if (!NORM) skv_gemv_epilogue_fetch_cs<R, QKV>(eop, qe, erows, eunit);   // (NORM: behind the weight prefetch)
    f32x2 acc[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[r][j] = (f32x2){0.f, 0.f};
    // one k-step of one row into its accumulators: acc[r][j] = fma(w, x, acc[r][j]), k-steps ascending in every variant below
    auto step = [&](const u32x4 (&w)[R], const f32x2 (&xx)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < R; ++r)
                acc[r][j] = __builtin_elementwise_fma((f32x2){bf_lo(w[r][j]), bf_hi(w[r][j])}, xx[j], acc[r][j]);
    };

    if constexpr (NORM) {
        // K == 4096, eight k-steps: the first PRE of every row are requested before the prologue computes, the rest behind it
        constexpr int PRE = R <= 2 ? SKV_GEMV_PRE_R2 : 4;
        u32x4 wpre[PRE][R];
#pragma unroll
        for (int u = 0; u < PRE; ++u)
#pragma unroll
            for (int r = 0; r < R; ++r)
                wpre[u][r] = wload(r, u);
        // xn goes through LDS and every wave picks up its k-step slices (vector 64 u + lane for step u)
        __shared__ u32x4 s_xn[512];
        __shared__ float s_ss[4];
        skv_norm_prologue_4096<false>(nin, residual != nullptr, bx == 0 ? h_out : nullptr, K, eps, tid, s_xn, s_ss);
        skv_gemv_epilogue_fetch_cs<R, QKV>(eop, qe, erows, eunit);
        f32x2 xn[8][4];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const u32x4 o = s_xn[u * 64 + lane];
#pragma unroll
            for (int j = 0; j < 4; ++j) xn[u][j] = (f32x2){bf_lo(o[j]), bf_hi(o[j])};
        }
        if (unit0 >= limit) return;
#pragma unroll
        for (int ks = 0; ks < 8; ks += 4) {
            u32x4 wv[4][R];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (ks + u < PRE) wv[u][r] = wpre[ks + u][r];
                    else wv[u][r] = wload(r, ks + u);
                }
#pragma unroll
            for (int u = 0; u < 4; ++u) step(wv[u], xn[ks + u]);
        }
    } else {
        // The stream as a software pipeline over groups of GS k-steps: group g + 1 (x and weights) is requested before group
        // g's FMAs, so a wave has two groups - 16 KB of weights - on their way at every moment and the stream never drains
        // between groups; K <= 8 * 512 at two rows per wave (the O projection) is in flight whole before the first FMA.  The
        // end of a row that is no whole number of groups - ksteps % GS steps and the K % 512 tail (lanes below the tail only)
        // - is one more request behind the drain (requested ahead of it, the conditional steps cost more registers than the
        // budget of four waves per SIMD leaves).
        constexpr int GS = R <= 2 ? 4 : 2;
        struct Group {
            u32x4 w[GS][R], x[GS];
        };
        auto request = [&](Group& g, int ks) {
#pragma unroll
            for (int u = 0; u < GS; ++u) {
                g.x[u] = xload(ks + u);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    g.w[u][r] = wload(r, ks + u);
            }
        };
        // the stream moves on by a group: every request has its immediate offsets within one.  (readfirstlane: the offset is
        // uniform, and as a plain induction variable the compiler would turn it into a 64-bit vector address per row - six
        // registers the two-row stream does not have.)
        auto advance = [&]() { kbytes = __builtin_amdgcn_readfirstlane(kbytes + GS * 1024u); };
        auto one = [&](const Group& g, int u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2 xx = (f32x2){bf_lo(g.x[u][j]), bf_hi(g.x[u][j])};
#pragma unroll
                for (int r = 0; r < R; ++r)
                    acc[r][j] = __builtin_elementwise_fma((f32x2){bf_lo(g.w[u][r][j]), bf_hi(g.w[u][r][j])}, xx, acc[r][j]);
                __builtin_amdgcn_sched_barrier(0);     // conversions stay next to their FMAs: unpacked, a group holds twice
            }                                          // the registers; and no request sinks below a step
        };
        auto fmas = [&](const Group& g) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < GS; ++u) one(g, u);
        };
        const int full = ksteps - ksteps % GS, rem = ksteps % GS;
        const bool tail = lane < (K % 512) / 8;      // K % 512 != 0 (GLM-4: 13696 = 26 x 512 + 384)
        // the end of the row: rem whole steps in slots 0 .. rem - 1 and the tail in the last slot (rem < GS: it is free)
        auto request_end = [&](Group& g) {
#pragma unroll
            for (int u = 0; u < GS - 1; ++u) {
                if (u < rem) {
                    g.x[u] = xload(u);
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        g.w[u][r] = wload(r, u);
                }
            }
            if (tail) {
                g.x[GS - 1] = xload(rem);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    g.w[GS - 1][r] = wload(r, rem);
            }
        };
        auto fmas_end = [&](const Group& g) {
#pragma unroll
            for (int u = 0; u < GS - 1; ++u) {
                __builtin_amdgcn_sched_barrier(0);
                if (u < rem) one(g, u);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (tail) one(g, GS - 1);
        };
        Group ga, gb;
        if (full > 0) {
            request(ga, 0);
            int left = full;                                // whole k-steps from ga's group on
            // steady state (three or more groups left): no branch between a request and the FMAs in front of it
            for (; left >= 3 * GS; left -= 2 * GS) {
                advance();
                request(gb, 0);
                fmas(ga);
                advance();
                request(ga, 0);
                fmas(gb);
            }
            const bool two = left >= 2 * GS;                // drain: two whole groups left, or one
            if (two) {
                advance();
                request(gb, 0);
            }
            fmas(ga);                                       // (stated once: in both arms of one branch its conversions are
            if (two) fmas(gb);                              // hoisted in front of the request and ga doubles in registers)
            advance();
        }
        Group ge;           // (a buffer of its own: a partial request into ga or gb would keep their old contents alive)
        request_end(ge);
        fmas_end(ge);
    }
    float tot[R];
#pragma unroll
    for (int r = 0; r < R; ++r) tot[r] = skv_gemv_row_total(acc[r]);
    skv_gemv_epilogue<R, SILU_PAIR, QKV, RMAX>(rows, tot, unit0, bx, tid, N, I, bias != nullptr, eop, y, qe, range_max);
}

// the bf16 format of the host entries (skv_gemv_frame.h)
struct GemvBf16 : GemvArgs {
    static constexpr int K_STEP = 8, K_MIN = 512;
    static constexpr bool SCALED = false;
    static constexpr bool Q_ROWS_ALONE = true;       // N = Hq * 128: skv_q_gemv_rope
    static constexpr bool NEAR_ROLE_ARGS_FIRST = true;      // a near-pull entry checks the role's arguments first, then the GEMV's own
    static constexpr bool QKV_REFUSES_NO_HEADS = false;     // the QKV entry with no heads: left to the GEMV's checks of N and K
    const bf16_t* W;
    GemvBf16(const GemvArgs& a, const void* w, const void*) : GemvArgs(a), W((const bf16_t*)w) {}
    template <int R, bool SILU, bool NORM, bool QKV, bool RMAX, bool NEARP>
    void launch(int grid, int I, uint16_t* range_max, const NearPull& near) const {
        hipLaunchKernelGGL((skv_gemv_kernel<R, SILU, NORM, QKV, RMAX, NEARP>), dim3(grid), dim3(256), 0, st, W, x, bias, y, N, K, I,
                           residual, w_norm, h_out, eps, qe, range_max, near);
    }
};

extern "C" int skv_gemv_bf16(const void* W, const void* x, const void* bias, void* y, int N, int K, int fuse_silu_mul,
                             skv_stream_t stream) {
    return skv_gemv_entry<GemvBf16>(W, nullptr, x, bias, y, N, K, fuse_silu_mul, stream);
}

extern "C" int skv_norm_gemv_bf16(const void* W, const void* x, const void* residual, const void* norm_weight, float eps,
                                  void* h_out, const void* bias, void* y, int N, int K, int fuse_silu_mul,
                                  skv_stream_t stream) {
    return skv_norm_gemv_entry<GemvBf16>(W, nullptr, x, residual, norm_weight, eps, h_out, bias, y, N, K, fuse_silu_mul, stream);
}

extern "C" int skv_norm_gemv_near_pull_bf16(const void* W, const void* x, const void* residual, const void* norm_weight, float eps,
                                            void* h_out, void* y, int N, int K, void* early_state, int blocks, int groups,
                                            int n_landmarks, int n_chunks, int early_max, const void* v_host,
                                            long long host_block_stride, int pull_parts, int active_lists, skv_stream_t stream) {
    return skv_norm_gemv_near_pull_entry<GemvBf16>(W, nullptr, x, residual, norm_weight, eps, h_out, y, N, K, early_state, blocks, groups,
                                                   n_landmarks, n_chunks, early_max, v_host, host_block_stride, pull_parts, active_lists,
                                                   stream);
}

extern "C" int skv_gemv_near_pull_bf16(const void* W, const void* x, const void* bias, void* y, int N, int K, void* early_state,
                                       int blocks, int groups, int n_landmarks, int n_chunks, int early_max, const void* v_host,
                                       long long host_block_stride, int pull_parts, int list, skv_stream_t stream) {
    return skv_gemv_near_pull_entry<GemvBf16>(W, nullptr, x, bias, y, N, K, early_state, blocks, groups, n_landmarks, n_chunks, early_max,
                                              v_host, host_block_stride, pull_parts, list, stream);
}

extern "C" int skv_norm_gemv_rangemax_bf16(const void* W, const void* x, const void* residual, const void* norm_weight, float eps,
                                           void* h_out, const void* bias, void* y, int N, int K, void* range_max,
                                           skv_stream_t stream) {
    return skv_norm_gemv_rangemax_entry<GemvBf16>(W, nullptr, x, residual, norm_weight, eps, h_out, bias, y, N, K, range_max, stream);
}

extern "C" int skv_qkv_gemv_rope_update(const void* Wqkv, const void* x, const void* residual, const void* norm_weight,
                                        float eps, void* h_out, const void* bias, const void* cos_sin, const int64_t* pos,
                                        const int64_t* row_idx, const void* q_override, void* q_out, void* k_cache,
                                        void* v_cache, int K, int q_heads, int kv_heads, int head_dim,
                                        long long cos_sin_stride, int cos_sin_rows, long long cache_stride_h, int cache_rows,
                                        int rope_mode, skv_stream_t stream) {
    return skv_qkv_gemv_rope_update_entry<GemvBf16>(Wqkv, nullptr, x, residual, norm_weight, eps, h_out, bias, cos_sin, pos, row_idx,
                                                    q_override, q_out, k_cache, v_cache, K, q_heads, kv_heads, head_dim, cos_sin_stride,
                                                    cos_sin_rows, cache_stride_h, cache_rows, rope_mode, stream);
}

// The q rows of skv_qkv_gemv_rope_update alone: same kernel, same waves, a grid that ends behind the last q head.  The k / v
// rows follow as the role of this layer's selection launch (skv_select_chunks_fused_kv_proj), which reads the h stored here.
extern "C" int skv_q_gemv_rope(const void* Wqkv, const void* x, const void* residual, const void* norm_weight, float eps,
                               void* h_out, const void* bias, const void* cos_sin, const int64_t* pos, const void* q_override,
                               void* q_out, int K, int q_heads, int kv_heads, int head_dim, long long cos_sin_stride,
                               int cos_sin_rows, int rope_mode, skv_stream_t stream) {
    if (!cos_sin || !pos || !q_out || !norm_weight || cos_sin_rows < 1 || q_heads < 1 || kv_heads < 1) return SKV_ERR_ARG;
    if (head_dim != 128 || K != 4096 || (rope_mode != 1 && rope_mode != 2)) return SKV_ERR_UNSUPPORTED;
    // (no wave of this grid owns a k or v head: the caches are never touched, and the row index every wave's lane 0 loads goes unused)
    QkvEpilogue qe{(const bf16_t*)cos_sin, pos, pos, (const bf16_t*)q_override, (bf16_t*)q_out, nullptr, nullptr, cos_sin_stride, 0,
                   q_heads, kv_heads, 0, rope_mode == 2, cos_sin_rows};
    return skv_gemv_launch<GemvBf16>(Wqkv, nullptr, x, bias, nullptr, q_heads * 128, K, 0, residual, norm_weight, h_out, eps, true, stream, &qe);
}
