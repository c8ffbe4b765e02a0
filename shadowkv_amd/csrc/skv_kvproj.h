// The fused QKV projection of one decode token, split by rows (skv_gemv.hip keeps the q rows as a launch of their own):
// the RoPE / cache-append epilogue that the GEMV kernels' QKV variant (skv_gemv_frame.h) shares with the k/v ROLE of a later
// launch, the block-cooperative residual add + RMSNorm prologue - the ONE statement of it: both GEMV kernels and the role
// call it - and the role itself.
//
// The landmark scan needs only q, so the k and v rows (2 * Hkv * 128 of the (Hq + 2 Hkv) * 128 weight rows, 16.8 of 50 MB
// at Llama-3.1-8B) need not stream in front of it: extra workgroups of the scan launch or of the top-k launch compute
// them.  Nothing reads the new token's K / V row before the fetch launch, which follows both.  Per-row arithmetic is the
// fused kernel's: same element -> thread mapping of the prologue (its first 256 threads), same lane -> element mapping,
// k-step order and reduction tree of a row, same epilogue - the cache row holds the same bits.
#pragma once
#include "skv_common.h"


struct QkvEpilogue {
    const bf16_t* cos_sin;
    const int64_t* pos;       // [1]
    const int64_t* row_idx;   // [1]
    const bf16_t* q_override; // nullable [Hq][128]
    bf16_t* q_out;            // [Hq][128]
    bf16_t* k_cache;          // [Hkv][cache_rows][128]
    bf16_t* v_cache;
    long long cs_stride, cache_stride_h;
    int Hq, Hkv, cache_rows, glm, cs_rows;
};

// k/v role of a selection launch; blocks == 0: the launch has no such role
struct KvProj {
    const bf16_t* W;          // fused [q; k; v] weights [(Hq + 2 Hkv) * 128][4096]
    const bf16_t* h;          // [4096] the residual stream the q launch stored (or its input where it had no residual to add)
    const bf16_t* w_norm;     // [4096]
    const bf16_t* bias;       // nullable [(Hq + 2 Hkv) * 128]
    float eps;
    int blocks;               // role workgroups of the launch
    QkvEpilogue qe;
};
// rotation pairs (= waves) the role covers, and its workgroups in a launch of `threads` threads per workgroup
__host__ __device__ static inline int skv_kv_proj_pairs(int kv_heads) { return kv_heads * 128; }
__host__ __device__ static inline int skv_kv_proj_blocks(int kv_heads, int threads) { return (skv_kv_proj_pairs(kv_heads) + threads / 64 - 1) / (threads / 64); }

// h = x + residual (bf16; residual null: h = x), RMS statistics, xn = bf16(h * rstd * w_norm) into s_xn [512] (vector v = the
// 8 elements 8 v ..): threads 0 .. 255 of the workgroup split the 4096 elements exactly like skv_add_rmsnorm_kernel (thread t
// owns 16-B vectors t and t + 256, same per-thread order, same wave tree, same (s0+s1)+(s2+s3)).  WIDE: the workgroup has
// more than 256 threads; the others only take part in the two barriers.
// Two halves.  skv_norm_prologue_load requests the thread's vectors of x, residual and w_norm; skv_norm_prologue_4096 computes.
// A caller that streams weights puts its prefetch BETWEEN the two: the memory counter retires in order, so the compute half
// then waits for these (L2-resident) vectors only and its arithmetic and barriers run while the weights fly; w_norm is on
// its way before the first barrier instead of being a round trip of its own behind it.
struct NormOperands {
    u32x4 x[2], r[2], g[2];
};
template <bool WIDE>
__device__ __forceinline__ NormOperands skv_norm_prologue_load(const bf16_t* __restrict__ x, const bf16_t* __restrict__ residual,
                                                               const bf16_t* __restrict__ w_norm, int tid) {
    NormOperands in{};
    const bf16_t* r = residual ? residual : x;      // (no residual: x once more, unused - a conditional load would be waited for)
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int v = (WIDE ? tid & 255 : tid) + it * 256;      // (WIDE: the threads past 255 load and compute nothing they keep)
        in.x[it] = reinterpret_cast<const u32x4*>(x)[v];
        in.r[it] = reinterpret_cast<const u32x4*>(r)[v];
        if (w_norm) in.g[it] = reinterpret_cast<const u32x4*>(w_norm)[v];       // (null: the caller passes it to the compute half)
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);    // (no instruction: the loads stay here, in front of what the caller requests next)
    return in;
}
template <bool WIDE>
__device__ __forceinline__ void skv_norm_prologue_4096(const NormOperands& in, bool has_residual, bf16_t* __restrict__ h_out,
                                                       int K /* 4096 */, float eps, int tid, u32x4* s_xn, float* s_ss,
                                                       const bf16_t* __restrict__ late_w_norm = nullptr) {
    const bool on = !WIDE || tid < 256;
    const int lane = tid & 63, wave = tid >> 6;
    u32x4 hx[2];
    if (on) {
        float ss = 0.f;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            u32x4 a = in.x[it];
            const u32x4 c = in.r[it];
#pragma unroll
            for (int j = 0; j < 4; ++j) {       // (a select, no branch: a load used in one arm only is moved into it and waited for)
                const uint32_t sum = pack_bf2(bf_lo(a[j]) + bf_lo(c[j]), bf_hi(a[j]) + bf_hi(c[j]));
                a[j] = has_residual ? sum : a[j];
            }
            hx[it] = a;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ss = __builtin_fmaf(bf_lo(a[j]), bf_lo(a[j]), ss);
                ss = __builtin_fmaf(bf_hi(a[j]), bf_hi(a[j]), ss);
            }
        }
        if (h_out) {
#pragma unroll
            for (int it = 0; it < 2; ++it) reinterpret_cast<u32x4*>(h_out)[tid + it * 256] = hx[it];
        }
        ss = wave_tree_sum(ss);
        if (lane == 0) s_ss[wave] = ss;
    }
    __syncthreads();
    if (on) {
        const float tot = (s_ss[0] + s_ss[1]) + (s_ss[2] + s_ss[3]);
        const float rstd = 1.0f / sqrtf(tot / (float)K + eps);
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            // (late_w_norm: a caller without the registers to hold w_norm across the barrier did not request it with x)
            const u32x4 g = late_w_norm ? reinterpret_cast<const u32x4*>(late_w_norm)[tid + it * 256] : in.g[it];
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = pack_bf2(bf_lo(hx[it][j]) * rstd * bf_lo(g[j]), bf_hi(hx[it][j]) * rstd * bf_hi(g[j]));
            s_xn[tid + it * 256] = o;
        }
    }
    __syncthreads();
}
// both halves back to back, for a caller with nothing to put between them
template <bool WIDE>
__device__ __forceinline__ void skv_norm_prologue_4096(const bf16_t* __restrict__ x, const bf16_t* __restrict__ residual,
                                                       const bf16_t* __restrict__ w_norm, bf16_t* __restrict__ h_out, int K /* 4096 */,
                                                       float eps, int tid, u32x4* s_xn, float* s_ss) {
    const NormOperands in = skv_norm_prologue_load<WIDE>(x, residual, w_norm, tid);
    skv_norm_prologue_4096<WIDE>(in, residual != nullptr, h_out, K, eps, tid, s_xn, s_ss);
}

// A wave that owns R / 2 rotation pairs of ONE head (rows[], totals tot[]): bias, rounding to the projection's bf16 output,
// RoPE at the token's position for q / k, then q -> q_out, k / v -> the cache row (same arithmetic as
// skv_qkv_rope_update_kernel).  The loads are split from the arithmetic and run IN FRONT of the weight stream, in two steps:
// skv_qkv_epilogue_fetch requests what depends on no other load (bias, the position, the cache row index of a k / v head, the
// q_override values of a q head) and goes before the first weight request; skv_qkv_epilogue_fetch_cs requests the wave's cos /
// sin values at that position and goes behind it - the memory counter retires in order, so waiting for the position there
// leaves every weight request in flight.  skv_qkv_epilogue_apply (lane 0) is arithmetic and stores only.  Every address is
// the wave's, not the lane's, and every load is unconditional - where the value is not needed the address is one that is
// known to be readable (`spare`, bf16 [1]) - so no branch and no wait for a value stands in front of the stream.
template <int R>
struct QkvOperands {
    long long row, pos;       // cache row of a k / v head, the token's position
    bf16_t bias[R];
    bf16_t c[R / 2], sn[R / 2];   // cos / sin of the pairs that rotate
    bf16_t ov[R];             // q_override values of a q head
};
template <int R>
__device__ __forceinline__ QkvOperands<R> skv_qkv_epilogue_fetch(const QkvEpilogue& qe, const bf16_t* __restrict__ bias,
                                                                 const int (&rows)[R], int unit0, const bf16_t* spare) {
    const int head = unit0 / 128;                       // the wave's R rows belong to one head
    QkvOperands<R> op{};
    op.pos = *qe.pos;
    op.row = *(head >= qe.Hq ? qe.row_idx : qe.pos);    // (a q head pushes no row)
    const bool ov = head < qe.Hq && qe.q_override;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        op.bias[r] = *(bias ? bias + rows[r] : spare);
        op.ov[r] = *(ov ? qe.q_override + (size_t)head * 128 + (rows[r] - head * 128) : spare);
    }
    return op;
}
template <int R>
__device__ __forceinline__ void skv_qkv_epilogue_fetch_cs(QkvOperands<R>& op, const QkvEpilogue& qe, const int (&rows)[R], int unit0) {
    const int head = unit0 / 128;
    const long long pcl = min(max(op.pos, 0ll), (long long)qe.cs_rows - 1);   // see skv_dense.hip
    const bf16_t* cs = qe.cos_sin + pcl * qe.cs_stride;
#pragma unroll
    for (int p = 0; p < R / 2; ++p) {
        const int d1 = rows[2 * p] - head * 128;
        // NeoX: pair (t, t+64), cos[t], sin[64+t]; GLM: pair (2t, 2t+1), cos[t], sin[32+t] for t < 32, the rest passes through
        const bool rot = head < qe.Hq + qe.Hkv && (!qe.glm || d1 < 64);
        const int t = qe.glm ? d1 >> 1 : d1;
        op.c[p] = cs[rot ? t : 0];
        op.sn[p] = cs[rot ? t + (qe.glm ? 32 : 64) : 0];
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);    // (no instruction: keeps the compiler from sinking these loads to their use)
}
template <int R>
__device__ __forceinline__ void skv_qkv_epilogue_apply(const QkvEpilogue& qe, bool has_bias, const QkvOperands<R>& op,
                                                       const int (&rows)[R], const float (&tot)[R], int unit0) {
    const int head = unit0 / 128;
    float o[R];
#pragma unroll
    for (int r = 0; r < R; ++r) o[r] = bfr(has_bias ? bfr(tot[r]) + bf2f(op.bias[r]) : tot[r]);  // the projection output is bf16
    const long long row = op.row;
    if (head >= qe.Hq + qe.Hkv) {                       // V: copy into the cache row
        if (row >= 0 && row < qe.cache_rows) {
            bf16_t* dst = qe.v_cache + (long long)(head - qe.Hq - qe.Hkv) * qe.cache_stride_h + row * 128;
#pragma unroll
            for (int r = 0; r < R; ++r) dst[rows[r] - head * 128] = f2bf(o[r]);
        }
        return;
    }
    float res[R];
    int dim[R];
#pragma unroll
    for (int p = 0; p < R / 2; ++p) {
        const int d1 = rows[2 * p] - head * 128, d2 = rows[2 * p + 1] - head * 128;
        dim[2 * p] = d1; dim[2 * p + 1] = d2;
        const float x1 = o[2 * p], x2 = o[2 * p + 1];
        if (!qe.glm || d1 < 64) {
            const float c = bf2f(op.c[p]), sn = bf2f(op.sn[p]);
            res[2 * p] = bfr(x1 * c) + bfr(-x2 * sn);
            res[2 * p + 1] = bfr(x2 * c) + bfr(x1 * sn);
        } else {
            res[2 * p] = x1; res[2 * p + 1] = x2;   // pass-through dims
        }
    }
    if (head < qe.Hq) {
        bf16_t* dst = qe.q_out + (size_t)head * 128;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float v = res[r];
            if (qe.q_override) v = bf2f(op.ov[r]) + v * 0.0f;
            dst[dim[r]] = f2bf(v);
        }
    } else if (row >= 0 && row < qe.cache_rows) {
        bf16_t* dst = qe.k_cache + (long long)(head - qe.Hq) * qe.cache_stride_h + row * 128;
#pragma unroll
        for (int r = 0; r < R; ++r) dst[dim[r]] = f2bf(res[r]);
    }
}

#define SKV_KV_PROJ_LDS_BYTES (512 * 16 + 16)      // xn [512] u32x4 + the prologue's four wave sums

// The k/v role: workgroup `rb` of kp.blocks, THREADS threads; every wave owns ONE rotation pair of a k or v head, as a wave
// of the fused launch does (its wave index there: Hq * 64 + pair).  DEEP: all eight 1-KiB segments of both rows are requested
// before the first use (64 VGPRs); otherwise two k-steps at a time, for a host kernel that runs at a 64-VGPR budget.
template <int THREADS, bool DEEP>
__device__ __forceinline__ void skv_kv_proj_role(const KvProj& kp, int rb, int tid, unsigned char* lds) {
    u32x4* s_xn = reinterpret_cast<u32x4*>(lds);
    float* s_ss = reinterpret_cast<float*>(lds + 512 * 16);
    const int lane = tid & 63, wave = tid >> 6;
    const int pair = rb * (THREADS / 64) + wave;
    const bool active = pair < skv_kv_proj_pairs(kp.qe.Hkv);
    const int w = kp.qe.Hq * 64 + (active ? pair : 0);  // (an idle wave of the last workgroup reads pair 0 and writes nothing)
    const int unit0 = 2 * w;
    int rows[2];
    if (kp.qe.glm) {
        rows[0] = unit0; rows[1] = unit0 + 1;
    } else {
        rows[0] = (w / 64) * 128 + (w % 64); rows[1] = rows[0] + 64;
    }
    const bf16_t* wp[2] = {kp.W + (size_t)rows[0] * 4096 + 8 * lane, kp.W + (size_t)rows[1] * 4096 + 8 * lane};
    constexpr int PRE = DEEP ? 8 : 2;
    // DEEP, order of the requests: the prologue's operands, the epilogue's, then the weights (the counter retires in order: the
    // prologue computes while the weights are on their way).  At the 64-VGPR budget there is no room to hold them that long.
    constexpr bool NORM_FIRST = DEEP, FETCH_FIRST = DEEP;
    NormOperands in;
    QkvOperands<2> op{};
    if constexpr (NORM_FIRST) in = skv_norm_prologue_load<(THREADS > 256)>(kp.h, nullptr, kp.w_norm, tid);
    if constexpr (FETCH_FIRST) op = skv_qkv_epilogue_fetch<2>(kp.qe, kp.bias, rows, unit0, kp.w_norm);
    u32x4 wv[2][PRE];
#pragma unroll
    for (int u = 0; u < PRE; ++u)
#pragma unroll
        for (int r = 0; r < 2; ++r) wv[r][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)u * 512));
    if constexpr (!NORM_FIRST) in = skv_norm_prologue_load<(THREADS > 256)>(kp.h, nullptr, nullptr, tid);
    skv_norm_prologue_4096<(THREADS > 256)>(in, false, nullptr, 4096, kp.eps, tid, s_xn, s_ss, NORM_FIRST ? nullptr : kp.w_norm);
    if constexpr (FETCH_FIRST) skv_qkv_epilogue_fetch_cs<2>(op, kp.qe, rows, unit0);
    f32x2 acc[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[r][j] = (f32x2){0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ks += PRE) {
        if (ks > 0) {
#pragma unroll
            for (int u = 0; u < PRE; ++u)
#pragma unroll
                for (int r = 0; r < 2; ++r)
                    wv[r][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[r] + (size_t)(ks + u) * 512));
        }
#pragma unroll
        for (int u = 0; u < PRE; ++u) {
            const u32x4 o = s_xn[(ks + u) * 64 + lane];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2 xx = (f32x2){bf_lo(o[j]), bf_hi(o[j])};
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const f32x2 ww = (f32x2){bf_lo(wv[r][u][j]), bf_hi(wv[r][u][j])};
                    acc[r][j] = __builtin_elementwise_fma(ww, xx, acc[r][j]);
                }
            }
        }
    }
    float tot[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        float s = ((acc[r][0].x + acc[r][0].y) + (acc[r][1].x + acc[r][1].y)) +
                  ((acc[r][2].x + acc[r][2].y) + (acc[r][3].x + acc[r][3].y));
        tot[r] = wave_tree_sum(s);
    }
    if constexpr (!FETCH_FIRST) {
        if (lane == 0 && active) {       // (at the 64-VGPR budget: the writing lane alone, behind the reduction, as before)
            op = skv_qkv_epilogue_fetch<2>(kp.qe, kp.bias, rows, unit0, kp.w_norm);
            skv_qkv_epilogue_fetch_cs<2>(op, kp.qe, rows, unit0);
        }
    }
    if (lane == 0 && active) skv_qkv_epilogue_apply<2>(kp.qe, kp.bias != nullptr, op, rows, tot, unit0);
}
