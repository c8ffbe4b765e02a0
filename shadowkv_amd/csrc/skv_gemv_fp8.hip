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
// vectors.  Per 16 B of weights: 8 v_cvt_pk_f32_fp8 (gfx950 decodes OCP e4m3fn, not MI300's fnuz) + 8 packed FMAs.  The norm
// prologue is skv_gemv_kernel's, element for element: h and xn are bit-identical to skv_add_rmsnorm; only the pickup of xn from
// LDS differs (vectors 128 u + 2 lane, 128 u + 2 lane + 1 for step u).
#include "../../include/shadowkv_hip.h"
#include "skv_common.h"
#include "skv_early.h"
#include "skv_kvproj.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

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

// Template parameters as in skv_gemv_kernel (skv_gemv.hip): R rows per wave, SILU_PAIR (W = [gate; up]), NORM (residual add +
// RMSNorm prologue, K == 4096), QKV (split + RoPE + cache push in the epilogue), RMAX (the sampler's range keys), NEARP (the
// near-miss pull role in the launch's first np.blocks workgroups).
template <int R, bool SILU_PAIR, bool NORM, bool QKV, bool RMAX = false, bool NEARP = false>
__global__ __launch_bounds__(256) void skv_gemv_fp8_kernel(const uint8_t* __restrict__ W, const float* __restrict__ scale,
                                                           const bf16_t* __restrict__ x, const bf16_t* __restrict__ bias,
                                                           bf16_t* __restrict__ y, int N, int K, int I /* SILU_PAIR: rows of one half */,
                                                           const bf16_t* __restrict__ residual, const bf16_t* __restrict__ w_norm,
                                                           bf16_t* __restrict__ h_out, float eps, QkvEpilogue qe,
                                                           uint16_t* __restrict__ range_max = nullptr, NearPull np = NearPull{}) {
    int bx = blockIdx.x;
    if constexpr (NEARP) {
        if (bx < np.blocks) {
            __shared__ int s_near[6 * 64 + 8];
            skv_near_pull_role(np, bx, threadIdx.x, s_near);
            return;
        }
        bx -= np.blocks;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ksteps = NORM ? 4 : K / 1024;  // 64 lanes x 16 elements per step (NORM: K == 4096, static trip count)
    // rows of this wave (same ownership as skv_gemv_kernel)
    int rows[R];
    const int unit0 = (bx * 4 + wave) * (SILU_PAIR ? R / 2 : R);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (SILU_PAIR) rows[r] = (r & 1) ? I + unit0 + r / 2 : unit0 + r / 2;  // (gate, up) pairs
        else if (QKV && !qe.glm) {
            const int w = unit0 / R, head = w / (128 / R), t0 = (R / 2) * (w % (128 / R));
            rows[r] = head * 128 + t0 + (r >> 1) + ((r & 1) ? 64 : 0);
        } else rows[r] = unit0 + r;
    }
    const int limit = SILU_PAIR ? I : N;
    if (!NORM && unit0 >= limit) return;   // (NORM: every wave takes part in the block-wide prologue first)
    const uint8_t* wp[R];
    float sc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int row = rows[r];
        const int base_unit = SILU_PAIR ? unit0 + r / 2 : unit0 + r;
        if (base_unit >= limit) row = SILU_PAIR ? ((r & 1) ? I : 0) : 0;  // clamp: computed and discarded
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
        // Block-cooperative prologue, restated from skv_gemv_kernel (thread t owns 16-B vectors t and t + 256, same per-thread
        // order, same wave tree, same (s0+s1)+(s2+s3)): h, rstd and xn are bit-identical to skv_add_rmsnorm.
        __shared__ u32x4 s_xn[512];
        __shared__ float s_ss[4];
        u32x4 hx[2];
        float ss = 0.f;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int v = tid + it * 256;
            u32x4 a = reinterpret_cast<const u32x4*>(x)[v];
            if (residual) {
                u32x4 c = reinterpret_cast<const u32x4*>(residual)[v];
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = pack_bf2(bf_lo(a[j]) + bf_lo(c[j]), bf_hi(a[j]) + bf_hi(c[j]));
            }
            hx[it] = a;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ss = __builtin_fmaf(bf_lo(a[j]), bf_lo(a[j]), ss);
                ss = __builtin_fmaf(bf_hi(a[j]), bf_hi(a[j]), ss);
            }
        }
        if (h_out && bx == 0) {
#pragma unroll
            for (int it = 0; it < 2; ++it) reinterpret_cast<u32x4*>(h_out)[tid + it * 256] = hx[it];
        }
        ss = wave_tree_sum(ss);
        if (lane == 0) s_ss[wave] = ss;
        __syncthreads();
        const float tot = (s_ss[0] + s_ss[1]) + (s_ss[2] + s_ss[3]);
        const float rstd = 1.0f / sqrtf(tot / (float)K + eps);
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int v = tid + it * 256;
            u32x4 g = reinterpret_cast<const u32x4*>(w_norm)[v];
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = pack_bf2(bf_lo(hx[it][j]) * rstd * bf_lo(g[j]), bf_hi(hx[it][j]) * rstd * bf_hi(g[j]));
            s_xn[v] = o;
        }
        __syncthreads();
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
    for (int r = 0; r < R; ++r) {
        float s = ((acc[r][0].x + acc[r][0].y) + (acc[r][1].x + acc[r][1].y)) +
                  ((acc[r][2].x + acc[r][2].y) + (acc[r][3].x + acc[r][3].y));
        tot[r] = sc[r] * wave_tree_sum(s);       // the row's scale: one f32 multiply after the reduction
    }
    if (QKV) {
        if (lane == 0 && unit0 < N) skv_qkv_epilogue<R>(qe, bias, rows, tot, unit0);
        return;
    }
    __shared__ uint32_t s_kmax[RMAX ? 4 : 1];
    if (lane == 0) {
        if (SILU_PAIR) {
#pragma unroll
            for (int p = 0; p < R / 2; ++p) {
                const int i = unit0 + p;
                if (i < I) {
                    const float g = bfr(tot[2 * p]), u = bfr(tot[2 * p + 1]);   // the GEMV outputs are bf16 tensors
                    y[i] = f2bf(bfr(g / (1.0f + __expf(-g))) * u);
                }
            }
        } else {
            uint32_t kmax = 0u;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int n = unit0 + r;
                const bf16_t o = f2bf(bias ? bfr(tot[r]) + bf2f(bias[n < N ? n : 0]) : tot[r]);
                if (n < N) y[n] = o;
                if (RMAX) kmax = max(kmax, skv_bf16_order_key(o));
            }
            if constexpr (RMAX) s_kmax[wave] = kmax;
        }
    }
    if constexpr (RMAX && !SILU_PAIR && !QKV) {      // (N % 16 == 0: every wave of every workgroup arrives here)
        __syncthreads();
        if (tid == 0) range_max[bx] = (uint16_t)max(max(s_kmax[0], s_kmax[1]), max(s_kmax[2], s_kmax[3]));
    }
}

// every check of the GEMV's own arguments; host only, before any HIP call
static int gemv_fp8_args(const void* W, const void* scale, const void* x, const void* y, bool qkv, int N, int K, bool norm,
                         const void* w_norm) {
    if (!W || !scale || !x || (!y && !qkv) || N < 1) return SKV_ERR_ARG;
    if (K % 16 || K < 1024) return SKV_ERR_UNSUPPORTED;
    if (norm && (K != 4096 || !w_norm)) return SKV_ERR_UNSUPPORTED;
    return SKV_OK;
}

static int launch_gemv_fp8(const void* W, const void* scale, const void* x, const void* bias, void* y, int N, int K,
                           int fuse_silu_mul, const void* residual, const void* w_norm, void* h_out, float eps, bool norm,
                           hipStream_t st, const QkvEpilogue* qkv = nullptr, uint16_t* range_max = nullptr,
                           const NearPull* near = nullptr) {
    const int rc = gemv_fp8_args(W, scale, x, y, qkv != nullptr, N, K, norm, w_norm);
    if (rc != SKV_OK) return rc;
    QkvEpilogue qe{};
    if (qkv) qe = *qkv;
#define SKV_GEMV8(RR, SILU, NORMF, QKVF, RMAXF, NEARF, GRID, IARG, ...)                                                     \
    hipLaunchKernelGGL((skv_gemv_fp8_kernel<RR, SILU, NORMF, QKVF, RMAXF, NEARF>), dim3(GRID), dim3(256), 0, st,            \
                       (const uint8_t*)W, (const float*)scale, (const bf16_t*)x, (const bf16_t*)bias, (bf16_t*)y, N, K, IARG, \
                       (const bf16_t*)residual, (const bf16_t*)w_norm, (bf16_t*)h_out, eps, qe, __VA_ARGS__)
    if (near) {          // a launch of a layer's dense tail with the near-miss pull role in front of its grid
        if (qkv || range_max || near->blocks < 1 || near->E + SKV_NEAR_SLOTS > 32767) return SKV_ERR_UNSUPPORTED;
        if (norm && fuse_silu_mul && !(N % 2) && !bias) {                    // gate/up: list 0
            const int I = N / 2;
            SKV_GEMV8(4, true, true, false, false, true, near->blocks + (I + 7) / 8, I, (uint16_t*)nullptr, *near);
        } else if (!norm && !fuse_silu_mul && N <= 8192) {                   // down projection (two rows per wave): list 1
            SKV_GEMV8(2, false, false, false, false, true, near->blocks + (N + 7) / 8, 0, (uint16_t*)nullptr, *near);
        } else {
            return SKV_ERR_UNSUPPORTED;
        }
        return hipGetLastError() == hipSuccess ? SKV_OK : SKV_ERR_LAUNCH;
    }
    if (range_max) {     // the lm_head with the sampler's range keys: norm prologue, whole workgroups of 16 rows
        if (!norm || qkv || fuse_silu_mul || N % 16) return SKV_ERR_UNSUPPORTED;
        SKV_GEMV8(4, false, true, false, true, false, N / 16, 0, range_max);
        return hipGetLastError() == hipSuccess ? SKV_OK : SKV_ERR_LAUNCH;
    }
    if (qkv) {
        if (fuse_silu_mul || N != (qe.Hq + 2 * qe.Hkv) * 128) return SKV_ERR_ARG;
        if (norm) SKV_GEMV8(2, false, true, true, false, false, (N + 7) / 8, 0, (uint16_t*)nullptr);    // one rotation pair per wave
        else SKV_GEMV8(4, false, false, true, false, false, (N + 15) / 16, 0, (uint16_t*)nullptr);
        return hipGetLastError() == hipSuccess ? SKV_OK : SKV_ERR_LAUNCH;
    }
    if (fuse_silu_mul) {
        if (N % 2 || bias) return SKV_ERR_ARG;
        const int I = N / 2;
        const int grid = (I + 7) / 8;  // 4 waves x 2 (gate, up) pairs
        if (norm) SKV_GEMV8(4, true, true, false, false, false, grid, I, (uint16_t*)nullptr);
        else SKV_GEMV8(4, true, false, false, false, false, grid, I, (uint16_t*)nullptr);
    } else {
        const int grid = (N + 15) / 16;
        if (!norm && N <= 8192)    // few output rows (O and down projections): two rows per wave, as the bf16 launch
            SKV_GEMV8(2, false, false, false, false, false, (N + 7) / 8, 0, (uint16_t*)nullptr);
        else if (norm) SKV_GEMV8(4, false, true, false, false, false, grid, 0, (uint16_t*)nullptr);
        else SKV_GEMV8(4, false, false, false, false, false, grid, 0, (uint16_t*)nullptr);
    }
#undef SKV_GEMV8
    return hipGetLastError() == hipSuccess ? SKV_OK : SKV_ERR_LAUNCH;
}

extern "C" int skv_gemv_fp8(const void* W8, const void* scale, const void* x, const void* bias, void* y, int N, int K,
                            int fuse_silu_mul, skv_stream_t stream) {
    return launch_gemv_fp8(W8, scale, x, bias, y, N, K, fuse_silu_mul, nullptr, nullptr, nullptr, 0.f, false, (hipStream_t)stream);
}

extern "C" int skv_norm_gemv_fp8(const void* W8, const void* scale, const void* x, const void* residual, const void* norm_weight,
                                 float eps, void* h_out, const void* bias, void* y, int N, int K, int fuse_silu_mul,
                                 skv_stream_t stream) {
    return launch_gemv_fp8(W8, scale, x, bias, y, N, K, fuse_silu_mul, residual, norm_weight, h_out, eps, true, (hipStream_t)stream);
}

extern "C" int skv_norm_gemv_rangemax_fp8(const void* W8, const void* scale, const void* x, const void* residual,
                                          const void* norm_weight, float eps, void* h_out, const void* bias, void* y, int N, int K,
                                          void* range_max, skv_stream_t stream) {
    if (!range_max) return SKV_ERR_ARG;
    return launch_gemv_fp8(W8, scale, x, bias, y, N, K, 0, residual, norm_weight, h_out, eps, true, (hipStream_t)stream, nullptr,
                           (uint16_t*)range_max);
}

extern "C" int skv_qkv_gemv_rope_update_fp8(const void* Wqkv8, const void* scale, const void* x, const void* residual,
                                            const void* norm_weight, float eps, void* h_out, const void* bias, const void* cos_sin,
                                            const int64_t* pos, const int64_t* row_idx, const void* q_override, void* q_out,
                                            void* k_cache, void* v_cache, int K, int q_heads, int kv_heads, int head_dim,
                                            long long cos_sin_stride, int cos_sin_rows, long long cache_stride_h, int cache_rows,
                                            int rope_mode, skv_stream_t stream) {
    if (!cos_sin || !pos || !row_idx || !q_out || !k_cache || !v_cache || cos_sin_rows < 1 || q_heads < 1 || kv_heads < 1)
        return SKV_ERR_ARG;
    if (head_dim != 128 || (rope_mode != 1 && rope_mode != 2)) return SKV_ERR_UNSUPPORTED;
    QkvEpilogue qe{(const bf16_t*)cos_sin, pos, row_idx, (const bf16_t*)q_override, (bf16_t*)q_out, (bf16_t*)k_cache,
                   (bf16_t*)v_cache, cos_sin_stride, cache_stride_h, q_heads, kv_heads, cache_rows, rope_mode == 2, cos_sin_rows};
    return launch_gemv_fp8(Wqkv8, scale, x, bias, nullptr, (q_heads + 2 * kv_heads) * 128, K, 0, residual, norm_weight, h_out, eps,
                           norm_weight != nullptr, (hipStream_t)stream, &qe);
}

// (the argument checks and the carving of skv_gemv.hip's near_pull_of, restated: that file stays as it is)
static int near_pull_fp8_of(NearPull& np, void* early_state, int blocks, int groups, int n_landmarks, int n_chunks, int early_max,
                            const void* v_host, long long host_block_stride, int pull_parts, int list, int active_lists) {
    if (pull_parts != 1 && pull_parts != 2 && pull_parts != 4) return SKV_ERR_ARG;
    if (list < 0 || list >= SKV_NEAR_LISTS || active_lists < 1 || active_lists > SKV_NEAR_LISTS || list >= active_lists) return SKV_ERR_ARG;
    if (!early_state || !v_host || blocks < 1 || groups < 1 || n_landmarks < 1 || n_chunks < 1 || early_max < 1 || early_max > 128 ||
        (host_block_stride % 8))
        return SKV_ERR_ARG;
    if (n_chunks > (1 << 18)) return SKV_ERR_UNSUPPORTED;      // (the early state's limit, skv_select_chunks_fused)
    const EarlyState es = skv_carve_early(early_state, blocks, groups, n_landmarks, n_chunks, early_max);
    np = skv_near_pull(es, v_host, host_block_stride, blocks, n_chunks, early_max, pull_parts, list, active_lists);
    return SKV_OK;
}

extern "C" int skv_norm_gemv_near_pull_fp8(const void* W8, const void* scale, const void* x, const void* residual,
                                           const void* norm_weight, float eps, void* h_out, void* y, int N, int K, void* early_state,
                                           int blocks, int groups, int n_landmarks, int n_chunks, int early_max, const void* v_host,
                                           long long host_block_stride, int pull_parts, int active_lists, skv_stream_t stream) {
    int rc = gemv_fp8_args(W8, scale, x, y, false, N, K, true, norm_weight);
    if (rc != SKV_OK) return rc;
    NearPull np{};
    rc = near_pull_fp8_of(np, early_state, blocks, groups, n_landmarks, n_chunks, early_max, v_host, host_block_stride, pull_parts, 0,
                          active_lists);
    if (rc != SKV_OK) return rc;
    return launch_gemv_fp8(W8, scale, x, nullptr, y, N, K, 1, residual, norm_weight, h_out, eps, true, (hipStream_t)stream, nullptr,
                           nullptr, &np);
}

extern "C" int skv_gemv_near_pull_fp8(const void* W8, const void* scale, const void* x, const void* bias, void* y, int N, int K,
                                      void* early_state, int blocks, int groups, int n_landmarks, int n_chunks, int early_max,
                                      const void* v_host, long long host_block_stride, int pull_parts, int list, skv_stream_t stream) {
    int rc = gemv_fp8_args(W8, scale, x, y, false, N, K, false, nullptr);
    if (rc != SKV_OK) return rc;
    NearPull np{};
    rc = near_pull_fp8_of(np, early_state, blocks, groups, n_landmarks, n_chunks, early_max, v_host, host_block_stride, pull_parts, list,
                          SKV_NEAR_LISTS);
    if (rc != SKV_OK) return rc;
    return launch_gemv_fp8(W8, scale, x, bias, y, N, K, 0, nullptr, nullptr, nullptr, 0.f, false, (hipStream_t)stream, nullptr, nullptr,
                           &np);
}
