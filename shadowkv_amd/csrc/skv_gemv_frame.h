// The frame the decode GEMV kernels share: skv_gemv_kernel (skv_gemv.hip, bf16 weights), skv_gemv_fp8_kernel (skv_gemv_fp8.hip,
// e4m3 weights + a row scale) and skv_gemv_mxfp4_kernel (skv_gemv_mxfp4.hip, e2m1 nibbles + e8m0 block scales) differ only in how
// they stream and multiply a weight row.  Everything around that stream is stated here once: the near-pull role in front of the
// grid, which rows a wave owns, a row's reduction, the epilogue, and on the host the branch tree that picks a kernel instance and
// the bodies of the extern "C" entries.  The residual add + RMSNorm prologue the kernels call is skv_norm_prologue_4096
// (skv_kvproj.h), near_pull_of is next to skv_near_pull (skv_launch.h).
//
// Template parameters of the kernels: R rows per wave; SILU_PAIR: W = [gate; up], the wave's rows are R / 2 (gate, up)
// pairs and y[i] = bf16(silu(gate_i)) * up_i; NORM: x is the pre-norm hidden state (K == 4096); QKV: W = fused [q; k; v] of
// ONE token (head_dim 128), the wave's rows are R / 2 rotation pairs of one head - NeoX (t, t+64), GLM (2t, 2t+1) - and lane
// 0 rotates and writes q / the cache row (skv_qkv_epilogue); RMAX (lm_head, N % 16 == 0): the workgroup also leaves the
// LARGEST of its 16 outputs as an order-preserving 16-bit key in range_max[block] - the sampler (skv_sample.hip) then finds
// the rows that can hold a top-k logit from N / 16 keys; NEARP: the first np.blocks workgroups do not compute - they stage
// the near misses of this step's selection ahead of the next step (skv_near_pull_role) while the GEMV streams.
#pragma once
#include "skv_common.h"
#include "skv_early.h"
#include "skv_kvproj.h"

// NEARP: true for a workgroup of the pull role (it has done its work: the kernel returns); the GEMV's own workgroups follow
// the role's in the grid and get their index in bx.
template <bool NEARP>
__device__ __forceinline__ bool skv_gemv_near_pull_block(const NearPull& np, int& bx) {
    if constexpr (NEARP) {
        if (bx < np.blocks) {
            __shared__ int s_near[6 * 64 + 8];
            skv_near_pull_role(np, bx, threadIdx.x, s_near);
            return true;
        }
        bx -= np.blocks;
    }
    return false;
}

// The R weight rows of a wave whose first output unit (an output row, or a (gate, up) pair) is unit0 = (bx * 4 + wave) *
// (SILU_PAIR ? R / 2 : R).
template <int R, bool SILU_PAIR, bool QKV>
__device__ __forceinline__ void skv_gemv_wave_rows(int (&rows)[R], int unit0, int I, bool glm) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (SILU_PAIR) rows[r] = (r & 1) ? I + unit0 + r / 2 : unit0 + r / 2;  // (gate, up) pairs
        else if (QKV && !glm) {
            // unit0 = R * wave index; a wave owns R/2 rotation pairs (t, t+64) of one head: 128/R waves per head,
            // rows t0, t0+64, t0+1, t0+65, ...
            const int w = unit0 / R, head = w / (128 / R), t0 = (R / 2) * (w % (128 / R));
            rows[r] = head * 128 + t0 + (r >> 1) + ((r & 1) ? 64 : 0);
        } else rows[r] = unit0 + r;
    }
}
// the row to stream for rows[r]: a row past the end of a ragged last wave (limit = units of the launch) is clamped - computed
// and discarded
template <int R, bool SILU_PAIR>
__device__ __forceinline__ int skv_gemv_stream_row(const int (&rows)[R], int r, int unit0, int limit, int I) {
    int row = rows[r];
    const int base_unit = SILU_PAIR ? unit0 + r / 2 : unit0 + r;
    if (base_unit >= limit) row = SILU_PAIR ? ((r & 1) ? I : 0) : 0;
    return row;
}

// a row's dot product from the wave's 64 x 4 packed partial sums: 8 -> 1 per lane, then the wave tree
__device__ __forceinline__ float skv_gemv_row_total(const f32x2 (&acc)[4]) {
    const float s = ((acc[0].x + acc[0].y) + (acc[1].x + acc[1].y)) + ((acc[2].x + acc[2].y) + (acc[3].x + acc[3].y));
    return wave_tree_sum(s);
}

// The operands of the epilogue: skv_gemv_epilogue_fetch requests them - the bias values of the wave's rows (the down
// projection of the call-order path carries the residual there), or what skv_qkv_epilogue_fetch names - and belongs IN FRONT
// of the weight stream (QKV: skv_gemv_epilogue_fetch_cs behind the first weight request); skv_gemv_epilogue then holds
// arithmetic and stores only.  The addresses are the wave's and the loads unconditional (skv_kvproj.h says why); `spare` is a
// readable bf16 for the values a launch does not have.  (A launch without the QKV epilogue uses the bias field alone.)
template <int R, bool SILU_PAIR, bool QKV>
__device__ __forceinline__ QkvOperands<R> skv_gemv_epilogue_fetch(const int (&rows)[R], int unit0, int N, const bf16_t* __restrict__ bias,
                                                                  const QkvEpilogue& qe, const bf16_t* spare) {
    if constexpr (QKV) return skv_qkv_epilogue_fetch<R>(qe, bias, rows, unit0, spare);
    QkvOperands<R> op{};
    if constexpr (!SILU_PAIR) {
#pragma unroll
        for (int r = 0; r < R; ++r) op.bias[r] = *(bias ? bias + (unit0 + r < N ? unit0 + r : 0) : spare);
    }
    return op;
}
template <int R, bool QKV>
__device__ __forceinline__ void skv_gemv_epilogue_fetch_cs(QkvOperands<R>& op, const QkvEpilogue& qe, const int (&rows)[R], int unit0) {
    if constexpr (QKV) skv_qkv_epilogue_fetch_cs<R>(op, qe, rows, unit0);
}

// tot[R] -> the launch's outputs (lane 0 of every wave writes)
template <int R, bool SILU_PAIR, bool QKV, bool RMAX>
__device__ __forceinline__ void skv_gemv_epilogue(const int (&rows)[R], const float (&tot)[R], int unit0, int bx, int tid, int N,
                                                  int I, bool has_bias, const QkvOperands<R>& op, bf16_t* __restrict__ y,
                                                  const QkvEpilogue& qe, uint16_t* __restrict__ range_max) {
    const int lane = tid & 63, wave = tid >> 6;
    if constexpr (QKV) {
        if (lane == 0 && unit0 < N) skv_qkv_epilogue_apply<R>(qe, has_bias, op, rows, tot, unit0);
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
                const bf16_t o = f2bf(has_bias ? bfr(tot[r]) + bf2f(op.bias[r]) : tot[r]);
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
// fetch and apply back to back, for a kernel that leaves the epilogue's loads behind its reduction (a wave past the end of a
// QKV launch neither loads nor stores)
template <int R, bool SILU_PAIR, bool QKV, bool RMAX>
__device__ __forceinline__ void skv_gemv_epilogue(const int (&rows)[R], const float (&tot)[R], int unit0, int bx, int tid, int N,
                                                  int I, const bf16_t* __restrict__ bias, bf16_t* __restrict__ y,
                                                  const QkvEpilogue& qe, uint16_t* __restrict__ range_max, const bf16_t* spare) {
    QkvOperands<R> op{};
    if (!QKV || unit0 < N) {
        op = skv_gemv_epilogue_fetch<R, SILU_PAIR, QKV>(rows, unit0, N, bias, qe, spare);
        skv_gemv_epilogue_fetch_cs<R, QKV>(op, qe, rows, unit0);
    }
    skv_gemv_epilogue<R, SILU_PAIR, QKV, RMAX>(rows, tot, unit0, bx, tid, N, I, bias != nullptr, op, y, qe, range_max);
}

// Host.  A format is a struct L: GemvArgs (the arguments every format's kernel takes) plus its weight pointer - the scaled
// formats: and the scale pointer behind it - built by L(args, W, scale), and
//   K_STEP, K_MIN         K must be a multiple of the one and at least the other
//   SCALED                a scale pointer follows W in every entry (bf16: absent - its forwarders pass nullptr, nothing reads it)
//   Q_ROWS_ALONE          the format has the q-only launch (N = Hq * 128)
//   launch<R, SILU, NORM, QKV, RMAX, NEARP>(grid, I, range_max, near)    starts the format's kernel
// and the two places where the answers of bf16 and of the scaled formats to a refused call differ (tests/test_gemv_refusals_cpu.py
// holds every entry to them):
//   NEAR_ROLE_ARGS_FIRST  a near-pull entry checks the role's arguments (near_pull_of) before the GEMV's own: a call that is wrong
//                         in both gets the role's code from bf16 and the GEMV's from FP8 / MXFP4
//   QKV_REFUSES_NO_HEADS  the QKV entry refuses q_heads < 1 || kv_heads < 1 itself (SKV_ERR_ARG); bf16 has no such check there and
//                         answers with whatever the GEMV's checks say about N = (q_heads + 2 * kv_heads) * 128 and K
struct GemvArgs {
    const bf16_t *x, *bias;
    bf16_t* y;
    int N, K;
    const bf16_t *residual, *w_norm;
    bf16_t* h_out;
    float eps;
    QkvEpilogue qe;
    hipStream_t st;
};

// the kernel instance and the grid of a launch, for every format
template <class L>
static int skv_gemv_dispatch(const L& l, int N, bool bias, bool fuse_silu_mul, bool norm, const QkvEpilogue* qkv, uint16_t* range_max,
                             const NearPull* near) {
    const NearPull none{};
    if (near) {          // a launch of a layer's dense tail with the near-miss pull role in front of its grid
        if (qkv || range_max || near->blocks < 1 || near->E + SKV_NEAR_SLOTS > 32767) return SKV_ERR_UNSUPPORTED;
        if (norm && fuse_silu_mul && !(N % 2) && !bias)                      // gate/up: list 0
            l.template launch<4, true, true, false, false, true>(near->blocks + (N / 2 + 7) / 8, N / 2, nullptr, *near);
        else if (!norm && !fuse_silu_mul && N <= 8192)                       // down projection (two rows per wave): list 1
            l.template launch<2, false, false, false, false, true>(near->blocks + (N + 7) / 8, 0, nullptr, *near);
        else return SKV_ERR_UNSUPPORTED;
    } else if (range_max) {     // the lm_head with the sampler's range keys: norm prologue, whole workgroups of 16 rows
        if (!norm || qkv || fuse_silu_mul || N % 16) return SKV_ERR_UNSUPPORTED;
        l.template launch<4, false, true, false, true, false>(N / 16, 0, range_max, none);
    } else if (qkv) {
        if (fuse_silu_mul || (N != (qkv->Hq + 2 * qkv->Hkv) * 128 && !(L::Q_ROWS_ALONE && N == qkv->Hq * 128))) return SKV_ERR_ARG;
        // norm: one rotation pair per wave: 3,072 waves for N = 6144 (two pairs per wave: 200.4 -> 202.3 tok/s)
        if (norm) l.template launch<2, false, true, true, false, false>((N + 7) / 8, 0, nullptr, none);
        else l.template launch<4, false, false, true, false, false>((N + 15) / 16, 0, nullptr, none);
    } else if (fuse_silu_mul) {
        if (N % 2 || bias) return SKV_ERR_ARG;
        const int I = N / 2, grid = (I + 7) / 8;     // 4 waves x 2 (gate, up) pairs
        if (norm) l.template launch<4, true, true, false, false, false>(grid, I, nullptr, none);
        else l.template launch<4, true, false, false, false, false>(grid, I, nullptr, none);
    } else if (!norm && N <= 8192) {
        // few output rows (O and down projections: N = 4096 -> 256 blocks = 1 per CU with 4 rows per wave): 2 rows
        // per wave doubles the waves and the bytes in flight per CU (measured 198.3 -> 200.7 tok/s; 1 row: 199.3)
        l.template launch<2, false, false, false, false, false>((N + 7) / 8, 0, nullptr, none);
    } else if (norm) l.template launch<4, false, true, false, false, false>((N + 15) / 16, 0, nullptr, none);
    else l.template launch<4, false, false, false, false, false>((N + 15) / 16, 0, nullptr, none);
    return hipGetLastError() == hipSuccess ? SKV_OK : SKV_ERR_LAUNCH;
}

// every check of the GEMV's own arguments; host only, before any HIP call
template <class L>
static int skv_gemv_check(const void* W, const void* scale, const void* x, const void* y, bool qkv, int N, int K, bool norm,
                          const void* w_norm) {
    if (!W || (L::SCALED && !scale) || !x || (!y && !qkv) || N < 1) return SKV_ERR_ARG;
    if (K % L::K_STEP || K < L::K_MIN) return SKV_ERR_UNSUPPORTED;
    if (norm && (K != 4096 || !w_norm)) return SKV_ERR_UNSUPPORTED;
    return SKV_OK;
}

// check, build the format's launcher, dispatch
template <class L>
static int skv_gemv_launch(const void* W, const void* scale, const void* x, const void* bias, void* y, int N, int K, int fuse_silu_mul,
                           const void* residual, const void* w_norm, void* h_out, float eps, bool norm, skv_stream_t stream,
                           const QkvEpilogue* qkv = nullptr, uint16_t* range_max = nullptr, const NearPull* near = nullptr) {
    const int rc = skv_gemv_check<L>(W, scale, x, y, qkv != nullptr, N, K, norm, w_norm);
    if (rc != SKV_OK) return rc;
    const L l(GemvArgs{(const bf16_t*)x, (const bf16_t*)bias, (bf16_t*)y, N, K, (const bf16_t*)residual, (const bf16_t*)w_norm,
                       (bf16_t*)h_out, eps, qkv ? *qkv : QkvEpilogue{}, (hipStream_t)stream},
              W, scale);
    return skv_gemv_dispatch(l, N, bias != nullptr, fuse_silu_mul != 0, norm, qkv, range_max, near);
}

// The six kinds of entry; a format's extern "C" names forward to them.
template <class L>
static int skv_gemv_entry(const void* W, const void* scale, const void* x, const void* bias, void* y, int N, int K, int fuse_silu_mul,
                          skv_stream_t stream) {
    return skv_gemv_launch<L>(W, scale, x, bias, y, N, K, fuse_silu_mul, nullptr, nullptr, nullptr, 0.f, false, stream);
}

template <class L>
static int skv_norm_gemv_entry(const void* W, const void* scale, const void* x, const void* residual, const void* norm_weight, float eps,
                               void* h_out, const void* bias, void* y, int N, int K, int fuse_silu_mul, skv_stream_t stream) {
    return skv_gemv_launch<L>(W, scale, x, bias, y, N, K, fuse_silu_mul, residual, norm_weight, h_out, eps, true, stream);
}

template <class L>
static int skv_norm_gemv_rangemax_entry(const void* W, const void* scale, const void* x, const void* residual, const void* norm_weight,
                                        float eps, void* h_out, const void* bias, void* y, int N, int K, void* range_max,
                                        skv_stream_t stream) {
    if (!range_max) return SKV_ERR_ARG;
    return skv_gemv_launch<L>(W, scale, x, bias, y, N, K, 0, residual, norm_weight, h_out, eps, true, stream, nullptr, (uint16_t*)range_max);
}

template <class L>
static int skv_qkv_gemv_rope_update_entry(const void* Wqkv, const void* scale, const void* x, const void* residual,
                                          const void* norm_weight, float eps, void* h_out, const void* bias, const void* cos_sin,
                                          const int64_t* pos, const int64_t* row_idx, const void* q_override, void* q_out, void* k_cache,
                                          void* v_cache, int K, int q_heads, int kv_heads, int head_dim, long long cos_sin_stride,
                                          int cos_sin_rows, long long cache_stride_h, int cache_rows, int rope_mode, skv_stream_t stream) {
    if (!cos_sin || !pos || !row_idx || !q_out || !k_cache || !v_cache || cos_sin_rows < 1 ||
        (L::QKV_REFUSES_NO_HEADS && (q_heads < 1 || kv_heads < 1)))
        return SKV_ERR_ARG;
    if (head_dim != 128 || (rope_mode != 1 && rope_mode != 2)) return SKV_ERR_UNSUPPORTED;
    QkvEpilogue qe{(const bf16_t*)cos_sin, pos, row_idx, (const bf16_t*)q_override, (bf16_t*)q_out, (bf16_t*)k_cache,
                   (bf16_t*)v_cache, cos_sin_stride, cache_stride_h, q_heads, kv_heads, cache_rows, rope_mode == 2, cos_sin_rows};
    return skv_gemv_launch<L>(Wqkv, scale, x, bias, nullptr, (q_heads + 2 * kv_heads) * 128, K, 0, residual, norm_weight, h_out, eps,
                              norm_weight != nullptr, stream, &qe);
}

// The near-miss pull role in front of the grid of the gate/up launch (norm, fused SiLU; list 0 of `active_lists`) ...
template <class L>
static int skv_norm_gemv_near_pull_entry(const void* W, const void* scale, const void* x, const void* residual, const void* norm_weight,
                                         float eps, void* h_out, void* y, int N, int K, void* early_state, int blocks, int groups,
                                         int n_landmarks, int n_chunks, int early_max, const void* v_host, long long host_block_stride,
                                         int pull_parts, int active_lists, skv_stream_t stream) {
    NearPull np{};
    int rc = L::NEAR_ROLE_ARGS_FIRST ? SKV_OK : skv_gemv_check<L>(W, scale, x, y, false, N, K, true, norm_weight);
    if (rc == SKV_OK)
        rc = near_pull_of(np, early_state, blocks, groups, n_landmarks, n_chunks, early_max, v_host, host_block_stride, pull_parts, 0,
                          active_lists);
    if (rc != SKV_OK) return rc;
    return skv_gemv_launch<L>(W, scale, x, nullptr, y, N, K, 1, residual, norm_weight, h_out, eps, true, stream, nullptr, nullptr, &np);
}

// ... and of the down projection (N <= 8192), with near-miss list `list` (1: ranks S + 65 .. S + 128)
template <class L>
static int skv_gemv_near_pull_entry(const void* W, const void* scale, const void* x, const void* bias, void* y, int N, int K,
                                    void* early_state, int blocks, int groups, int n_landmarks, int n_chunks, int early_max,
                                    const void* v_host, long long host_block_stride, int pull_parts, int list, skv_stream_t stream) {
    NearPull np{};
    int rc = L::NEAR_ROLE_ARGS_FIRST ? SKV_OK : skv_gemv_check<L>(W, scale, x, y, false, N, K, false, nullptr);
    if (rc == SKV_OK)
        rc = near_pull_of(np, early_state, blocks, groups, n_landmarks, n_chunks, early_max, v_host, host_block_stride, pull_parts, list,
                          SKV_NEAR_LISTS);
    if (rc != SKV_OK) return rc;
    return skv_gemv_launch<L>(W, scale, x, bias, y, N, K, 0, nullptr, nullptr, nullptr, 0.f, false, stream, nullptr, nullptr, &np);
}
