// MInference "vertical + slash" sparse prefill (the reference's minference_prefill_kernel, models/tensor_op.py:68-117): the
// per-head index estimate from the last 64 queries, and the sparse causal attention over the kept columns and diagonals.
// bf16 in / out, f32 accumulation, head_dim 128, kv_len == q_len == L.  Contract: DESIGN.md section 9.
//
// Estimate (two launches, no atomics: every output element is written by one thread, in a fixed summation order):
//   m = min(64, L) query rows r = L - m .. L - 1; A[r][j] = q_r . k_j (no 1 / sqrt(D)), -inf for j > r; P = softmax_j(A), f32.
//   c[j] = sum_r P[r][j] (+inf for j < 30);  d[s] = sum_r P[r][r - s] (+inf for s < 100).
//   launch 1 (vs_rowstat): workgroup = (sequence, query head, 2,048-key chunk): per query row the chunk's max and sum of
//     exp, online over 64-key tiles, in registers; the two key halves of a tile meet once through LDS.
//   launch 2 (vs_scores): workgroup = (sequence, query head, 64-index tile t): folds the chunk partials in chunk order, then
//     the P tile of keys 64 t .. + 63 (column sums -> c) and of the 128 keys that offsets 64 t .. + 63 touch (diagonal
//     sums -> d), each through LDS.
//   Score tiles: 4 waves, wave w = (query half w & 1, key half w >> 1); S^T = K.Q^T on v_mfma_f32_32x32x16_bf16 with the Q
//   fragments in registers (the layout of skv_flash_tile.h) and K read straight from global memory.
//
// Sparse attention (two launches):
//   launch 1 (vs_bitmap): one bit per (sequence, query head, slash offset in [0, L)), so the attention can ask "does a
//     window of this block cover column v" with at most five word reads; zeroed and set by one workgroup per head.
//   launch 2 (vs_attn): workgroup = 64 query rows (one mask block b, e = 64 (b + 1)) of one (sequence, query head), 2 waves
//     of 32 rows; the tile body (Q / K / V layouts, online softmax, P.V) is skv_flash_tile.h, with CAN_BE_EMPTY = true: a
//     row may attend no key of a tile, or none at all (it then writes zeros).  Key tiles of 64 come from
//       - the slash windows of the block, merged on the fly from the head's ascending offset list into contiguous ranges
//         (windows with ascending s have descending ends) and cut from the top into tiles [max(lo, top - 64), top);
//       - then 64 consecutive entries of the head's ascending vertical list below min(e, L), minus duplicates and minus
//         columns a window already covered (the bitmap), gathered row by row.
//     Each tile's key ids sit in LDS (INT_MAX = not attended); a row's mask is key id <= row.  Full slash tiles below a
//     wave's first row skip the mask.  The next tile's rows are loaded under the current tile's MFMAs.  The grid runs the
//     last (heaviest) blocks first.
#include "../../include/shadowkv_hip.h"
#include "skv_flash_tile.h"

#include <limits.h>

typedef __attribute__((ext_vector_type(4))) int vs_i32x4;

#define VS_LASTQ 64          // queries of the estimate
#define VS_CHUNK 2048        // keys per row-statistics workgroup
#define VS_PP (2 * FT_KB + 4) // P LDS row pitch, f32
#define VS_SINKS 30
#define VS_LOCAL 100

// Q fragments of query row L - m + qrow (zero when qrow >= m)
__device__ __forceinline__ void vs_load_q(ft_bf16x8 (&qf)[8], const bf16_t* qh, long long qss, int L, int m, int qrow, int h) {
    const bool ok = qrow < m;
    ft_load_q(qf, qh + (long long)(L - m + (ok ? qrow : 0)) * qss, ok, h);
}

// S^T[key][query] for keys key0 + crow(i, h) (K rows read from global, zero outside [0, L)): 32 keys x 32 queries
__device__ __forceinline__ ft_f32x16 vs_scores32(const ft_bf16x8 (&qf)[8], const bf16_t* kh, long long kss, int L, int key0,
                                                 int r, int h) {
    const int key = key0 + r;
    const bool ok = key >= 0 && key < L;
    const bf16_t* kp = kh + (long long)(ok ? key : 0) * kss + 8 * h;
    u32x4 kw[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        kw[s] = *reinterpret_cast<const u32x4*>(kp + 16 * s);
        if (!ok) kw[s] = (u32x4){0u, 0u, 0u, 0u};
    }
    ft_f32x16 sc = (ft_f32x16){};
#pragma unroll
    for (int s = 0; s < 8; ++s)
        sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(ft_bf16x8, kw[s]), qf[s], sc, 0, 0, 0);
    return sc;
}

// ---------------------------------------------------------------------------------------------------- estimate, launch 1
__global__ __launch_bounds__(256) void vs_rowstat_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                         float* __restrict__ part, int Hq, int G, int L, long long qsb,
                                                         long long qsh, long long qss, long long ksb, long long ksh,
                                                         long long kss, int n_chunk) {
    __shared__ float s_m[2][VS_LASTQ], s_l[2][VS_LASTQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5, qhalf = wave & 1, khalf = wave >> 1;
    const int chunk = (int)(blockIdx.x % (unsigned)n_chunk), bh = (int)(blockIdx.x / (unsigned)n_chunk);
    const int b = bh / Hq, hq = bh - b * Hq;
    const int m = min(VS_LASTQ, L);
    const int qrow = 32 * qhalf + r, rabs = L - m + qrow;
    ft_bf16x8 qf[8];
    vs_load_q(qf, q + (long long)b * qsb + (long long)hq * qsh, qss, L, m, qrow, h);
    const bf16_t* kh = k + (long long)b * ksb + (long long)(hq / G) * ksh;
    const float LOG2E = 1.44269504088896341f;
    float mx = -INFINITY, sm = 0.f;
    const int k_end = min(L, (chunk + 1) * VS_CHUNK);
    for (int key0 = chunk * VS_CHUNK; key0 < k_end; key0 += FT_KB) {
        const int kb = key0 + 32 * khalf;
        ft_f32x16 sc = vs_scores32(qf, kh, kss, L, kb, r, h);
        float mt = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = kb + ft_crow(i, h);
            const float x = (key <= rabs && key < L) ? sc[i] * LOG2E : -INFINITY;
            sc[i] = x;
            mt = fmaxf(mt, x);
        }
        const float mn = fmaxf(mx, mt);
        if (mn == -INFINITY) continue;
        float rs = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) rs += __builtin_amdgcn_exp2f(sc[i] - mn);
        sm = sm * __builtin_amdgcn_exp2f(mx - mn) + rs;
        mx = mn;
    }
    // lanes l and l ^ 32 hold the same query; then the two key halves
    {
        const float mo = __shfl_xor(mx, 32), so = __shfl_xor(sm, 32);
        const float mn = fmaxf(mx, mo);
        if (mn != -INFINITY) {
            sm = (h == 0) ? sm * __builtin_amdgcn_exp2f(mx - mn) + so * __builtin_amdgcn_exp2f(mo - mn)
                          : so * __builtin_amdgcn_exp2f(mo - mn) + sm * __builtin_amdgcn_exp2f(mx - mn);
            mx = mn;
        }
    }
    if (h == 0) {
        s_m[khalf][qrow] = mx;
        s_l[khalf][qrow] = sm;
    }
    __syncthreads();
    if (tid < VS_LASTQ) {
        const float m0 = s_m[0][tid], m1 = s_m[1][tid];
        const float mn = fmaxf(m0, m1);
        float l = 0.f;
        if (mn != -INFINITY) l = s_l[0][tid] * __builtin_amdgcn_exp2f(m0 - mn) + s_l[1][tid] * __builtin_amdgcn_exp2f(m1 - mn);
        float* pp = part + ((long long)bh * n_chunk + chunk) * (2 * VS_LASTQ);
        pp[tid] = mn;
        pp[VS_LASTQ + tid] = l;
    }
}

// ---------------------------------------------------------------------------------------------------- estimate, launch 2
__global__ __launch_bounds__(256) void vs_scores_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                        const float* __restrict__ part, float* __restrict__ col,
                                                        float* __restrict__ diag, int Hq, int G, int L, long long qsb,
                                                        long long qsh, long long qss, long long ksb, long long ksh,
                                                        long long kss, int n_chunk, int n_tile) {
    __shared__ float s_p[VS_LASTQ * VS_PP];
    __shared__ float s_mx[VS_LASTQ], s_inv[VS_LASTQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5, qhalf = wave & 1, khalf = wave >> 1;
    const int t = (int)(blockIdx.x % (unsigned)n_tile), bh = (int)(blockIdx.x / (unsigned)n_tile);
    const int b = bh / Hq, hq = bh - b * Hq;
    const int m = min(VS_LASTQ, L);
    const int qrow = 32 * qhalf + r, rabs = L - m + qrow;
    const float LOG2E = 1.44269504088896341f;

    if (tid < VS_LASTQ) {                      // fold the chunk partials of row tid, in chunk order
        const float* pp = part + (long long)bh * n_chunk * (2 * VS_LASTQ);
        float mx = -INFINITY, l = 0.f;
        for (int c = 0; c < n_chunk; ++c) {
            const float mc = pp[c * 2 * VS_LASTQ + tid], lc = pp[c * 2 * VS_LASTQ + VS_LASTQ + tid];
            const float mn = fmaxf(mx, mc);
            if (mn == -INFINITY) continue;
            l = l * __builtin_amdgcn_exp2f(mx - mn) + lc * __builtin_amdgcn_exp2f(mc - mn);
            mx = mn;
        }
        s_mx[tid] = mx;
        s_inv[tid] = l > 0.f ? 1.0f / l : 0.f;
    }
    ft_bf16x8 qf[8];
    vs_load_q(qf, q + (long long)b * qsb + (long long)hq * qsh, qss, L, m, qrow, h);
    const bf16_t* kh = k + (long long)b * ksb + (long long)(hq / G) * ksh;
    __syncthreads();
    const float rmx = s_mx[qrow], rinv = s_inv[qrow];

    // P[qrow][c0 + key offset] into s_p[qrow][slot0 + key offset] for the 64 keys key0 .. key0 + 63
    auto p_tile = [&](int key0, int slot0) {
        const int kb = key0 + 32 * khalf;
        const ft_f32x16 sc = vs_scores32(qf, kh, kss, L, kb, r, h);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = kb + ft_crow(i, h);
            const bool ok = qrow < m && key >= 0 && key <= rabs && key < L;
            s_p[qrow * VS_PP + slot0 + 32 * khalf + ft_crow(i, h)] = ok ? __builtin_amdgcn_exp2f(sc[i] * LOG2E - rmx) * rinv : 0.f;
        }
    };

    const int s0 = FT_KB * t;
    p_tile(s0, 0);                              // columns 64 t .. + 63
    __syncthreads();
    if (tid < FT_KB && s0 + tid < L) {
        float acc = 0.f;
        for (int i = 0; i < VS_LASTQ; ++i) acc += s_p[i * VS_PP + tid];
        col[(long long)bh * L + s0 + tid] = (s0 + tid < VS_SINKS) ? INFINITY : acc;
    }
    __syncthreads();
    // offsets s0 + si: row qrow meets key L - m + qrow - s0 - si = base + 64 + qrow - si, base = L - m - s0 - 64
    const int base = L - m - s0 - FT_KB;
    p_tile(base, 0);
    p_tile(base + FT_KB, FT_KB);
    __syncthreads();
    if (tid < FT_KB && s0 + tid < L) {
        float acc = 0.f;
        for (int i = 0; i < VS_LASTQ; ++i) acc += s_p[i * VS_PP + FT_KB + i - tid];
        diag[(long long)bh * L + s0 + tid] = (s0 + tid < VS_LOCAL) ? INFINITY : acc;
    }
}

// -------------------------------------------------------------------------------------------------- attention, launch 1
__global__ __launch_bounds__(256) void vs_bitmap_kernel(const int* __restrict__ slash, uint32_t* __restrict__ bits, int L,
                                                        int n_slash, int words) {
    const int bh = blockIdx.x;
    uint32_t* bw = bits + (long long)bh * words;
    for (int w = threadIdx.x; w < words; w += 256) bw[w] = 0u;
    __threadfence_block();
    __syncthreads();
    const int* sl = slash + (long long)bh * n_slash;
    for (int i = threadIdx.x; i < n_slash; i += 256) {
        const int s = sl[i];
        if (s >= 0 && s < L) atomicOr(&bw[s >> 5], 1u << (s & 31));
    }
}

// any bit of [lo, hi] set (lo <= hi, both in [0, L))
__device__ __forceinline__ bool vs_any_bit(const uint32_t* bw, int lo, int hi) {
    for (int w = lo >> 5; w <= (hi >> 5); ++w) {
        uint32_t x = bw[w];
        if (w == (lo >> 5)) x &= ~0u << (lo & 31);
        if (w == (hi >> 5)) x &= ~0u >> (31 - (hi & 31));
        if (x) return true;
    }
    return false;
}

// -------------------------------------------------------------------------------------------------- attention, launch 2
__global__ __launch_bounds__(128) void vs_attn_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, bf16_t* __restrict__ out,
    const int* __restrict__ vert, const int* __restrict__ slash, const uint32_t* __restrict__ bits, int Hq, int G, int L,
    int n_vert, int n_slash, int words, long long qsb, long long qsh, long long qss, long long ksb, long long ksh,
    long long kss, long long vsb, long long vsh, long long vss, float scale_log2, int n_blk) {
    __shared__ __attribute__((aligned(16))) bf16_t s_k[FT_KB * FT_KP];
    __shared__ __attribute__((aligned(16))) bf16_t s_vt[FT_D * FT_VP];
    __shared__ __attribute__((aligned(16))) int s_kid[FT_KB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nbh = (int)(gridDim.x / (unsigned)n_blk);
    const int bh = (int)(blockIdx.x % (unsigned)nbh);
    const int blk = n_blk - 1 - (int)(blockIdx.x / (unsigned)nbh);     // last (heaviest) block first
    const int b = bh / Hq, hq = bh - b * Hq, hk = hq / G;
    const int e = FT_KB * (blk + 1);
    const int lim = min(e, L);                                         // list entries >= lim do nothing for this block
    const int qw = FT_KB * blk + 32 * wave, qi = qw + r;
    const bool row_ok = qi < L, wave_on = qw < L;
    const int wave_hi = min(qw + 31, L - 1);

    ft_bf16x8 qf[8];
    ft_load_q(qf, q + (long long)b * qsb + (long long)hq * qsh + (long long)min(qi, L - 1) * qss, row_ok, h);
    const bf16_t* kb = k + (long long)b * ksb + (long long)hk * ksh;
    const bf16_t* vb = v + (long long)b * vsb + (long long)hk * vsh;
    const int* sl = slash + (long long)bh * n_slash;
    const int* vl = vert + (long long)bh * n_vert;
    const uint32_t* bw = bits + (long long)bh * words;

    // ---- tile source (uniform across the workgroup): slash ranges from the top, then vertical runs
    int sp = 0;
    while (sp < n_slash && sl[sp] < 0) ++sp;                          // negative offsets do nothing
    int top = e, cov = e;                                              // keys [cov, top) still due; >= top emitted
    int vp = 0;                                                        // next vertical entry
    // next tile: kind 0 = none, 1 = keys [start, start + cnt), 2 = vertical entries start .. start + 63
    auto next_tile = [&](int& kind, int& start, int& cnt) {
        for (;;) {
            // absorb the next windows while they touch what is due or emitted and a full tile is not yet due
            while (sp < n_slash && cov > top - FT_KB) {
                const int s = sl[sp];
                if (s >= lim) { sp = n_slash; break; }
                const int hi = max(e - s, FT_KB);
                if (hi < cov) break;                                   // a gap: the window starts a new range
                cov = min(cov, hi - FT_KB);
                ++sp;
            }
            if (cov < top) {
                start = max(cov, top - FT_KB);
                cnt = top - start;
                top = start;
                kind = 1;
                return;
            }
            if (sp < n_slash) {                                        // a new range below everything emitted
                const int s = sl[sp];
                if (s < lim) {
                    top = max(e - s, FT_KB);
                    cov = top - FT_KB;
                    ++sp;
                    continue;
                }
                sp = n_slash;
            }
            if (vp < n_vert && vl[vp] < lim) {
                kind = 2;
                start = vp;
                cnt = 0;
                vp += FT_KB;
                return;
            }
            kind = 0;
            return;
        }
    };

    u32x4 kr[4][2], vr[4][2];
    int kid_next = INT_MAX;                                            // key id of row tid of the next tile (tid < 64)
    auto tile_key = [&](int kind, int start, int cnt, int row) -> int {
        if (kind == 1) return row < cnt ? start + row : INT_MAX;
        const int i = start + row;
        if (i >= n_vert) return INT_MAX;
        const int x = vl[i];
        return (x >= 0 && x < lim) ? x : INT_MAX;
    };
    auto load_tile = [&](int kind, int start, int cnt) {
        ft_load_tile<128>(kr, vr, kb, vb, kss, vss, L, tid, [&](int row) { return tile_key(kind, start, cnt, row); });
        if (tid < FT_KB) {
            int key = tile_key(kind, start, cnt, tid);
            if (kind == 2 && key != INT_MAX) {
                // a duplicate of the previous entry, or a column some window of this block covers, is not gathered again
                const int i = start + tid;
                if (i > 0 && vl[i - 1] == key) key = INT_MAX;
                else {
                    const int lo = max(0, e - key - FT_KB);
                    const int hi = min(L - 1, key < FT_KB ? e - 1 : e - key - 1);
                    if (lo <= hi && vs_any_bit(bw, lo, hi)) key = INT_MAX;
                }
            }
            kid_next = key;
        }
    };
    auto store_tile = [&]() {
        ft_store_tile<128>(s_k, s_vt, kr, vr, tid);
        if (tid < FT_KB) s_kid[tid] = kid_next;
    };

    ft_f32x16 o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = (ft_f32x16){};
    float m = -INFINITY, l = 0.f;

    int kind, start, cnt;
    next_tile(kind, start, cnt);
    if (kind != 0) load_tile(kind, start, cnt);
    while (kind != 0) {
        const int cur_kind = kind, cur_start = start, cur_cnt = cnt;
        __syncthreads();                       // every wave is done reading the previous tile
        store_tile();
        __syncthreads();
        next_tile(kind, start, cnt);
        if (kind != 0) load_tile(kind, start, cnt);   // in flight under this tile's MFMAs
        // smallest key of the tile: a wave whose rows all lie above it has nothing to do
        const int tmin = cur_kind == 1 ? cur_start : vl[cur_start];
        if (!wave_on || tmin > wave_hi) continue;

        ft_f32x16 sc[2];
        ft_scores_from_lds(sc, s_k, qf, r, h);
        float mt = -INFINITY;
        if (cur_kind == 1 && cur_cnt == FT_KB && cur_start + FT_KB - 1 <= qw) {   // full window tile below every row
            mt = ft_scale_unmasked(sc, scale_log2);
        } else {
#pragma unroll
            for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const vs_i32x4 id = *reinterpret_cast<const vs_i32x4*>(&s_kid[32 * kb2 + 8 * g + 4 * h]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = 4 * g + j;      // ft_crow(i, h) = 8 g + 4 h + j
                        const float x = id[j] <= qi ? sc[kb2][i] * scale_log2 : -INFINITY;
                        sc[kb2][i] = x;
                        mt = fmaxf(mt, x);
                    }
                }
        }
        ft_softmax_pv<true>(sc, mt, m, l, o, s_vt, r, h);
    }

    if (!row_ok) return;
    ft_write_out<true>(o, l, out + (((long long)b * L + qi) * Hq + hq) * FT_D, h);
}

// -------------------------------------------------------------------------------------------------------------- host
extern "C" long long skv_vs_estimate_workspace_bytes(int batch_size, int q_heads, int q_len) {
    if (batch_size < 1 || q_heads < 1 || q_len < 1) return 0;
    return (long long)batch_size * q_heads * ((q_len + VS_CHUNK - 1) / VS_CHUNK) * 2 * VS_LASTQ * (long long)sizeof(float);
}

extern "C" long long skv_vs_attention_workspace_bytes(int batch_size, int q_heads, int q_len) {
    if (batch_size < 1 || q_heads < 1 || q_len < 1) return 0;
    return (long long)batch_size * q_heads * ((q_len + 31) / 32) * (long long)sizeof(uint32_t);
}

extern "C" int skv_vs_estimate(const void* q, const void* k, void* col_score, void* diag_score, void* workspace,
                               int batch_size, int q_heads, int kv_heads, int q_len, int kv_len, int head_dim,
                               long long q_stride_b, long long q_stride_h, long long q_stride_s, long long k_stride_b,
                               long long k_stride_h, long long k_stride_s, skv_stream_t stream) {
    const void* const ptrs[2] = {q, k};
    const long long strides[6] = {q_stride_b, q_stride_h, q_stride_s, k_stride_b, k_stride_h, k_stride_s};
    if (!col_score || !diag_score || !workspace) return SKV_ERR_ARG;
    const int rc = ft_check_attn_args(ptrs, 2, batch_size, q_heads, kv_heads, q_len, kv_len, false, head_dim, strides, 6);
    if (rc != SKV_OK) return rc;
    if (((uintptr_t)col_score | (uintptr_t)diag_score | (uintptr_t)workspace) % 4) return SKV_ERR_ARG;
    const long long n_chunk = (q_len + VS_CHUNK - 1) / VS_CHUNK, n_tile = (q_len + FT_KB - 1) / FT_KB;
    const long long nbh = (long long)batch_size * q_heads;
    if (nbh * n_tile > INT_MAX) return SKV_ERR_UNSUPPORTED;
    const int G = q_heads / kv_heads;
    hipLaunchKernelGGL(vs_rowstat_kernel, dim3((unsigned)(nbh * n_chunk)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)q, (const bf16_t*)k, (float*)workspace, q_heads, G, q_len, q_stride_b, q_stride_h,
                       q_stride_s, k_stride_b, k_stride_h, k_stride_s, (int)n_chunk);
    if (hipGetLastError() != hipSuccess) return SKV_ERR_LAUNCH;
    hipLaunchKernelGGL(vs_scores_kernel, dim3((unsigned)(nbh * n_tile)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)q, (const bf16_t*)k, (const float*)workspace, (float*)col_score, (float*)diag_score,
                       q_heads, G, q_len, q_stride_b, q_stride_h, q_stride_s, k_stride_b, k_stride_h, k_stride_s,
                       (int)n_chunk, (int)n_tile);
    return hipGetLastError() == hipSuccess ? SKV_OK : SKV_ERR_LAUNCH;
}

extern "C" int skv_vs_sparse_attention(const void* q, const void* k, const void* v, void* out, const void* vertical_idx,
                                       const void* slash_idx, void* workspace, int batch_size, int q_heads, int kv_heads,
                                       int q_len, int kv_len, int head_dim, int n_vertical, int n_slash,
                                       long long q_stride_b, long long q_stride_h, long long q_stride_s,
                                       long long k_stride_b, long long k_stride_h, long long k_stride_s,
                                       long long v_stride_b, long long v_stride_h, long long v_stride_s, float scale,
                                       skv_stream_t stream) {
    const void* const ptrs[2] = {q, k};
    const long long strides[9] = {q_stride_b, q_stride_h, q_stride_s, k_stride_b, k_stride_h,
                                  k_stride_s, v_stride_b, v_stride_h, v_stride_s};
    if (!v || !out || !vertical_idx || !slash_idx || !workspace) return SKV_ERR_ARG;
    if (n_vertical < 1 || n_slash < 1) return SKV_ERR_ARG;
    const int rc = ft_check_attn_args(ptrs, 2, batch_size, q_heads, kv_heads, q_len, kv_len, false, head_dim, strides, 9);
    if (rc != SKV_OK) return rc;
    if (((uintptr_t)v | (uintptr_t)out) % 16) return SKV_ERR_ARG;
    if (((uintptr_t)vertical_idx | (uintptr_t)slash_idx | (uintptr_t)workspace) % 4) return SKV_ERR_ARG;
    const long long n_blk = (q_len + FT_KB - 1) / FT_KB, nbh = (long long)batch_size * q_heads;
    if (nbh * n_blk > INT_MAX) return SKV_ERR_UNSUPPORTED;
    const int words = (q_len + 31) / 32;
    hipLaunchKernelGGL(vs_bitmap_kernel, dim3((unsigned)nbh), dim3(256), 0, (hipStream_t)stream, (const int*)slash_idx,
                       (uint32_t*)workspace, q_len, n_slash, words);
    if (hipGetLastError() != hipSuccess) return SKV_ERR_LAUNCH;
    hipLaunchKernelGGL(vs_attn_kernel, dim3((unsigned)(nbh * n_blk)), dim3(128), 0, (hipStream_t)stream, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, (const int*)vertical_idx, (const int*)slash_idx,
                       (const uint32_t*)workspace, q_heads, q_heads / kv_heads, q_len, n_vertical, n_slash, words,
                       q_stride_b, q_stride_h, q_stride_s, k_stride_b, k_stride_h, k_stride_s, v_stride_b, v_stride_h,
                       v_stride_s, scale * 1.44269504088896341f, (int)n_blk);
    return hipGetLastError() == hipSuccess ? SKV_OK : SKV_ERR_LAUNCH;
}
