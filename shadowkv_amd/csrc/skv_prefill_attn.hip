// Causal GQA flash attention, forward pass, for the prefill of a prompt (DecoderLM.prefill: flash_attn_with_kvcache(causal=True)
// at the reference's models/base.py:293 and :311).  bf16 in / out, f32 accumulation, head_dim 128.
//
// Mask (flash-attn's causal convention, aligned bottom-right): query row i of q_len attends keys j <= kv_len - q_len + i.
// kv_len == q_len is the prompt itself; kv_len > q_len a continuation on top of a full-attention cache.
//
// Structure (flash-style loop, one pass over K / V per query block; the tile body, its register and LDS layouts and the
// online softmax are skv_flash_tile.h):
//   workgroup = 4 waves = 128 query rows of one (sequence, query head); wave w owns rows q0 + 32 w .. + 31.
//   Tile t is keys 64 t .. 64 t + 63.  Tiles wholly above a wave's diagonal are skipped; only tiles that cross it are
//   masked.  Key 0 is visible to every row, so no row is ever empty (CAN_BE_EMPTY = false).
//   The grid is ordered last query block first, so the longest workgroups start first and the causal triangle leaves no
//   tail of long ones.  The query heads of one KV head are adjacent in the grid (their K / V reads meet in the caches).
#include "../../include/shadowkv_hip.h"
#include "skv_flash_tile.h"

#include <limits.h>

#define PF_QB 128            // query rows per workgroup (4 waves x 32)

__global__ __launch_bounds__(256) void skv_prefill_attn_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, bf16_t* __restrict__ out,
    int bs, int Hq, int G, int q_len, int kv_len, long long qsb, long long qsh, long long qss, long long ksb, long long ksh,
    long long kss, long long vsb, long long vsh, long long vss, float scale_log2, int n_qblk) {
    __shared__ __attribute__((aligned(16))) bf16_t s_k[FT_KB * FT_KP];
    __shared__ __attribute__((aligned(16))) bf16_t s_vt[FT_D * FT_VP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nbh = bs * Hq;
    const int bh = (int)(blockIdx.x % (unsigned)nbh);
    const int qblk = n_qblk - 1 - (int)(blockIdx.x / (unsigned)nbh);      // last (longest) query block first
    const int b = bh / Hq, hq = bh - b * Hq, hk = hq / G;
    const int off = kv_len - q_len;
    const int q0 = qblk * PF_QB;
    const int qw = q0 + wave * 32;                                      // first query row of this wave
    const int qi = qw + r;                                              // this lane's query row
    const bool row_ok = qi < q_len;
    const int lim = off + min(qi, q_len - 1);                           // last key this lane's row attends
    const int wave_lo = off + qw;                                       // smallest limit in the wave
    const int wave_hi = off + min(qw + 31, q_len - 1);                  // largest limit in the wave
    const bool wave_on = qw < q_len;
    const int n_tiles = (off + min(q0 + PF_QB, q_len) - 1) / FT_KB + 1;

    ft_bf16x8 qf[8];
    ft_load_q(qf, q + (long long)b * qsb + (long long)hq * qsh + (long long)min(qi, q_len - 1) * qss, row_ok, h);

    const bf16_t* kb = k + (long long)b * ksb + (long long)hk * ksh;
    const bf16_t* vb = v + (long long)b * vsb + (long long)hk * vsh;
    u32x4 kr[2][2], vr[2][2];
    auto load_tile = [&](int t) {
        ft_load_tile<256>(kr, vr, kb, vb, kss, vss, kv_len, tid, [&](int row) { return t * FT_KB + row; });
    };

    ft_f32x16 o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = (ft_f32x16){};
    float m = -INFINITY, l = 0.f;

    load_tile(0);
    for (int t = 0; t < n_tiles; ++t) {
        __syncthreads();                       // every wave is done reading the previous tile
        ft_store_tile<256>(s_k, s_vt, kr, vr, tid);
        __syncthreads();
        if (t + 1 < n_tiles) load_tile(t + 1); // in flight under this tile's MFMAs
        const int key0 = t * FT_KB;
        if (!wave_on || key0 > wave_hi) continue;

        ft_f32x16 sc[2];
        ft_scores_from_lds(sc, s_k, qf, r, h);
        float mt = -INFINITY;
        if (key0 + FT_KB - 1 > wave_lo) {      // the tile crosses the diagonal of some row of this wave
#pragma unroll
            for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = key0 + 32 * kb2 + ft_crow(i, h);
                    const float x = key <= lim ? sc[kb2][i] * scale_log2 : -INFINITY;
                    sc[kb2][i] = x;
                    mt = fmaxf(mt, x);
                }
        } else {
            mt = ft_scale_unmasked(sc, scale_log2);
        }
        ft_softmax_pv<false>(sc, mt, m, l, o, s_vt, r, h);
    }

    if (!row_ok) return;
    ft_write_out<false>(o, l, out + (((long long)b * q_len + qi) * Hq + hq) * FT_D, h);
}

extern "C" int skv_prefill_attention(const void* q, const void* k, const void* v, void* out, int batch_size, int q_heads,
                                     int kv_heads, int q_len, int kv_len, int head_dim, long long q_stride_b,
                                     long long q_stride_h, long long q_stride_s, long long k_stride_b, long long k_stride_h,
                                     long long k_stride_s, long long v_stride_b, long long v_stride_h, long long v_stride_s,
                                     float scale, skv_stream_t stream) {
    const void* const ptrs[4] = {q, k, v, out};
    const long long strides[9] = {q_stride_b, q_stride_h, q_stride_s, k_stride_b, k_stride_h,
                                  k_stride_s, v_stride_b, v_stride_h, v_stride_s};
    const int rc = ft_check_attn_args(ptrs, 4, batch_size, q_heads, kv_heads, q_len, kv_len, true, head_dim, strides, 9);
    if (rc != SKV_OK) return rc;
    const long long n_qblk = (q_len + PF_QB - 1) / PF_QB;
    const long long grid = n_qblk * batch_size * q_heads;
    if (grid > INT_MAX) return SKV_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(skv_prefill_attn_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, batch_size, q_heads, q_heads / kv_heads, q_len,
                       kv_len, q_stride_b, q_stride_h, q_stride_s, k_stride_b, k_stride_h, k_stride_s, v_stride_b, v_stride_h,
                       v_stride_s, scale * 1.44269504088896341f, (int)n_qblk);
    return hipGetLastError() == hipSuccess ? SKV_OK : SKV_ERR_LAUNCH;
}
