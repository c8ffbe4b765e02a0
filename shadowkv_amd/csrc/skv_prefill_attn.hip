// Causal GQA flash attention, forward pass, for the prefill of a prompt (DecoderLM.prefill: flash_attn_with_kvcache(causal=True)
// at the reference's models/base.py:293 and :311).  bf16 in / out, f32 accumulation, head_dim 128.
//
// Mask (flash-attn's causal convention, aligned bottom-right): query row i of q_len attends keys j <= kv_len - q_len + i.
// kv_len == q_len is the prompt itself; kv_len > q_len a continuation on top of a full-attention cache.
//
// Structure (flash-style loop, one pass over K / V per query block):
//   workgroup = 4 waves = 128 query rows of one (sequence, query head); wave w owns rows q0 + 32 w .. + 31.
//   Q tile of a wave in registers as the B operand of v_mfma_f32_32x32x16_bf16 (lane l: row l & 31, dims 16 s + 8 (l >> 5) ..).
//   K / V tiles of 64 keys streamed through LDS: K row-major (272-byte rows: conflict-free 16-byte row reads), V transposed
//   ([d][key], 144-byte rows) so that the P.V operand is 8-byte reads.  The next tile's global loads are issued before the
//   current tile's MFMAs and written to LDS after them (one LDS buffer, two barriers per tile).
//   S^T = K.Q^T ("swapped" product): a lane holds 32 scores of ONE query row (its column l & 31); the row max / sum need only
//   the partner lane l ^ 32.  The f32 score tile is then the B operand of O^T += V^T.P^T with no lane movement: registers
//   8 s .. 8 s + 7 of a 32-key score tile, rounded to bf16 (as flash-attn rounds P before P.V), are the fragment of k-step s,
//   and the V^T operand takes its keys in the same permuted order (key 16 s + 8 (j >> 2) + 4 h + (j & 3) for element j).
//   O^T accumulates in 4 x 16 f32 per lane: query l & 31, dims 32 dblk + (r & 3) + 8 (r >> 2) + 4 h.
//   Online softmax in f32 in the log2 domain, the textbook order (the running max is updated, and O rescaled, on every tile
//   whose max grows; no deferred-max threshold).
//   Tiles wholly above a wave's diagonal are skipped; only tiles that cross it are masked.  The grid is ordered last query
//   block first, so the longest workgroups start first and the causal triangle leaves no tail of long ones.  The query heads
//   of one KV head are adjacent in the grid (their K / V reads meet in the caches).
#include "../../include/shadowkv_hip.h"
#include "skv_common.h"

#include <limits.h>

typedef __attribute__((ext_vector_type(8))) __bf16 pf_bf16x8;
typedef __attribute__((ext_vector_type(16))) float pf_f32x16;

#define PF_D 128
#define PF_QB 128            // query rows per workgroup (4 waves x 32)
#define PF_KB 64             // keys per tile
#define PF_KP (PF_D + 8)     // K LDS row pitch, bf16 (272 bytes)
#define PF_VP (PF_KB + 8)    // V^T LDS row pitch, bf16 (144 bytes)

// row of the 32x32 C/D tile held in register r by lane half h
__device__ __forceinline__ int pf_crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__global__ __launch_bounds__(256) void skv_prefill_attn_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, bf16_t* __restrict__ out,
    int bs, int Hq, int G, int q_len, int kv_len, long long qsb, long long qsh, long long qss, long long ksb, long long ksh,
    long long kss, long long vsb, long long vsh, long long vss, float scale_log2, int n_qblk) {
    __shared__ __attribute__((aligned(16))) bf16_t s_k[PF_KB * PF_KP];
    __shared__ __attribute__((aligned(16))) bf16_t s_vt[PF_D * PF_VP];

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
    const int n_tiles = (off + min(q0 + PF_QB, q_len) - 1) / PF_KB + 1;

    // Q fragments (B operand of the score product): Q[qi][16 s + 8 h .. + 7]
    pf_bf16x8 qf[8];
    {
        const bf16_t* qp = q + (long long)b * qsb + (long long)hq * qsh + (long long)min(qi, q_len - 1) * qss + 8 * h;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            u32x4 w = *reinterpret_cast<const u32x4*>(qp + 16 * s);
            if (!row_ok) w = (u32x4){0u, 0u, 0u, 0u};
            qf[s] = __builtin_bit_cast(pf_bf16x8, w);
        }
    }

    // tile staging: thread t moves rows 2 p and 2 p + 1 (p = (t + 256 i) >> 4, i = 0, 1) of chunk c = t & 15 (dims 8 c .. 8 c + 7)
    const bf16_t* kb = k + (long long)b * ksb + (long long)hk * ksh;
    const bf16_t* vb = v + (long long)b * vsb + (long long)hk * vsh;
    const int st_c = tid & 15;
    u32x4 kr[2][2], vr[2][2];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = (tid + 256 * i) >> 4;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int key = t * PF_KB + 2 * p + e;
                u32x4 a = {0u, 0u, 0u, 0u}, c = {0u, 0u, 0u, 0u};
                if (key < kv_len) {
                    a = *reinterpret_cast<const u32x4*>(kb + (long long)key * kss + 8 * st_c);
                    c = *reinterpret_cast<const u32x4*>(vb + (long long)key * vss + 8 * st_c);
                }
                kr[i][e] = a;
                vr[i][e] = c;
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = (tid + 256 * i) >> 4;
#pragma unroll
            for (int e = 0; e < 2; ++e) *reinterpret_cast<u32x4*>(&s_k[(2 * p + e) * PF_KP + 8 * st_c]) = kr[i][e];
            // V^T: element j of the chunk is dim 8 c + j; keys 2 p and 2 p + 1 share one 32-bit word
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t x0 = vr[i][0][w], x1 = vr[i][1][w];
                const uint32_t lo = (x0 & 0xffffu) | (x1 << 16);
                const uint32_t hi = (x0 >> 16) | (x1 & 0xffff0000u);
                *reinterpret_cast<uint32_t*>(&s_vt[(8 * st_c + 2 * w) * PF_VP + 2 * p]) = lo;
                *reinterpret_cast<uint32_t*>(&s_vt[(8 * st_c + 2 * w + 1) * PF_VP + 2 * p]) = hi;
            }
        }
    };

    pf_f32x16 o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = (pf_f32x16){};
    float m = -INFINITY, l = 0.f;

    load_tile(0);
    for (int t = 0; t < n_tiles; ++t) {
        __syncthreads();                       // every wave is done reading the previous tile
        store_tile();
        __syncthreads();
        if (t + 1 < n_tiles) load_tile(t + 1); // in flight under this tile's MFMAs
        const int key0 = t * PF_KB;
        if (!wave_on || key0 > wave_hi) continue;

        // S^T[key][query] for keys key0 + 32 kb + crow(reg, h), query qi
        pf_f32x16 sc[2];
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2) {
            sc[kb2] = (pf_f32x16){};
            const bf16_t* kp = &s_k[(32 * kb2 + r) * PF_KP + 8 * h];
#pragma unroll
            for (int s = 0; s < 8; ++s)
                sc[kb2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    __builtin_bit_cast(pf_bf16x8, *reinterpret_cast<const u32x4*>(kp + 16 * s)), qf[s], sc[kb2], 0, 0, 0);
        }
        float mt = -INFINITY;
        if (key0 + PF_KB - 1 > wave_lo) {      // the tile crosses the diagonal of some row of this wave
#pragma unroll
            for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = key0 + 32 * kb2 + pf_crow(i, h);
                    const float x = key <= lim ? sc[kb2][i] * scale_log2 : -INFINITY;
                    sc[kb2][i] = x;
                    mt = fmaxf(mt, x);
                }
        } else {
#pragma unroll
            for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float x = sc[kb2][i] * scale_log2;
                    sc[kb2][i] = x;
                    mt = fmaxf(mt, x);
                }
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        // key 0 is visible to every row, so m is finite from tile 0 on; a row with no visible key in this tile keeps m
        const float m_new = fmaxf(m, mt);
        const float alpha = __builtin_amdgcn_exp2f(m - m_new);    // 0 on tile 0 (m = -inf), 1 when the max does not grow
        m = m_new;
        float rs = 0.f;
        uint32_t pk[2][8];
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
            for (int i = 0; i < 16; i += 2) {
                const float p0 = __builtin_amdgcn_exp2f(sc[kb2][i] - m_new);
                const float p1 = __builtin_amdgcn_exp2f(sc[kb2][i + 1] - m_new);
                rs += p0;
                rs += p1;
                pk[kb2][i >> 1] = pack_bf2(p0, p1);
            }
        l = l * alpha + rs;
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[d][i] *= alpha;

        // O^T[d][query] += V^T[d][key] P^T[key][query], k-step (kb2, s): keys key0 + 32 kb2 + 16 s + ...
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const pf_bf16x8 pb = __builtin_bit_cast(
                    pf_bf16x8, (u32x4){pk[kb2][4 * s], pk[kb2][4 * s + 1], pk[kb2][4 * s + 2], pk[kb2][4 * s + 3]});
                const int kc = 32 * kb2 + 16 * s + 4 * h;
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const bf16_t* vp = &s_vt[(32 * d + r) * PF_VP + kc];
                    const u32x2 a0 = *reinterpret_cast<const u32x2*>(vp);
                    const u32x2 a1 = *reinterpret_cast<const u32x2*>(vp + 8);
                    const pf_bf16x8 va = __builtin_bit_cast(pf_bf16x8, (u32x4){a0[0], a0[1], a1[0], a1[1]});
                    o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, pb, o[d], 0, 0, 0);
                }
            }
    }

    if (!row_ok) return;
    l = l + __shfl_xor(l, 32);
    const float inv = 1.0f / l;
    bf16_t* op = out + (((long long)b * q_len + qi) * Hq + hq) * PF_D + 4 * h;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const u32x2 w = {pack_bf2(o[d][4 * g] * inv, o[d][4 * g + 1] * inv),
                             pack_bf2(o[d][4 * g + 2] * inv, o[d][4 * g + 3] * inv)};
            *reinterpret_cast<u32x2*>(op + 32 * d + 8 * g) = w;
        }
}

extern "C" int skv_prefill_attention(const void* q, const void* k, const void* v, void* out, int batch_size, int q_heads,
                                     int kv_heads, int q_len, int kv_len, int head_dim, long long q_stride_b,
                                     long long q_stride_h, long long q_stride_s, long long k_stride_b, long long k_stride_h,
                                     long long k_stride_s, long long v_stride_b, long long v_stride_h, long long v_stride_s,
                                     float scale, skv_stream_t stream) {
    if (!q || !k || !v || !out) return SKV_ERR_ARG;
    if (batch_size < 1 || q_heads < 1 || kv_heads < 1 || q_len < 1 || kv_len < q_len || q_heads % kv_heads) return SKV_ERR_ARG;
    const long long strides[9] = {q_stride_b, q_stride_h, q_stride_s, k_stride_b, k_stride_h,
                                  k_stride_s, v_stride_b, v_stride_h, v_stride_s};
    for (long long s : strides)
        if (s % 8) return SKV_ERR_ARG;          // 16-byte rows: every operand row is read as 16-byte vectors
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) % 16) return SKV_ERR_ARG;
    if (head_dim != PF_D) return SKV_ERR_UNSUPPORTED;
    const long long n_qblk = (q_len + PF_QB - 1) / PF_QB;
    const long long grid = n_qblk * batch_size * q_heads;
    if (grid > INT_MAX) return SKV_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(skv_prefill_attn_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, batch_size, q_heads, q_heads / kv_heads, q_len,
                       kv_len, q_stride_b, q_stride_h, q_stride_s, k_stride_b, k_stride_h, k_stride_s, v_stride_b, v_stride_h,
                       v_stride_s, scale * 1.44269504088896341f, (int)n_qblk);
    return hipGetLastError() == hipSuccess ? SKV_OK : SKV_ERR_LAUNCH;
}
