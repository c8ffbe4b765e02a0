// One 64-key tile step of bf16 flash attention (forward, head_dim 128, f32 accumulation) on v_mfma_f32_32x32x16_bf16,
// shared by the dense causal prefill kernel (skv_prefill_attn.hip) and the MInference vertical + slash kernel
// (skv_minference.hip).  A kernel keeps what is its own - which keys make up a tile, the mask, the workgroup shape, the
// skip conditions - and calls in here for everything else.  One wave owns 32 query rows; lane l: r = l & 31, h = l >> 5.
//
// Layouts:
//   Q tile of a wave in registers as the B operand of the MFMA (lane l: query row r, dims 16 s + 8 h .. + 7 in qf[s]).
//   K / V tiles of 64 keys go through LDS: K row-major (FT_KP: 272-byte rows, conflict-free 16-byte row reads), V transposed
//   ([d][key], FT_VP: 144-byte rows) so that the P.V operand is 8-byte reads.  A kernel loads the next tile's rows from
//   global memory into registers (ft_load_tile) before the current tile's MFMAs and writes them to LDS after them
//   (ft_store_tile; one LDS buffer, two barriers per tile).
//   S^T = K.Q^T ("swapped" product): a lane holds 32 scores of ONE query row (its column r) per 32-key half, key
//   32 kb2 + ft_crow(i, h) in sc[kb2][i]; the row max / sum need only the partner lane l ^ 32.  The f32 score tile is then
//   the B operand of O^T += V^T.P^T with no lane movement: registers 8 s .. 8 s + 7 of a 32-key score tile, rounded to bf16
//   (as flash-attn rounds P before P.V), are the fragment of k-step s, and the V^T operand takes its keys in the same
//   permuted order (key 16 s + 8 (j >> 2) + 4 h + (j & 3) for element j).
//   O^T accumulates in 4 x 16 f32 per lane: query r, dims 32 d + ft_crow(i, h) in o[d][i].
//   Online softmax in f32 in the log2 domain, the textbook order (the running max is updated, and O rescaled, on every tile
//   whose max grows; no deferred-max threshold).
//
// CAN_BE_EMPTY (ft_softmax_pv, ft_write_out): a row of the sparse kernel may have met no key yet (m = -inf) or none at all
// (l = 0); the guards keep its weights and its output at 0 instead of NaN.  In the dense kernel key 0 is visible to every
// row, so the guards would never fire and the guarded form yields the same bits there; they are a template parameter, not
// unconditional, so that the dense softmax step carries no extra compare / select per tile.
//
// Every floating-point operation below keeps its order (built with -ffp-contract=off): results are fixed bit for bit.
#pragma once
#include "skv_common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 ft_bf16x8;
typedef __attribute__((ext_vector_type(16))) float ft_f32x16;

#define FT_D 128
#define FT_KB 64             // keys per tile
#define FT_KP (FT_D + 8)     // K LDS row pitch, bf16 (272 bytes)
#define FT_VP (FT_KB + 8)    // V^T LDS row pitch, bf16 (144 bytes)

// row of the 32x32 C/D tile held in register r by lane half h
__device__ __forceinline__ int ft_crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Q fragments of the row at qp (B operand of S^T = K.Q^T), zero when !ok (qp must still be readable)
__device__ __forceinline__ void ft_load_q(ft_bf16x8 (&qf)[8], const bf16_t* qp, bool ok, int h) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        u32x4 w = *reinterpret_cast<const u32x4*>(qp + 8 * h + 16 * s);
        if (!ok) w = (u32x4){0u, 0u, 0u, 0u};
        qf[s] = __builtin_bit_cast(ft_bf16x8, w);
    }
}

// Tile staging by NTHREADS threads: thread t moves rows 2 p and 2 p + 1 (p = ft_pair_row(t, i), i < 512 / NTHREADS) of chunk
// c = t & 15 (dims 8 c .. 8 c + 7).  p = (t + NTHREADS i) >> 4 = (t >> 4) + (NTHREADS / 16) i: one value, two spellings.  The
// compiler does not fold one into the other and builds each kernel's staging addresses, and from them its schedule, on
// the spelling it is given: the 256-thread kernel is measurably faster on the first, the 128-thread kernel on the second.
template <int NTHREADS>
__device__ __forceinline__ int ft_pair_row(int tid, int i) {
    return NTHREADS == 256 ? (tid + NTHREADS * i) >> 4 : (tid >> 4) + (NTHREADS / 16) * i;
}

// key_of(row) names the key of tile row `row`; rows whose key is >= n_keys are zero.
template <int NTHREADS, typename KeyOf>
__device__ __forceinline__ void ft_load_tile(u32x4 (&kr)[512 / NTHREADS][2], u32x4 (&vr)[512 / NTHREADS][2], const bf16_t* kb,
                                             const bf16_t* vb, long long kss, long long vss, int n_keys, int tid, KeyOf key_of) {
    const int st_c = tid & 15;
#pragma unroll
    for (int i = 0; i < 512 / NTHREADS; ++i) {
        const int p = ft_pair_row<NTHREADS>(tid, i);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int key = key_of(2 * p + e);
            u32x4 a = {0u, 0u, 0u, 0u}, c = {0u, 0u, 0u, 0u};
            if (key < n_keys) {
                a = *reinterpret_cast<const u32x4*>(kb + (long long)key * kss + 8 * st_c);
                c = *reinterpret_cast<const u32x4*>(vb + (long long)key * vss + 8 * st_c);
            }
            kr[i][e] = a;
            vr[i][e] = c;
        }
    }
}

template <int NTHREADS>
__device__ __forceinline__ void ft_store_tile(bf16_t* s_k, bf16_t* s_vt, const u32x4 (&kr)[512 / NTHREADS][2],
                                              const u32x4 (&vr)[512 / NTHREADS][2], int tid) {
    const int st_c = tid & 15;
#pragma unroll
    for (int i = 0; i < 512 / NTHREADS; ++i) {
        const int p = ft_pair_row<NTHREADS>(tid, i);
#pragma unroll
        for (int e = 0; e < 2; ++e) *reinterpret_cast<u32x4*>(&s_k[(2 * p + e) * FT_KP + 8 * st_c]) = kr[i][e];
        // V^T: element j of the chunk is dim 8 c + j; keys 2 p and 2 p + 1 share one 32-bit word
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t x0 = vr[i][0][w], x1 = vr[i][1][w];
            const uint32_t lo = (x0 & 0xffffu) | (x1 << 16);
            const uint32_t hi = (x0 >> 16) | (x1 & 0xffff0000u);
            *reinterpret_cast<uint32_t*>(&s_vt[(8 * st_c + 2 * w) * FT_VP + 2 * p]) = lo;
            *reinterpret_cast<uint32_t*>(&s_vt[(8 * st_c + 2 * w + 1) * FT_VP + 2 * p]) = hi;
        }
    }
}

// S^T[key][query] of the tile in s_k: tile row 32 kb2 + ft_crow(i, h), this lane's query, in sc[kb2][i]
__device__ __forceinline__ void ft_scores_from_lds(ft_f32x16 (&sc)[2], const bf16_t* s_k, const ft_bf16x8 (&qf)[8], int r, int h) {
#pragma unroll
    for (int kb2 = 0; kb2 < 2; ++kb2) {
        sc[kb2] = (ft_f32x16){};
        const bf16_t* kp = &s_k[(32 * kb2 + r) * FT_KP + 8 * h];
#pragma unroll
        for (int s = 0; s < 8; ++s)
            sc[kb2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                __builtin_bit_cast(ft_bf16x8, *reinterpret_cast<const u32x4*>(kp + 16 * s)), qf[s], sc[kb2], 0, 0, 0);
    }
}

// the mask of a tile that every row of the wave sees whole: scale only; returns the lane's maximum
__device__ __forceinline__ float ft_scale_unmasked(ft_f32x16 (&sc)[2], float scale_log2) {
    float mt = -INFINITY;
#pragma unroll
    for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float x = sc[kb2][i] * scale_log2;
            sc[kb2][i] = x;
            mt = fmaxf(mt, x);
        }
    return mt;
}

// Online-softmax step and O^T += V^T.P^T for the tile in s_vt.  sc: masked (-inf) and scaled scores, mt: their maximum in
// this lane.  A row with no visible key in this tile keeps m.
template <bool CAN_BE_EMPTY>
__device__ __forceinline__ void ft_softmax_pv(const ft_f32x16 (&sc)[2], float mt, float& m, float& l, ft_f32x16 (&o)[4],
                                              const bf16_t* s_vt, int r, int h) {
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float m_new = fmaxf(m, mt);
    // a row with no key yet: every weight stays 0
    const float m_use = (CAN_BE_EMPTY && m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m - m_use);    // 0 on the row's first tile (m = -inf), 1 when the max does not grow
    m = m_new;
    float rs = 0.f;
    uint32_t pk[2][8];
#pragma unroll
    for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
            const float p0 = __builtin_amdgcn_exp2f(sc[kb2][i] - m_use);
            const float p1 = __builtin_amdgcn_exp2f(sc[kb2][i + 1] - m_use);
            rs += p0;
            rs += p1;
            pk[kb2][i >> 1] = pack_bf2(p0, p1);
        }
    l = l * alpha + rs;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[d][i] *= alpha;

    // O^T[d][query] += V^T[d][key] P^T[key][query], k-step (kb2, s): tile rows 32 kb2 + 16 s + ...
#pragma unroll
    for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const ft_bf16x8 pb = __builtin_bit_cast(
                ft_bf16x8, (u32x4){pk[kb2][4 * s], pk[kb2][4 * s + 1], pk[kb2][4 * s + 2], pk[kb2][4 * s + 3]});
            const int kc = 32 * kb2 + 16 * s + 4 * h;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const bf16_t* vp = &s_vt[(32 * d + r) * FT_VP + kc];
                const u32x2 a0 = *reinterpret_cast<const u32x2*>(vp);
                const u32x2 a1 = *reinterpret_cast<const u32x2*>(vp + 8);
                const ft_bf16x8 va = __builtin_bit_cast(ft_bf16x8, (u32x4){a0[0], a0[1], a1[0], a1[1]});
                o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, pb, o[d], 0, 0, 0);
            }
        }
}

// epilogue: O / l as bf16 to the lane's output row `orow` ([128]); both lanes of a pair must call
template <bool CAN_BE_EMPTY>
__device__ __forceinline__ void ft_write_out(const ft_f32x16 (&o)[4], float l, bf16_t* orow, int h) {
    l = l + __shfl_xor(l, 32);
    const float inv = (CAN_BE_EMPTY && !(l > 0.f)) ? 0.f : 1.0f / l;   // a row that attends no key writes zeros
    bf16_t* op = orow + 4 * h;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const u32x2 w = {pack_bf2(o[d][4 * g] * inv, o[d][4 * g + 1] * inv),
                             pack_bf2(o[d][4 * g + 2] * inv, o[d][4 * g + 3] * inv)};
            *reinterpret_cast<u32x2*>(op + 32 * d + 8 * g) = w;
        }
}

// host: the argument checks every attention entry point makes on its bf16 operands, SKV_ERR_ARG before SKV_ERR_UNSUPPORTED.
// ptrs: the operands read or written as 16-byte vectors; strides in elements.
static inline int ft_check_attn_args(const void* const* ptrs, int n_ptrs, int bs, int Hq, int Hkv, int q_len, int kv_len,
                                     bool kv_may_exceed_q, int head_dim, const long long* strides, int n_strides) {
    uintptr_t bits = 0;
    for (int i = 0; i < n_ptrs; ++i) {
        if (!ptrs[i]) return SKV_ERR_ARG;
        bits |= (uintptr_t)ptrs[i];
    }
    if (bs < 1 || Hq < 1 || Hkv < 1 || q_len < 1 || Hq % Hkv) return SKV_ERR_ARG;
    if (kv_may_exceed_q ? kv_len < q_len : kv_len != q_len) return SKV_ERR_ARG;
    for (int i = 0; i < n_strides; ++i)
        if (strides[i] % 8) return SKV_ERR_ARG;  // 16-byte rows: every operand row is read as 16-byte vectors
    if (bits % 16) return SKV_ERR_ARG;
    if (head_dim != FT_D) return SKV_ERR_UNSUPPORTED;
    return SKV_OK;
}
