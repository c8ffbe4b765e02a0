// Body of the landmark scan kernels of skv_select.hip (skv_score_tile_kernel, skv_score_tile_fp8_kernel): included once per
// kernel with SKV_SCORE_F8 defined to 0 or 1, NOT a header.  Textual inclusion (and not a shared inline function) because the
// bf16 kernel's code must not move with this feature: its G = 4 instantiation sits exactly at its 64-VGPR budget, and as an
// inlined function the same statements were register-allocated and scheduled differently.
//
// In scope: template <int G, int ABL, int WAVES, int PD, bool KVP>; q, lm, D, part_max, part_sum, N, T, alpha, eh, fs, kp;
// lm_scale (FP8: f32 [B][N]).  FP8 (DESIGN.md section 13): lm is the e4m3 byte table [B][N][128]; same lane <-> element
// assignment (a lane's 8 bytes are elements 8*sub .. 8*sub+7, a wave-instruction reads 4 rows = 512 contiguous bytes); the
// row's scale is requested WITH the row (no dependent round trip); the lane rebuilds the 16-byte unit the bf16 table would
// have held (skv_fp8v.h: exact) and hands it to score_row_group unchanged, so the FP8 scan writes the bytes the bf16 scan
// writes for the dequantised table.
    constexpr bool F8 = SKV_SCORE_F8 != 0 && G > 0;   // (value-dependent: the other form's statements are discarded, not checked)
    // k/v projection role (skv_kvproj.h; KVP: an instantiation of its own, the plain scan keeps its registers and LDS):
    // kp.blocks workgroups in grid rows of their own BEHIND the scan's tiles, so the scan's dispatch ramp is not delayed
    if constexpr (KVP) {
        const int role_y0 = (int)gridDim.y - (kp.blocks + (int)gridDim.x - 1) / (int)gridDim.x;
        if ((int)blockIdx.y >= role_y0) {
            __shared__ __attribute__((aligned(16))) unsigned char s_kvp[SKV_KV_PROJ_LDS_BYTES];
            const int rb = ((int)blockIdx.y - role_y0) * (int)gridDim.x + (int)blockIdx.x;
            if (rb < kp.blocks) skv_kv_proj_role<64 * WAVES, false>(kp, rb, threadIdx.x, s_kvp);
            return;
        }
    }
    constexpr int ITERS = 64 / WAVES;               // 4-row wave-instructions per wave
    constexpr int GH = G > 8 ? 4 : G;               // query heads per pass
    constexpr int PASSES = G / GH;
    constexpr int GP = (GH + 1) / 2;
    constexpr int DEPTH = PD < ITERS ? PD : ITERS;
    static_assert(G % GH == 0, "G must be 1, 2, 4, 8 or a multiple of 4");
    const int b = blockIdx.y, t = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 15, rsel = lane >> 4;
    __shared__ __attribute__((aligned(16))) bf16_t sD[G][SKV_TILE];
    // query heads of passes 1.. : one private copy per wave (written and read by the same wave: no barrier)
    __shared__ __attribute__((aligned(16))) bf16_t sQ[PASSES > 1 ? WAVES : 1][PASSES > 1 ? (G - GH) * 128 : 8];

    // q fragment of the first pass: GH x 8 floats, packed in pairs of query heads for v_pk_fma_f32
    f32x2 qf[GP][8];
    auto unpack_q = [&](int gp, const u32x4 w0, const u32x4 w1) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            qf[gp][2 * j] = (f32x2){bf_lo(w0[j]), bf_lo(w1[j])};
            qf[gp][2 * j + 1] = (f32x2){bf_hi(w0[j]), bf_hi(w1[j])};
        }
    };
#pragma unroll
    for (int gp = 0; gp < GP; ++gp) {
        u32x4 w0 = *reinterpret_cast<const u32x4*>(q + ((size_t)b * G + 2 * gp) * 128 + 8 * sub);
        u32x4 w1 = (2 * gp + 1 < GH) ? *reinterpret_cast<const u32x4*>(q + ((size_t)b * G + 2 * gp + 1) * 128 + 8 * sub) : w0;
        unpack_q(gp, w0, w1);
    }
    if constexpr (PASSES > 1) {
        constexpr int QV = (G - GH) * 16;           // 16-B units of the later passes' heads
#pragma unroll
        for (int k = 0; k < (QV + 63) / 64; ++k) {
            const int u = lane + 64 * k;
            if (u < QV) reinterpret_cast<u32x4*>(&sQ[wave][0])[u] = reinterpret_cast<const u32x4*>(q + ((size_t)b * G + GH) * 128)[u];
        }
    }

    const bool flag_wave = ABL == 0 && eh.dthr_in != nullptr && wave == (G < WAVES ? G : 0);
    // early fetch: the heads' thresholds.  Uniform addresses (kernel argument + blockIdx): scalar loads into SGPRs, requested
    // here and consumed behind the barrier - no vector register is held across the loop (the G = 4 kernel sits exactly at
    // its 64-VGPR budget) and no wave waits for them
    float dth[G];
#pragma unroll
    for (int g = 0; g < G; ++g) dth[g] = (ABL == 0 && eh.dthr_in != nullptr) ? eh.dthr_in[(size_t)blockIdx.y * G + g] : INFINITY;
    const int row0 = t * SKV_TILE + wave * (4 * ITERS) + rsel;
    typename ScoreRowUnit<F8>::type x[ITERS];
    float xs[F8 ? ITERS : 1];     // F8: the rows' scales (f32 powers of two)
    auto request = [&](int i) __attribute__((always_inline)) {
        int row = row0 + i * 4;
        row = row < N ? row : N - 1;  // clamp: out-of-range rows are computed and discarded
        if constexpr (F8) {
            x[i] = __builtin_nontemporal_load(
                reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned char*>(lm) + ((size_t)b * N + row) * 128 + 8 * sub));
            xs[i] = lm_scale[(size_t)b * N + row];
        } else {
            x[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(lm + ((size_t)b * N + row) * 128 + 8 * sub));
        }
    };
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) request(i);
    if (ABL == 1) {   // memory stream only: fold the loaded words so the loads stay, skip all arithmetic
        uint32_t f = 0;
#pragma unroll
        for (int i = 0; i < ITERS; ++i) {
            if (i + DEPTH < ITERS) request(i + DEPTH);
            if constexpr (F8) f ^= x[i][0] ^ x[i][1] ^ __float_as_uint(xs[i]);
            else f ^= x[i][0] ^ x[i][1] ^ x[i][2] ^ x[i][3];
            __builtin_amdgcn_sched_barrier(0);
        }
        if (f == 0x12345u) D[0] = (bf16_t)f;
        return;
    }
    SCORE_STAMP(0);
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
        // program order: request row group i + DEPTH, then consume row group i (the compiler's counted vmcnt wait leaves the
        // DEPTH younger requests in flight); the scheduling barriers keep hipcc from hoisting every request to the top again
        if (i + DEPTH < ITERS) request(i + DEPTH);
        __builtin_amdgcn_sched_barrier(0);
#ifdef SKV_SCORE_STAMPS
        if (i == 0 || i == ITERS - 1) {          // when the first / the last row group's data is there
            if (x[i][0] == 0x12345678u) sD[0][0] = 1;
            SCORE_STAMP(i == 0 ? 1 : 2);
        }
#endif
        if constexpr (F8) score_row_group<GH>(qf, skv_e4m3x8_dequant(x[i], xs[i]), &sD[0][0], wave * (4 * ITERS) + i * 4 + rsel, lane, alpha);
        else score_row_group<GH>(qf, x[i], &sD[0][0], wave * (4 * ITERS) + i * 4 + rsel, lane, alpha);
        __builtin_amdgcn_sched_barrier(0);
    }
    SCORE_STAMP(3);
    if constexpr (PASSES > 1) {
#pragma unroll
        for (int p = 1; p < PASSES; ++p) {
            // the next pass's q fragment must not be built while this one is live, and the stash must really be READ here
            // (forwarding the stored registers would keep all G heads live: that is what the stash is there to avoid)
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int gp = 0; gp < GP; ++gp) {
                const u32x4 w0 = *reinterpret_cast<const u32x4*>(&sQ[wave][((p - 1) * GH + 2 * gp) * 128 + 8 * sub]);
                const u32x4 w1 = *reinterpret_cast<const u32x4*>(&sQ[wave][((p - 1) * GH + 2 * gp + 1) * 128 + 8 * sub]);
                unpack_q(gp, w0, w1);
            }
#pragma unroll
            for (int i = 0; i < ITERS; ++i) {
                if constexpr (F8)
                    score_row_group<GH>(qf, skv_e4m3x8_dequant(x[i], xs[i]), &sD[p * GH][0], wave * (4 * ITERS) + i * 4 + rsel, lane, alpha);
                else
                    score_row_group<GH>(qf, x[i], &sD[p * GH][0], wave * (4 * ITERS) + i * 4 + rsel, lane, alpha);
                __builtin_amdgcn_sched_barrier(0);  // one row group at a time (interleaved they need > 64 VGPRs)
            }
        }
    }
    __syncthreads();
    SCORE_STAMP(4);
    if (ABL == 2) {
        if (tid < SKV_TILE && t * SKV_TILE + tid < N) {
#pragma unroll
            for (int g = 0; g < G; ++g) D[((size_t)b * G + g) * N + t * SKV_TILE + tid] = sD[g][tid];
        }
        return;
    }

    // fused selection (fs.ctil != nullptr): per slot the 15-bit key of kappa = max_g (logit_g - ctil_g) and the slot's G logits
    // side by side (Dt [B][N][G]) - every wave takes 256 / WAVES columns, one lane per column (G LDS reads of 2 B, a few VALU
    // operations, one 2-B and one 2G-B store per lane: 64-B / 16G-B runs per wave); D [B][G][N] is not written then
    const bool fused = ABL == 0 && fs.ctil != nullptr;
    if (fused) {
        constexpr int CPW = SKV_TILE / WAVES;                // columns per wave: 16 (G <= 4) or 32 (G = 8)
        const int col = wave * CPW + lane, j = t * SKV_TILE + col;
        if (lane < CPW && j < N) {
            float kap = -INFINITY;
            uint32_t pk[(G + 1) / 2];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const bf16_t d = sD[g][col];
                kap = fmaxf(kap, bf2f(d) - fs.ctil[(size_t)b * G + g]);
                if (g & 1) pk[g / 2] |= (uint32_t)d << 16;
                else pk[g / 2] = d;
            }
            // (clamped below zero: K_j = D - c <= 0 always, a kappa above it is a stale ctil - the clamp is monotone, so the
            // candidate rule stands, and it keeps every key of a row within a few hundred codes: one histogram window)
            fs.keys[(size_t)b * fs.key_stride + j] = skv_kappa_key(fminf(kap, -0x1p-12f));
            bf16_t* dt = reinterpret_cast<bf16_t*>(fs.Dt) + ((size_t)b * N + j) * G;
            if constexpr (G == 8) *reinterpret_cast<u32x4*>(dt) = (u32x4){pk[0], pk[1], pk[2], pk[3]};
            else if constexpr (G == 4) *reinterpret_cast<u32x2*>(dt) = (u32x2){pk[0], pk[1]};
            else if constexpr (G == 2) *reinterpret_cast<uint32_t*>(dt) = pk[0];
            else {
#pragma unroll
                for (int g = 0; g < G; ++g) dt[g] = sD[g][col];
            }
        }
    }
    // early-fetch flags (off: eh.dthr_in == nullptr): one wave that has no query head in the statistics below (or wave 0)
    // compares its 4 columns' logits with the heads' thresholds and compacts the flagged slots of the tile
    if (flag_wave) {
        const int c0 = 4 * lane;
        unsigned fl = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float th = dth[g];
            const u32x2 v = *reinterpret_cast<const u32x2*>(&sD[g][c0]);     // the lane's 4 logits of head g: one LDS read
            fl |= (bf_lo(v[0]) >= th ? 1u : 0u) | (bf_hi(v[0]) >= th ? 2u : 0u) | (bf_lo(v[1]) >= th ? 4u : 0u) |
                  (bf_hi(v[1]) >= th ? 8u : 0u);
        }
        if ((t + 1) * SKV_TILE > N) {                        // last tile: columns past the row are not slots
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t * SKV_TILE + c0 + k >= N) fl &= ~(1u << k);
        }
        int base = 0;
        if (__ballot(fl != 0u) != 0ull) {                    // (most tiles of most steps have a few flagged slots; many have none)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long bal = __ballot((fl >> k) & 1u);
                const int pos = base + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
                if (((fl >> k) & 1u) && pos < SKV_EARLY_K)
                    eh.flag_slot[((size_t)b * T + t) * SKV_EARLY_K + pos] = t * SKV_TILE + c0 + k;
                base += __builtin_popcountll(bal);
            }
        }
        if (lane == 0) eh.flag_cnt[(size_t)b * T + t] = min(base, SKV_EARLY_K);
    }
    // per-tile statistics: wave w owns query head g = w (+ k*waves) and all 256 columns of the tile, 4 consecutive
    // columns per lane, so max, integer exp-sum and the logit store need no cross-wave step and no further barrier
    // (ablation, tools/score_probe.hip: the previous column-per-thread tail cost 3.5 of 11.5 us).
    for (int g = wave; g < G; g += WAVES) {
        const int c0 = 4 * lane;
        float dv[4];
        float mloc = -INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dv[k] = bf2f(sD[g][c0 + k]);
            if (t * SKV_TILE + c0 + k < N) mloc = fmaxf(mloc, dv[k]);
        }
        const float m = wave_max_dpp(mloc);
        unsigned long long e = 0ull;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t * SKV_TILE + c0 + k < N) e += exp_to_fixed(spec_exp(dv[k] - m));
        e = wave_sum_u64_dpp(e);
        bf16_t* drow = D + ((size_t)b * G + g) * N + (size_t)t * SKV_TILE + c0;
        if (fused) {
            // (the logits went out slot-major above)
        } else if (t * SKV_TILE + c0 + 3 < N && (((size_t)drow) & 7) == 0) {
            *reinterpret_cast<u32x2*>(drow) = *reinterpret_cast<const u32x2*>(&sD[g][c0]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t * SKV_TILE + c0 + k < N) drow[k] = sD[g][c0 + k];
        }
        if (lane == 0) {
            part_max[((size_t)b * T + t) * G + g] = m;
            part_sum[((size_t)b * T + t) * G + g] = fixed_to_float(e);
        }
    }
    SCORE_STAMP(5);
