// The fp32-verify attention kernel of attention.hip, included once per form by attention_forms.h (no include guard on purpose; the
// forms, their flags and their trailing parameters are described there).  Particular to this kernel:
//   PM_ATTN_SEG   scores of denied keys become -inf in every half-tile, the V^T columns of padding keys (segment 255) are zeroed in
//                 every tile, the running max is raised at every half-tile (no deferred rescale), and a query that has met no allowed
//                 key yet keeps negm = 0
//   PM_ATTN_BIAS  a key whose bias is -inf is padding (255), for the scores and for the V^T zeroing alike
template <bool EXP2, int QF>
__global__ __launch_bounds__(THREADS, 2) void PM_ATTN_KERNEL(const float* __restrict__ Q, const float* __restrict__ Kp,
                                                            const float* __restrict__ Vt, float* __restrict__ out,
                                                            int ldo, int heads, int Nq, int Nkv, int Nkv_pad, int nqb
#ifdef PM_ATTN_LENS
                                                            , const int* __restrict__ lens
#endif
#ifdef PM_ATTN_SEG
                                                            , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask
#endif
#ifdef PM_ATTN_BIAS
                                                            , const float* __restrict__ key_bias
#endif
#ifdef PM_ATTN_PICK
                                                            , const unsigned char* __restrict__ pick, int want
#endif
                                                            ) {
    constexpr int TILE_BYTES = KT * ROWB;
    constexpr int STAGE_BYTES = 2 * TILE_BYTES;              // K tile + V^T tile
    constexpr float kDefer = EXP2 ? 8.0f : 0.0f;             // skip the O rescale while the row max grows < 2^8
    __shared__ __attribute__((aligned(16))) unsigned char lds[3 * STAGE_BYTES];   // 3-stage K / V^T ring

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    // 1-D grid.  Workgroup L runs on XCD L % 8 (private 4 MiB L2): give all query blocks of one (batch, head) the
    // same L % 8 so its K / V^T are fetched from HBM once and re-read from that XCD's L2.
    int bh, qblk;
    {
        const int L = blockIdx.x, total_bh = gridDim.x / nqb;
        if ((total_bh & 7) == 0) {
            const int slot = L >> 3;
            qblk = slot % nqb;
            bh = (slot / nqb) * 8 + (L & 7);
        } else {
            qblk = L % nqb;
            bh = L / nqb;
        }
    }
    const int b = bh / heads, h = bh % heads;
    const int q0 = qblk * (4 * QF * 16) + wave * (QF * 16);
#ifdef PM_ATTN_PICK
    // the picked form: a workgroup whose image is not the launch's kind is done here, before any LDS write, DMA
    // request, barrier or store -- workgroup-uniform (b is, and the flag goes through a scalar), so no wave is left at a barrier
    if (__builtin_amdgcn_readfirstlane((int)pick[b]) != want) return;
#endif
#ifdef PM_ATTN_LENS
    {                                                        // workgroup-uniform: this image's key count
        const int n = __builtin_amdgcn_readfirstlane(lens[b]);
        Nkv = n < 1 ? 1 : (n > Nkv ? Nkv : n);
    }
#endif
#ifdef PM_ATTN_SEG
    const unsigned char* segb = key_seg + (size_t)b * Nkv;  // this image's key segments; keys at or beyond Nkv are padding
#ifdef PM_ATTN_BIAS
    const float* biasb = key_bias + (size_t)b * Nkv;         // this image's key biases; -inf = the key is padding
    auto seg_of = [&](int key) -> unsigned { return key < Nkv && biasb[key] != -INFINITY ? (unsigned)segb[key] : 255u; };
    auto bias_of = [&](int key) -> float { return key < Nkv ? biasb[key] : 0.f; };
#else
    auto seg_of = [&](int key) -> unsigned { return key < Nkv ? (unsigned)segb[key] : 255u; };
#endif
    unsigned qmask[QF];                                      // the segments this lane's query of tile qf attends to
#pragma unroll
    for (int qf = 0; qf < QF; ++qf) {
        int q = q0 + qf * 16 + l15;
        q = q < Nq ? q : Nq - 1;
        qmask[qf] = query_mask[(size_t)b * Nq + q];
    }
#endif

    const float* Qbh = Q + (size_t)bh * Nq * DH;
    const unsigned char* Kbh = reinterpret_cast<const unsigned char*>(Kp + (size_t)bh * Nkv_pad * DH);
    const unsigned char* Vbh = reinterpret_cast<const unsigned char*>(Vt + (size_t)bh * DH * Nkv_pad);
    const size_t v_row_bytes = (size_t)Nkv_pad * sizeof(float);

    // Q fragments stay in registers for the whole kernel (column operand of S^T)
    uint4 qreg[QF][NCH];
#pragma unroll
    for (int qf = 0; qf < QF; ++qf) {
        int q = q0 + qf * 16 + l15;
        q = q < Nq ? q : Nq - 1;
        const unsigned char* qrow = reinterpret_cast<const unsigned char*>(Qbh + (size_t)q * DH);
#pragma unroll
        for (int c = 0; c < NCH; ++c) qreg[qf][c] = *reinterpret_cast<const uint4*>(qrow + (c * 4 + g) * 16);
    }

    f32x4_t o[4][QF];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < QF; ++j) o[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float mrun[QF], lrun[QF];            // running max; per-lane partial row sums (reduced at the end)
    // The S^T accumulators START from -m (the running max of their query column) instead of 0, so the MFMA delivers
    // s - m and the softmax needs no subtraction per score.  m is the value at the time the QK^T of a half-tile is
    // issued; the (rare) rescale branch below moves already-computed scores to a new max.  Before the first
    // half-tile m is undefined and the accumulators start from 0.
    f32x4_t negm[QF];
#pragma unroll
    for (int j = 0; j < QF; ++j) { mrun[j] = -INFINITY; lrun[j] = 0.f; negm[j] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }

    const int ntiles = (Nkv + KT - 1) / KT;
    const int nhalves = (Nkv + 31) / 32;                     // 32-key half-tiles that contain at least one valid key
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);

    // S^T of one half-tile: 2 key tiles x QF query tiles
    auto qk_half = [&](f32x4_t (&sd)[2][QF], int hh) {
        const unsigned char* Kl = lds + ((hh >> 1) % 3) * STAGE_BYTES;
        const int pc = hh & 1;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
            for (int qf = 0; qf < QF; ++qf) sd[kk][qf] = negm[qf];
            const int krow = 16 * (2 * pc + kk) + l15;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const uint4 kfrag = lds_chunk(Kl, krow, c * 4 + g);
#pragma unroll
                for (int qf = 0; qf < QF; ++qf) Mma<float>::run(sd[kk][qf], kfrag, qreg[qf][c]);
            }
        }
    };

    // (1) row max of half-tile hh and the rare rescale branch
    auto rowmax_rescale = [&](f32x4_t (&sc)[2][QF], int hh) {
        const int t = hh >> 1, pc = hh & 1, kv0 = t * KT;
#if defined(PM_ATTN_SEG) && defined(PM_ATTN_BIAS)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kv0 + 16 * (2 * pc + kk) + 4 * g + r;
                const unsigned sg = seg_of(key);
                const float kb = bias_of(key);                   // an allowed key's score becomes s + bias: one f32 add, before the maximum
#pragma unroll
                for (int qf = 0; qf < QF; ++qf) {
                    if (!((sg < 32u) & ((qmask[qf] >> (sg & 31u)) & 1u))) sc[kk][qf][r] = -INFINITY;
                    else sc[kk][qf][r] += kb;
                }
            }
#elif defined(PM_ATTN_SEG)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned sg = seg_of(kv0 + 16 * (2 * pc + kk) + 4 * g + r);
#pragma unroll
                for (int qf = 0; qf < QF; ++qf)
                    if (!((sg < 32u) & ((qmask[qf] >> (sg & 31u)) & 1u))) sc[kk][qf][r] = -INFINITY;
            }
#else
        if (kv0 + KT > Nkv) {                                // ragged last tile: mask keys beyond Nkv
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kv0 + 16 * (2 * pc + kk) + 4 * g + r;
                    if (key >= Nkv) {
#pragma unroll
                        for (int qf = 0; qf < QF; ++qf) sc[kk][qf][r] = -INFINITY;
                    }
                }
        }
#endif
        float tmax[QF];                                      // max of (s - mb), mb = what the accumulators started from
        const bool first = (hh == 0);
#ifdef PM_ATTN_SEG
        bool grow = true;                                    // exact at every half-tile: the deferred rescale assumes a max that exists
        (void)first;
#else
        bool grow = first;
#endif
#pragma unroll
        for (int qf = 0; qf < QF; ++qf) {
            float m = vmax3(sc[0][qf][0], sc[0][qf][1], sc[0][qf][2]);
            m = vmax3(m, sc[0][qf][3], sc[1][qf][0]);
            m = vmax3(m, sc[1][qf][1], sc[1][qf][2]);
            m = vmax2(m, sc[1][qf][3]);                      // this lane's 8 keys only: enough to DETECT growth
            tmax[qf] = m;
            grow |= (m > kDefer);
        }
        if (__any(grow)) {                                   // wave-uniform: rescale everything at the old max exactly once
#pragma unroll
            for (int qf = 0; qf < QF; ++qf) {
#ifdef PM_ATTN_SEG
                // mrun = -inf: no allowed key met yet -- negm is 0 (the accumulators started from 0), l = O = 0.  While that lasts
                // nothing is moved, so no exp(-inf - (-inf)) is formed and -inf scores stay -inf.
                const float mb = mrun[qf] == -INFINITY ? 0.f : mrun[qf];
                const float mnew = vmax2(mrun[qf], group4_max(tmax[qf]) + mb);
                if (mnew == -INFINITY) continue;
#else
                const float mb = first ? 0.f : mrun[qf];
                const float mnew = vmax3(mrun[qf], group4_max(tmax[qf]) + mb, -1e30f);   // column max over the 4 lane groups
#endif
                const float alpha = EXP2 ? __builtin_amdgcn_exp2f(mrun[qf] - mnew) : expf(mrun[qf] - mnew);
                const float delta = mb - mnew;               // scores already hold s - mb: move them to s - mnew
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[kk][qf][r] += delta;
                mrun[qf] = mnew;
                negm[qf] = f32x4_t{-mnew, -mnew, -mnew, -mnew};
                lrun[qf] *= alpha;
#pragma unroll
                for (int df = 0; df < 4; ++df) {
                    o[df][qf][0] *= alpha; o[df][qf][1] *= alpha; o[df][qf][2] *= alpha; o[df][qf][3] *= alpha;
                }
            }
        }
    };

    // (2) ONE basic block: the exponentials and row sums of half-tile hh (VALU + transcendental) and, when there is a
    // next half-tile, the MFMAs of its S^T -- independent work the scheduler may interleave.  P stays fp32: the S^T
    // accumulators of a lane are exactly the k-slice the column operand of P.V needs.
    auto exp_and_next_qk = [&](auto has_next_c, f32x4_t (&sc)[2][QF], uint4 (&pfrag)[2][QF], f32x4_t (&sn)[2][QF], int hn) {
        constexpr bool has_next = decltype(has_next_c)::value;      // compile-time: the steady-state region has no branch
        if constexpr (has_next) qk_half(sn, hn);
#pragma unroll
        for (int qf = 0; qf < QF; ++qf) {
            float psum = 0.f;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pv = EXP2 ? __builtin_amdgcn_exp2f(sc[kk][qf][r]) : expf(sc[kk][qf][r]);   // sc = s - m
                    sc[kk][qf][r] = pv;
                    psum += pv;
                }
            lrun[qf] += psum;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                pfrag[kk][qf] = make_uint4(__float_as_uint(sc[kk][qf][0]), __float_as_uint(sc[kk][qf][1]),
                                           __float_as_uint(sc[kk][qf][2]), __float_as_uint(sc[kk][qf][3]));
        }
    };

    // (3) O^T += V^T . P^T for half-tile hh
    auto pv_half = [&](uint4 (&pfrag)[2][QF], int hh) {
        const int t = hh >> 1, pc = hh & 1;
        const unsigned char* Vl = lds + (t % 3) * STAGE_BYTES + TILE_BYTES;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int df = 0; df < 4; ++df) {
                const uint4 vfrag = lds_chunk(Vl, df * 16 + l15, (2 * pc + kk) * 4 + g);
#pragma unroll
                for (int qf = 0; qf < QF; ++qf) Mma<float>::run(o[df][qf], vfrag, pfrag[kk][qf]);
            }
    };

    // entering tile tn (called while the previous tile's second half is still to be consumed): vmcnt(0) says this wave's
    // share of the tile's DMA has landed, the barrier publishes every wave's share; the barrier also proves every wave
    // is done with tile tn-2, whose stage the DMA of tile tn+1 now reuses (3-stage ring)
    auto enter_tile = [&](int tn) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tn + 1 < ntiles) stage_tiles(lds + ((tn + 1) % 3) * STAGE_BYTES, Kbh, Vbh, v_row_bytes, tn + 1, wave_u, lane);
#ifdef PM_ATTN_SEG
        {                                                    // every tile: zero the V^T columns of padding keys (255, or >= Nkv)
            unsigned char* Vl = lds + (tn % 3) * STAGE_BYTES + TILE_BYTES;
            for (int idx = tid; idx < KT * SLOTS; idx += THREADS) {
                const int row = idx / SLOTS, lslot = idx % SLOTS;
                uint4* p = reinterpret_cast<uint4*>(Vl + row * ROWB + ((lslot ^ (row & (SLOTS - 1))) << 4));
                uint4 v = *p;
                const int k0 = tn * KT + lslot * 4;
                if (seg_of(k0 + 0) == 255u) v.x = 0u;
                if (seg_of(k0 + 1) == 255u) v.y = 0u;
                if (seg_of(k0 + 2) == 255u) v.z = 0u;
                if (seg_of(k0 + 3) == 255u) v.w = 0u;
                *p = v;
            }
            __syncthreads();
        }
#else
        if (tn * KT + KT > Nkv) {
            zero_ragged_v(lds + (tn % 3) * STAGE_BYTES + TILE_BYTES, tn * KT, Nkv, tid);
            __syncthreads();
        }
#endif
    };

    stage_tiles(lds, Kbh, Vbh, v_row_bytes, 0, wave_u, lane);
    enter_tile(0);

    // Software pipeline over half-tiles: the MFMAs of S^T(h+1) are independent of the softmax VALU work on S^T(h),
    // so the two interleave inside one wave; two named S buffers alternate (static register indexing).
    f32x4_t sA[2][QF], sB[2][QF];
    uint4 pfrag[2][QF];
    constexpr std::true_type kNext{};
    constexpr std::false_type kLast{};
    qk_half(sA, 0);
    int hs = 0;
    for (; hs + 2 < nhalves; hs += 2) {                                  // steady state: both following halves exist
        rowmax_rescale(sA, hs);
        exp_and_next_qk(kNext, sA, pfrag, sB, hs + 1);                  // S^T(hs+1): same tile, second half
        pv_half(pfrag, hs);
        enter_tile((hs + 2) >> 1);                                      // S^T(hs+2) opens the next tile
        rowmax_rescale(sB, hs + 1);
        exp_and_next_qk(kNext, sB, pfrag, sA, hs + 2);
        pv_half(pfrag, hs + 1);
    }
    if (hs + 1 < nhalves) {                                             // tail: one or two halves left
        rowmax_rescale(sA, hs);
        exp_and_next_qk(kNext, sA, pfrag, sB, hs + 1);
        pv_half(pfrag, hs);
        rowmax_rescale(sB, hs + 1);
        exp_and_next_qk(kLast, sB, pfrag, sA, 0);
        pv_half(pfrag, hs + 1);
    } else {
        rowmax_rescale(sA, hs);
        exp_and_next_qk(kLast, sA, pfrag, sB, 0);
        pv_half(pfrag, hs);
    }

    // ---- finalize: O = O^T / l, head-major inside the output row
    float inv[QF];
#pragma unroll
    for (int qf = 0; qf < QF; ++qf) {      // cross-lane steps first, outside any divergent region
#ifdef PM_ATTN_SEG
        const float lsum = group4_sum(lrun[qf]);
        inv[qf] = lsum > 0.f ? 1.0f / lsum : 0.f;            // (a query with no allowed key: a finite row)
#else
        inv[qf] = 1.0f / group4_sum(lrun[qf]);
#endif
    }
#pragma unroll
    for (int qf = 0; qf < QF; ++qf) {
        const int q = q0 + qf * 16 + l15;
        if (q < Nq) {
            float* orow = out + ((size_t)b * Nq + q) * ldo + h * DH;
#pragma unroll
            for (int df = 0; df < 4; ++df)
                store4(orow + df * 16 + g * 4, o[df][qf][0] * inv[qf], o[df][qf][1] * inv[qf],
                       o[df][qf][2] * inv[qf], o[df][qf][3] * inv[qf]);
        }
    }
}
