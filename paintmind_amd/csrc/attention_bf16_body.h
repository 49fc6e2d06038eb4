// The bf16 attention kernel of attention_bf16.hip, included once per form by attention_forms.h (no include guard on purpose; the
// forms, their flags and their trailing parameters are described there, and so is why the body is text).  Particular to this kernel:
//   PM_ATTN_LENS  everything below the clamp -- tile counts, the ragged-tile K mask, the V^T zeroing, steady_end / all_steady -- uses
//                 the per-image value; every base and row stride is unchanged and every read stays inside Nkv_pad
//   PM_ATTN_SEG   every half-tile takes the exact path: the mask sits where the ragged-tile mask sets scores to -inf, the V^T
//                 columns of padding keys are zeroed in every tile, and the running max of a query that has not met an allowed key
//                 yet stays "none" (negm 0, l 0) instead of -inf
//   PM_ATTN_BIAS  the running max is a max over s + bias; a key whose bias is -inf is padding (255) in seg_of, for the scores and
//                 for the V^T zeroing alike
template <bool EXP2, int QF>
__global__ __launch_bounds__(THREADS, 2) void PM_ATTN_KERNEL(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ Kp,
                                                                    const bf16_t* __restrict__ Vt, bf16_t* __restrict__ out,
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
    __shared__ __attribute__((aligned(16))) unsigned char lds[RING * STAGE_BYTES];   // K / V^T ring

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    // 1-D grid.  Workgroup L runs on XCD L % 8 (private 4 MiB L2): give all query blocks of one (batch, head) the
    // same L % 8 so its K / V^T (256 KiB) are fetched from HBM once and re-read from that XCD's L2.
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
    const unsigned char* segb = key_seg + (size_t)b * Nkv;  // this image's key segments
#ifdef PM_ATTN_BIAS
    const float* biasb = key_bias + (size_t)b * Nkv;         // this image's key biases; -inf = the key is padding
    auto seg_of = [&](int key) -> unsigned { return key < Nkv && biasb[key] != -INFINITY ? (unsigned)segb[key] : 255u; };
    auto bias_of = [&](int key) -> float { return key < Nkv ? biasb[key] : 0.f; };
#else
    // segment of key `key` of this image; keys at or beyond Nkv are padding
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

    const bf16_t* Qbh = Q + (size_t)bh * Nq * DH;
    const unsigned char* Kbh = reinterpret_cast<const unsigned char*>(Kp + (size_t)bh * Nkv_pad * DH);
    const unsigned char* Vbh = reinterpret_cast<const unsigned char*>(Vt + (size_t)bh * DH * Nkv_pad);
    const unsigned v_row_bytes = (unsigned)Nkv_pad * 2u;
    // DMA descriptors / lane offsets, and the per-lane parts of the fragment addresses (ds_read_b128 with immediate offsets)
    //   K row of S^T tile kf = 2 pc + kk, row i = l15:  32 pc + 8 (l15 >> 2) + 4 kk + (l15 & 3);  slot (4 c + g) ^ (row & 7)
    //     = stage + [8 (l15 >> 2) + (l15 & 3)] * 128 + (g ^ (l15 & 3)) * 16  +  pc * 4096 + kk * 512 + (c ^ kk) * 64
    //     (round 5: slot additionally ^ 4 where bit 3 of the row is set, i.e. "+ (c ^ kk ^ ((l15 >> 2) & 1)) * 64")
    //   V^T row 16 df + l15, slot (4 pc + g) ^ (l15 & 7)
    //     = stage + 8192 + l15 * 128 + ((4 pc + g) ^ (l15 & 7)) * 16  +  df * 2048
    const rsrc_t Kr = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(Kbh), 0, 0x7fffffff, 0x00020000);
    const rsrc_t Vr = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(Vbh), 0, 0x7fffffff, 0x00020000);
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
    const unsigned lslot = (unsigned)(((lane & 7) ^ ((lane >> 3) & 7)) << 4);
    const unsigned kvoff = (unsigned)(lane >> 3) * 128u + lslot;
    // K tile, bank conflicts (round 5): a ds_read_b128 is served 16 lanes at a time ({0-3, 12-15, 20-27}, ...), and the S^T row
    // order puts l15 = 0..3 and 12..15 on rows 0..3 and 24..27 -- same row & 7, same slot: a 2-way conflict on every K fragment
    // read (SQ_LDS_BANK_CONFLICT a third of SQ_LDS_IDX_ACTIVE).  Bit 3 of the row now flips bit 2 of the slot as well: the odd
    // 8-row chunks are DMA'd with the flipped source slot, and the read side flips it for the lanes with (l15 >> 2) odd.
    const unsigned kvoff1 = PM_ATTN_KSWZ ? kvoff ^ 64u : kvoff;
    const unsigned vvoff = (unsigned)(lane >> 3) * v_row_bytes + lslot;
    const unsigned kfrag_lane = lds_base + (unsigned)(8 * (l15 >> 2) + (l15 & 3)) * 128u + (unsigned)((g ^ (l15 & 3)) << 4) +
                                (PM_ATTN_KSWZ ? (unsigned)(((l15 >> 2) & 1) << 6) : 0u);          // slots with c ^ kk = 0
    const unsigned kfrag_laneB = kfrag_lane ^ 64u;                                                 // slots with c ^ kk = 1
    const unsigned vfrag_lane0 = lds_base + 8192u + (unsigned)l15 * 128u + (unsigned)(((0 + g) ^ (l15 & 7)) << 4);
    const unsigned vfrag_lane1 = lds_base + 8192u + (unsigned)l15 * 128u + (unsigned)(((4 + g) ^ (l15 & 7)) << 4);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int q0u = qblk * (4 * QF * 16) + wave_u * (QF * 16);       // q0, provably wave-uniform

    // one K tile + one V^T tile by DMA, 1 KiB per wave-instruction; the bank swizzle (slot ^ row) is applied to the SOURCE
    // address (kvoff / vvoff) and again on the read side
    auto stage_tiles = [&](int t) {
        unsigned char* stage = lds + (t % RING) * STAGE_BYTES;
        const unsigned kv0 = (unsigned)t * KT;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const unsigned chunk = (unsigned)wave_u * 2 + i;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(Kr, (__attribute__((address_space(3))) void*)(stage + chunk * 1024), 16, i ? kvoff1 : kvoff,
                                                     (kv0 + chunk * 8) * 128u, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(Vr, (__attribute__((address_space(3))) void*)(stage + KT * 128 + chunk * 1024), 16, vvoff,
                                                     chunk * 8 * v_row_bytes + kv0 * 2u, 0, 0);
        }
    };

    // Q fragments stay in registers for the whole kernel (column operand of S^T)
    v4u_t qreg[QF][2];
#pragma unroll
    for (int qf = 0; qf < QF; ++qf) {
        int q = q0 + qf * 16 + l15;
        q = q < Nq ? q : Nq - 1;
        const unsigned char* qrow = reinterpret_cast<const unsigned char*>(Qbh + (size_t)q * DH);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if constexpr (ABL & 64) { (void)qrow; qreg[qf][c] = v4u_t{0x3c003c00u + lane, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u}; }
            else qreg[qf][c] = *reinterpret_cast<const v4u_t*>(qrow + (c * 4 + g) * 16);
        }
    }

    f32x4_t o[4][QF];
    f32x4_t lacc[QF];                    // every element = l of the query column (sum of bf16 P, by MFMA with a ones operand)
    f32x4_t negm[QF];                    // -m (reference max of the query column) x4: the C operand of the S^T MFMAs
    v4u_t ones = v4u_t{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
    asm volatile("" : "+v"(ones));       // keep it in registers (not re-materialised in front of every use)

    const int ntiles = (Nkv + KT - 1) / KT;
    const int nhalves = (Nkv + 31) / 32;                     // 32-key half-tiles that contain at least one valid key

    auto k_issue = [&](v4u_t (&kf)[2][2], int hh) {
        const unsigned so = (unsigned)((hh >> 1) % RING) * STAGE_BYTES + (unsigned)(hh & 1) * 4096u;
        const unsigned ka = kfrag_lane + so, kb = kfrag_laneB + so;
        DSRX(kf[0][0], ka, 0 * 512); DSRX(kf[0][1], kb, 0 * 512);
        DSRX(kf[1][0], kb, 1 * 512); DSRX(kf[1][1], ka, 1 * 512);
    };
    auto v_issue = [&](v4u_t (&vf)[4], int hh) {
        const unsigned va = ((hh & 1) ? vfrag_lane1 : vfrag_lane0) + (unsigned)((hh >> 1) % RING) * STAGE_BYTES;
        DSRX(vf[0], va, 0 * 2048); DSRX(vf[1], va, 1 * 2048); DSRX(vf[2], va, 2 * 2048); DSRX(vf[3], va, 3 * 2048);
    };

    // S^T of one half-tile, starting from -m
    auto qk = [&](f32x4_t (&sd)[2][QF], v4u_t (&kf)[2][2]) {
#pragma unroll
        for (int qf = 0; qf < QF; ++qf) sd[0][qf] = mma(kf[0][0], qreg[qf][0], negm[qf]);
#pragma unroll
        for (int qf = 0; qf < QF; ++qf) sd[0][qf] = mma(kf[0][1], qreg[qf][1], sd[0][qf]);
#pragma unroll
        for (int qf = 0; qf < QF; ++qf) sd[1][qf] = mma(kf[1][0], qreg[qf][0], negm[qf]);
#pragma unroll
        for (int qf = 0; qf < QF; ++qf) sd[1][qf] = mma(kf[1][1], qreg[qf][1], sd[1][qf]);
    };

    // rare, wave-uniform: mask a ragged last tile, raise the running max, rescale everything at the old max exactly once
    auto rescale = [&](auto ragged_c, auto first_c, f32x4_t (&sc)[2][QF], int hh) {
        constexpr bool first = decltype(first_c)::value;
        const int kv0 = (hh >> 1) * KT, pc = hh & 1;
#if defined(PM_ATTN_SEG) && defined(PM_ATTN_BIAS)
        // every half-tile: an allowed key's score becomes s + bias (one f32 add, before the maximum below), a denied one -inf
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kv0 + 32 * pc + 8 * g + 4 * kk + r;
                const unsigned sg = seg_of(key);
                const float kb = bias_of(key);
#pragma unroll
                for (int qf = 0; qf < QF; ++qf) {
                    if (!((sg < 32u) & ((qmask[qf] >> (sg & 31u)) & 1u))) sc[kk][qf][r] = -INFINITY;
                    else sc[kk][qf][r] += kb;
                }
            }
#elif defined(PM_ATTN_SEG)
        // every half-tile: a key takes part in a query's softmax iff its segment is one the query attends to (padding, 255, never)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned sg = seg_of(kv0 + 32 * pc + 8 * g + 4 * kk + r);
#pragma unroll
                for (int qf = 0; qf < QF; ++qf)
                    if (!((sg < 32u) & ((qmask[qf] >> (sg & 31u)) & 1u))) sc[kk][qf][r] = -INFINITY;
            }
#else
        if (decltype(ragged_c)::value && kv0 + KT > Nkv) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kv0 + 32 * pc + 8 * g + 4 * kk + r;
                    if (key >= Nkv) {
#pragma unroll
                        for (int qf = 0; qf < QF; ++qf) sc[kk][qf][r] = -INFINITY;
                    }
                }
        }
#endif
#pragma unroll
        for (int qf = 0; qf < QF; ++qf) {
            float m = vmax3(sc[0][qf][0], sc[0][qf][1], sc[0][qf][2]);
            m = vmax3(m, sc[0][qf][3], sc[1][qf][0]);
            m = vmax3(m, sc[1][qf][1], sc[1][qf][2]);
            m = vmax2(m, sc[1][qf][3]);                      // this lane's 8 keys, relative to mb
#ifdef PM_ATTN_SEG
            // A query that has met no allowed key yet has l = 0 (the key at a running max contributes exactly 1) and keeps negm = 0:
            // its accumulators start from 0 as in the first half-tile, and there is no old max to rescale from.  While that
            // lasts nothing is moved: -inf scores stay -inf, and no exp(-inf - (-inf)) is ever formed.
            const bool none = first || lacc[qf][0] == 0.f;
            const float mold = none ? -INFINITY : -negm[qf][0];
            const float mb = none ? 0.f : mold;
            const float mnew = vmax3(mold, group4_max(m) + mb, -1e30f);
            if (mnew <= -1e30f) continue;                    // every key of this half-tile denied, and none allowed before it
#else
            const float mold = first ? -INFINITY : -negm[qf][0];
            const float mb = first ? 0.f : mold;             // what the accumulators started from
            const float mnew = vmax3(mold, group4_max(m) + mb, -1e30f);   // column max over the 4 lane groups
#endif
            const float delta = mb - mnew;                   // scores hold s - mb: move them to s - mnew
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[kk][qf][r] += delta;
            // -m moves by the same delta, component by component and in place (a quad rebuilt from one scalar costs the
            // COMMON path a copy of all of negm at the join)
            if constexpr (first) {
                negm[qf][0] = delta; negm[qf][1] = delta; negm[qf][2] = delta; negm[qf][3] = delta;
            } else {
                negm[qf][0] += delta; negm[qf][1] += delta; negm[qf][2] += delta; negm[qf][3] += delta;
            }
            if constexpr (!first) {                          // (the first half-tile finds l = O = 0: nothing to move)
                const float alpha = EXP2 ? __builtin_amdgcn_exp2f(mold - mnew) : expf(mold - mnew);
                lacc[qf][0] *= alpha; lacc[qf][1] *= alpha; lacc[qf][2] *= alpha; lacc[qf][3] *= alpha;
#pragma unroll
                for (int df = 0; df < 4; ++df) {
                    o[df][qf][0] *= alpha; o[df][qf][1] *= alpha; o[df][qf][2] *= alpha; o[df][qf][3] *= alpha;
                }
            }
        }
    };

    // entering tile tn (called while the previous tile's second half is still to be consumed): its DMA has landed
    // and is published by the barrier; the barrier also proves every wave is done with tile tn-2, whose stage the
    // DMA of tile tn+AHEAD now reuses (RING stages: tn-2 and tn+AHEAD share one)
    auto enter_tile = [&](auto ragged_c, int tn) {
        if (!(ABL & 8) || tn == 0) {
            // this wave's pieces of tile tn have landed: everything but the pieces of the younger tiles in flight behind them
            // (4 instructions per tile; vmcnt retires in issue order)
            // The barrier is the bare instruction: __syncthreads() carries a fence, for which hipcc drains vmcnt to 0 -- that
            // would wait for the younger tile as well.  Nothing else needs the fence here: the fast path reads LDS with
            // inline-asm ds_read only, and the exact path's V^T patch below is followed by a full __syncthreads().
            if (AHEAD == 2 && tn + 1 < ntiles) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        if (tn + AHEAD < ntiles && !(ABL & 4)) stage_tiles(tn + AHEAD);
#ifdef PM_ATTN_SEG
        if (decltype(ragged_c)::value) {                         // every tile: zero the V^T columns of padding keys (255, or >= Nkv)
            unsigned char* Vl = lds + (tn % RING) * STAGE_BYTES + TILE_BYTES;
            for (int idx = tid; idx < KT * 8; idx += THREADS) {
                const int row = idx / 8, ls = idx % 8;
                uint4* p = reinterpret_cast<uint4*>(Vl + row * 128 + ((ls ^ (row & 7)) << 4));
                uint4 v = *p;
                const int k0 = tn * KT + ls * 8;                 // first key of this 8-key chunk
                unsigned keep[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) keep[e] = seg_of(k0 + e) == 255u ? 0u : 0xffffu;
                v.x &= keep[0] | (keep[1] << 16);
                v.y &= keep[2] | (keep[3] << 16);
                v.z &= keep[4] | (keep[5] << 16);
                v.w &= keep[6] | (keep[7] << 16);
                *p = v;
            }
            __syncthreads();
        }
#else
        if (decltype(ragged_c)::value && tn * KT + KT > Nkv) {   // ragged last tile: zero the V^T columns of keys >= Nkv
            unsigned char* Vl = lds + (tn % RING) * STAGE_BYTES + TILE_BYTES;
            for (int idx = tid; idx < KT * 8; idx += THREADS) {
                const int row = idx / 8, ls = idx % 8;
                uint4* p = reinterpret_cast<uint4*>(Vl + row * 128 + ((ls ^ (row & 7)) << 4));
                uint4 v = *p;
                const int n = Nkv - (tn * KT + ls * 8);      // valid keys in this 8-key chunk (may be <= 0)
                v.x = n <= 0 ? 0u : (n == 1 ? (v.x & 0xffffu) : v.x);
                v.y = n <= 2 ? 0u : (n == 3 ? (v.y & 0xffffu) : v.y);
                v.z = n <= 4 ? 0u : (n == 5 ? (v.z & 0xffffu) : v.z);
                v.w = n <= 6 ? 0u : (n == 7 ? (v.w & 0xffffu) : v.w);
                *p = v;
            }
            __syncthreads();
        }
#endif
    };

    f32x4_t sA[2][QF];                   // S^T of ONE half-tile (single-buffered: group g of a step overwrites the tile it has consumed)
    v4u_t pf[QF];
    v4u_t kf[2][2], vf[4];

    // exponentials of the 16-query tile qf of S^T(h) and their packing into the P^T operand; S^T itself is left as it is
    auto exp_pack1 = [&](f32x4_t (&sc)[2][QF], int qf) {
        float e[2][4];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                e[kk][r] = (ABL & 1) ? sc[kk][qf][r] * 1.0001f : (EXP2 ? __builtin_amdgcn_exp2f(sc[kk][qf][r]) : expf(sc[kk][qf][r]));   // sc = s - m
        pf[qf] = v4u_t{pack_bf16x2(e[0][0], e[0][1]), pack_bf16x2(e[0][2], e[0][3]), pack_bf16x2(e[1][0], e[1][1]), pack_bf16x2(e[1][2], e[1][3])};
    };
    // P.V and the row sums of one half-tile (exact path)
    auto pv_all = [&]() {
#pragma unroll
        for (int df = 0; df < 4; ++df)
#pragma unroll
            for (int qf = 0; qf < QF; ++qf) o[df][qf] = mma(vf[df], pf[qf], o[df][qf]);
#pragma unroll
        for (int qf = 0; qf < QF; ++qf) lacc[qf] = mma(ones, pf[qf], lacc[qf]);
    };

    // One half-tile h of the FAST path, query-tile-major.  On entry sA = S^T(h) - m_ref (tiles 1..3 untouched, tile 0 already
    // turned into pf[0]), the K fragments of h+1 and then the V^T fragments of h are in flight (in that order).  Group g:
    //     matrix:  S^T(h+1, g) = K(h+1) Q_g - m_ref   (4 MFMAs, overwrites S^T(h, g))
    //              O^T(., g) += V^T(h) P(h, g),  l_g += 1 P(h, g)                    (5 MFMAs)
    //     vector:  P(h, g+1) = bf16(exp2(S^T(h, g+1)))  -- for g = 3: P(h+1, 0), from the S^T(h+1, 0) of this step's group 0
    // The K fragments of h+2 are requested behind the last QK^T MFMA, the V^T fragments of h+1 behind the last P.V MFMA.
    //   OPENS: h+2 is the first half of a new tile
    auto grp_mma = [&](f32x4_t (&sc)[2][QF], int g) {
        sc[0][g] = mma(kf[0][0], qreg[g][0], negm[g]);
        sc[1][g] = mma(kf[1][0], qreg[g][0], negm[g]);
        sc[0][g] = mma(kf[0][1], qreg[g][1], sc[0][g]);
        sc[1][g] = mma(kf[1][1], qreg[g][1], sc[1][g]);
    };
    auto grp_pv = [&](int g) {
#pragma unroll
        for (int df = 0; df < 4; ++df) o[df][g] = mma(vf[df], pf[g], o[df][g]);
        lacc[g] = mma(ones, pf[g], lacc[g]);
    };
    auto grp_sched = [&](bool last) {                        // 9 MFMAs, 8 transcendentals, 4 packs: M T T M P  x4, M  (last group: M T T P)
        if constexpr (EXP2 && !(ABL & 1)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x400, 2, 0);
                if (!last) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        }
    };
    auto step = [&](auto opens_c, f32x4_t (&sc)[2][QF], int hh) {
        constexpr bool OPENS = decltype(opens_c)::value;
        const unsigned va = (((hh + 1) & 1) ? vfrag_lane1 : vfrag_lane0) + (unsigned)(((hh + 1) >> 1) % RING) * STAGE_BYTES;
        const unsigned kso = (unsigned)(((hh + 2) >> 1) % RING) * STAGE_BYTES + (unsigned)(hh & 1) * 4096u;
        const unsigned ka = kfrag_lane + kso, kb = kfrag_laneB + kso;
#pragma unroll
        for (int g = 0; g < QF; ++g) {
            const bool last = g == QF - 1;
            if (OPENS && last) enter_tile(std::false_type{}, (hh + 2) >> 1);
            if (g == 0) LGKM4(4, kf[0][0], kf[0][1], kf[1][0], kf[1][1]);          // K(h+1) landed; the V^T(h) reads are younger
            grp_mma(sc, g);
            if (last) {                                       // the fragment registers are handed over to the next half-tile as they die
                __builtin_amdgcn_sched_barrier(0);
                DSRX(kf[0][0], ka, 0 * 512); DSRX(kf[0][1], kb, 0 * 512);
                DSRX(kf[1][0], kb, 1 * 512); DSRX(kf[1][1], ka, 1 * 512);
            }
            if (g == 0) {
                if (last) LGKM4(4, vf[0], vf[1], vf[2], vf[3]);                     // (QF = 1: the K(h+2) reads just issued stay in flight)
                else LGKM4(0, vf[0], vf[1], vf[2], vf[3]);
            }
            grp_pv(g);
            exp_pack1(sc, (g + 1) % QF);                      // last group: P(h+1, 0), from the S^T(h+1, 0) of this step's group 0
            grp_sched(last);
            asm volatile("" : "+v"(pf[(g + 1) % QF]));            // the packs are complete here (not sunk to their first use)
            __builtin_amdgcn_sched_barrier(0);
            if (last) { DSRX(vf[0], va, 0 * 2048); DSRX(vf[1], va, 1 * 2048); DSRX(vf[2], va, 2 * 2048); DSRX(vf[3], va, 3 * 2048); }
        }
    };

    // The exact path, one half-tile with every condition at run time, full waits and the running max raised at once: first and
    // last tiles, ragged tiles, short contexts, and a workgroup the fast path gave up on.  sA: S^T(h) -> P(h) -> S^T(h+1).
    auto slow_step = [&](int hh) {
        const bool next = hh + 1 < nhalves, next2 = hh + 2 < nhalves;
#pragma unroll
        for (int qf = 0; qf < QF; ++qf) exp_pack1(sA, qf);
        v_issue(vf, hh);
        if (next) {
            LGKM4(4, kf[0][0], kf[0][1], kf[1][0], kf[1][1]);
            qk(sA, kf);
        }
        if (next2 && !(hh & 1)) enter_tile(std::true_type{}, (hh + 2) >> 1);
        if (next2) k_issue(kf, hh + 2);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vf[0]), "+v"(vf[1]), "+v"(vf[2]), "+v"(vf[3]), "+v"(kf[0][0]), "+v"(kf[0][1]),
                     "+v"(kf[1][0]), "+v"(kf[1][1]));
        pv_all();
        if (next) rescale(std::true_type{}, std::false_type{}, sA, hh + 1);
    };

    constexpr std::true_type Y{};
    constexpr std::false_type N{};
    __shared__ int redo_vote[4];

    const int nh_full = 2 * (Nkv / KT);                      // half-tiles that lie in full tiles
    // A context without a ragged tile (self-attention: every stage-2 / ViT launch of the decode loop) runs ALL its half-tiles,
    // the last two included, through the fast step.  Past the end `step` still computes S^T(h+1) and prefetches K(h+2) / V^T(h+1):
    // they address ring stages that still hold already-consumed tiles (no DMA is issued past the last tile), and nothing they
    // produce is consumed.
    const bool all_steady = (Nkv % KT) == 0 && ntiles >= 3;
    const int steady_end = all_steady ? nhalves - 1 : min(nhalves - 3, nh_full - 2);   // one bound: the loop's shape is unchanged
#ifdef PM_ATTN_SEG
    bool exact = true;                                       // the lagged-max fast path was built for unmasked tiles
#else
    bool exact = steady_end <= 0;                            // workgroup-uniform: no fast step at all, or second attempt
#endif
    unsigned redo_mask = ~0u;                                // tiles the exact attempt stores (all, unless it is a second attempt)

    // O = O^T / l, head-major inside the output row, for the 16-query tiles in `mask`.  The wave's output rows go through the
    // (idle) K / V^T ring, so that every global store instruction writes 8 whole 128-byte rows (non-temporal)
    auto finalize = [&](unsigned mask) {
        constexpr int RS = 144;                              // staged row: 64 bf16 + pad, 16-B aligned, conflict-free
        unsigned char* obuf = lds + wave * (QF * 16 * RS);
#pragma unroll
        for (int qf = 0; qf < QF; ++qf) {
#ifdef PM_ATTN_SEG
            const float inv = lacc[qf][0] > 0.f ? 1.0f / lacc[qf][0] : 0.f;      // (a query with no allowed key: a finite row)
#else
            const float inv = 1.0f / lacc[qf][0];
#endif
#pragma unroll
            for (int df = 0; df < 4; ++df)
                *reinterpret_cast<uint2*>(obuf + (qf * 16 + l15) * RS + (df * 16 + g * 4) * 2) =
                    make_uint2(pack_bf16x2(o[df][qf][0] * inv, o[df][qf][1] * inv), pack_bf16x2(o[df][qf][2] * inv, o[df][qf][3] * inv));
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // wave-uniform 64-bit base + one 32-bit lane offset: nothing lane-dependent and 64 bits wide for the compiler to hoist to
        // the kernel entry and spill around the loop
        unsigned char* rowbase = reinterpret_cast<unsigned char*>(out + ((size_t)b * Nq + q0u) * ldo + h * DH);
        unsigned lane_off = ((unsigned)(lane >> 3) * (unsigned)ldo + (unsigned)(lane & 7) * 8u) * 2u;
        unsigned rd_off = (unsigned)(lane >> 3) * RS + (unsigned)(lane & 7) * 16u;
        // (this lambda sits inside the attempt loop: without the opaque moves the per-row addresses are loop-invariant, get hoisted
        // to the kernel entry -- 30 registers -- and are spilled around the K loop)
        asm volatile("" : "+v"(lane_off), "+v"(rd_off));
#pragma unroll
        for (int it = 0; it < QF * 2; ++it) {                // 8 rows x 128 B per store instruction
            const int q = q0 + it * 8 + (lane >> 3);
            if (q < Nq && ((mask >> (it >> 1)) & 1u) && (!(ABL & 32) || q < 0)) {
                const v4u_t v = *reinterpret_cast<const v4u_t*>(obuf + rd_off + it * 8 * RS);
                v4u_t* dst = reinterpret_cast<v4u_t*>(rowbase + (lane_off + (unsigned)(it * 8) * (unsigned)ldo * 2u));
                if constexpr (QF == 4) __builtin_nontemporal_store(v, dst);   // large launches stream their output past the caches;
                else *dst = v;                                                 // a small one is read at once by the next kernel of the chain
            }
        }
    };

    for (;;) {
#pragma unroll
        for (int j = 0; j < QF; ++j) {
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            lacc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            negm[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        stage_tiles(0);
        if (AHEAD == 2 && ntiles > 1) stage_tiles(1);
        enter_tile(Y, 0);
        k_issue(kf, 0);
        LGKM4(0, kf[0][0], kf[0][1], kf[1][0], kf[1][1]);
        qk(sA, kf);
        rescale(Y, Y, sA, 0);                                // m_ref = the maximum over the first 32 keys
        if (nhalves > 1) k_issue(kf, 1);

        int hs = 0;
#ifndef PM_ATTN_SEG
        if (!exact) {
            v_issue(vf, 0);
            exp_pack1(sA, 0);
            for (; hs < steady_end; hs += 2) {               // fast path
                step(Y, sA, hs);
                step(N, sA, hs + 1);
            }
            LGKM4(0, kf[0][0], kf[0][1], kf[1][0], kf[1][1]);    // the reads of the last step are not left outstanding
            LGKM4(0, vf[0], vf[1], vf[2], vf[3]);
            // hand-over to the exact steps: sA = S^T(hs) with tiles 1..3 untouched (tile 0 is exponentiated again, same bits), K(hs+1) in kf
        }
#else
        (void)step; (void)N; (void)steady_end;               // the fast path is not part of this form
#endif
#ifdef PM_ATTN_COUNT
        if (lane == 0) { atomicAdd(&g_attn_counters[1], (unsigned long long)hs); atomicAdd(&g_attn_counters[2], (unsigned long long)(nhalves - hs)); }
#endif
        for (; hs < nhalves; ++hs) slow_step(hs);

        // every wave is done reading the ring; and the vote: did a probability of the fast path leave the f32 range?
        unsigned badmask = 0;                                // wave-uniform: bit qf = tile qf of this wave overflowed
        if (!exact && !(ABL & 6)) {                          // (ablations that compute garbage do not vote)
#pragma unroll
            for (int qf = 0; qf < QF; ++qf) badmask |= __any(!(lacc[qf][0] < 1.8446744e19f)) ? (1u << qf) : 0u;     // 2^64; NaN fails too
            if (lane == 0) redo_vote[wave] = (int)badmask;
        }
        __syncthreads();
        if (exact) break;
        const int4 votes = *reinterpret_cast<const int4*>(redo_vote);
        if (__builtin_expect(__builtin_amdgcn_readfirstlane(votes.x | votes.y | votes.z | votes.w) == 0, 1)) break;
        // Rare: some 16-query tile of this workgroup overflowed.  The good tiles are stored now, from the fast path (a tile's
        // result never depends on its neighbours); the workgroup then runs again through the exact path and stores the others.
        if (tid == 0) atomicAdd(&g_attn_fallbacks, 1ull);
        finalize(~badmask);
        redo_mask = badmask;
        exact = true;                                        // (the exact attempt does not vote: no write races the read above)
        __syncthreads();                                     // the staging area is the ring: every wave has read its rows back
    }
    finalize(redo_mask);                                     // the common case: every tile, straight from the fast path
}
