// The fp32-verify attention kernel of attention.hip, which includes this file TWICE (no include guard on purpose), exactly as
// attention_bf16.hip includes attention_bf16_body.h -- see there: PM_ATTN_KERNEL names the kernel, PM_ATTN_LENS_PARAM is empty or
// ", const int* lens", and with PM_ATTN_LENS the key count is lens[b], read once per workgroup and clamped to [1, Nkv].
template <typename T, bool EXP2, int QF>
__global__ __launch_bounds__(THREADS, 2) void PM_ATTN_KERNEL(const T* __restrict__ Q, const T* __restrict__ Kp,
                                                            const T* __restrict__ Vt, T* __restrict__ out,
                                                            int ldo, int heads, int Nq, int Nkv, int Nkv_pad, int nqb PM_ATTN_LENS_PARAM) {
    using C = AttnCfg<T>;
    constexpr int TILE_BYTES = KT * C::ROWB;
    constexpr int STAGE_BYTES = 2 * TILE_BYTES;              // K tile + V^T tile
    constexpr float kDefer = EXP2 ? 8.0f : 0.0f;             // skip the O rescale while the row max grows < 2^8
    __shared__ __attribute__((aligned(16))) unsigned char lds[3 * STAGE_BYTES];   // 3-stage K / V^T ring

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    // 1-D grid.  Workgroup L runs on XCD L % 8 (private 4 MiB L2): give all query blocks of one (batch, head) the
    // same L % 8 so its K / V^T (256 KiB in bf16) are fetched from HBM once and re-read from that XCD's L2.
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
#ifdef PM_ATTN_LENS
    {                                                        // workgroup-uniform: this image's key count
        const int n = __builtin_amdgcn_readfirstlane(lens[b]);
        Nkv = n < 1 ? 1 : (n > Nkv ? Nkv : n);
    }
#endif

    const T* Qbh = Q + (size_t)bh * Nq * DH;
    const unsigned char* Kbh = reinterpret_cast<const unsigned char*>(Kp + (size_t)bh * Nkv_pad * DH);
    const unsigned char* Vbh = reinterpret_cast<const unsigned char*>(Vt + (size_t)bh * DH * Nkv_pad);
    const size_t v_row_bytes = (size_t)Nkv_pad * sizeof(T);
    // bf16: DMA descriptors / lane offsets, and the per-lane parts of the fragment addresses.  Fragment reads are inline-asm
    // ds_read_b128 with immediate offsets: with C++ LDS reads hipcc puts `s_waitcnt vmcnt(0)` in front of the first read
    // after the DMA issue, i.e. it waits for the NEXT tile's DMA right after issuing it (measured: 200 -> 171 us with the
    // DMA removed).  The explicit vmcnt(0) + barrier in enter_tile() is what orders reads after the DMA that fed them.
    //   K row of S^T tile kf = 2 pc + kk, row i = l15:  32 pc + 8 (l15 >> 2) + 4 kk + (l15 & 3);  slot (4 c + g) ^ (row & 7)
    //     = stage + [8 (l15 >> 2) + (l15 & 3)] * 128 + (g ^ (l15 & 3)) * 16  +  pc * 4096 + kk * 512 + (c ^ kk) * 64
    //   V^T row 16 df + l15, slot (4 pc + g) ^ (l15 & 7)
    //     = stage + 8192 + l15 * 128 + ((4 pc + g) ^ (l15 & 7)) * 16  +  df * 2048
    [[maybe_unused]] rsrc_t Kr, Vr;
    [[maybe_unused]] unsigned kvoff = 0, vvoff = 0, kfrag_lane = 0, vfrag_lane0 = 0, vfrag_lane1 = 0;
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
    if constexpr (sizeof(T) == 2) {
        Kr = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(Kbh), 0, 0x7fffffff, 0x00020000);
        Vr = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(Vbh), 0, 0x7fffffff, 0x00020000);
        const unsigned lslot = (unsigned)(((lane & 7) ^ ((lane >> 3) & 7)) << 4);
        kvoff = (unsigned)(lane >> 3) * 128u + lslot;
        vvoff = (unsigned)(lane >> 3) * (unsigned)v_row_bytes + lslot;
        kfrag_lane = lds_base + (unsigned)(8 * (l15 >> 2) + (l15 & 3)) * 128u + (unsigned)((g ^ (l15 & 3)) << 4);
        vfrag_lane0 = lds_base + 8192u + (unsigned)l15 * 128u + (unsigned)(((0 + g) ^ (l15 & 7)) << 4);
        vfrag_lane1 = lds_base + 8192u + (unsigned)l15 * 128u + (unsigned)(((4 + g) ^ (l15 & 7)) << 4);
    }
    typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
#define DSRX(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
    // the wait names the fragments as in/out operands, so every MFMA that consumes one is ordered behind it
#define LGKM_N(n, f) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(f))

    // Q fragments stay in registers for the whole kernel (column operand of S^T)
    uint4 qreg[QF][C::NCH];
#pragma unroll
    for (int qf = 0; qf < QF; ++qf) {
        int q = q0 + qf * 16 + l15;
        q = q < Nq ? q : Nq - 1;
        const unsigned char* qrow = reinterpret_cast<const unsigned char*>(Qbh + (size_t)q * DH);
#pragma unroll
        for (int c = 0; c < C::NCH; ++c) qreg[qf][c] = *reinterpret_cast<const uint4*>(qrow + (c * 4 + g) * 16);
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
    constexpr int LOADS_PER_TILE = 2 * ((KT / (1024 / C::ROWB)) / 4);   // DMA instructions per wave per tile (K + V^T)

    // bf16: issue the 4 K-fragment reads of half-tile hh ([kk][c]); they are waited for, one by one, in front of the MFMAs that
    // consume them (qk_half), so whatever the caller puts in between runs under their LDS latency.  Counted lgkmcnt is exact
    // here because LDS operations return in order and the loop has no scalar loads (checked in the ISA: all s_load are in
    // the kernel prologue).
    auto k_issue = [&](v4u_t (&kf)[2][2], int hh) {
        if constexpr (sizeof(T) == 2) {
            const unsigned ka = kfrag_lane + (unsigned)((hh >> 1) % 3) * STAGE_BYTES + (unsigned)(hh & 1) * 4096u;
            DSRX(kf[0][0], ka, 0 * 512 + 0 * 64); DSRX(kf[0][1], ka, 0 * 512 + 1 * 64);
            DSRX(kf[1][0], ka, 1 * 512 + 1 * 64); DSRX(kf[1][1], ka, 1 * 512 + 0 * 64);
        }
    };

    // S^T of one half-tile: 2 key tiles x QF query tiles
    auto qk_half = [&](f32x4_t (&sd)[2][QF], int hh, v4u_t (&kf)[2][2]) {
        const unsigned char* Kl = lds + ((hh >> 1) % 3) * STAGE_BYTES;
        const int pc = hh & 1;
        if constexpr (sizeof(T) == 2) {
            (void)Kl; (void)pc;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int qf = 0; qf < QF; ++qf) sd[kk][qf] = negm[qf];
            LGKM_N(3, kf[0][0]);
#pragma unroll
            for (int qf = 0; qf < QF; ++qf) Mma<T>::run(sd[0][qf], __builtin_bit_cast(uint4, kf[0][0]), qreg[qf][0]);
            LGKM_N(2, kf[0][1]);
#pragma unroll
            for (int qf = 0; qf < QF; ++qf) Mma<T>::run(sd[0][qf], __builtin_bit_cast(uint4, kf[0][1]), qreg[qf][1]);
            LGKM_N(1, kf[1][0]);
#pragma unroll
            for (int qf = 0; qf < QF; ++qf) Mma<T>::run(sd[1][qf], __builtin_bit_cast(uint4, kf[1][0]), qreg[qf][0]);
            LGKM_N(0, kf[1][1]);
#pragma unroll
            for (int qf = 0; qf < QF; ++qf) Mma<T>::run(sd[1][qf], __builtin_bit_cast(uint4, kf[1][1]), qreg[qf][1]);
            return;
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
            for (int qf = 0; qf < QF; ++qf) sd[kk][qf] = negm[qf];
            const int krow = key_of_row<T>(2 * pc + kk, l15);
#pragma unroll
            for (int c = 0; c < C::NCH; ++c) {
                const uint4 kfrag = lds_chunk<T>(Kl, krow, c * 4 + g);
#pragma unroll
                for (int qf = 0; qf < QF; ++qf) Mma<T>::run(sd[kk][qf], kfrag, qreg[qf][c]);
            }
        }
    };

    // (1) row max of half-tile hh and the rare rescale branch
    auto rowmax_rescale = [&](f32x4_t (&sc)[2][QF], int hh) {
        const int t = hh >> 1, pc = hh & 1, kv0 = t * KT;
        if (kv0 + KT > Nkv) {                                // ragged last tile: mask keys beyond Nkv
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kv0 + key_of_row<T>(2 * pc + kk, 4 * g + r);
                    if (key >= Nkv) {
#pragma unroll
                        for (int qf = 0; qf < QF; ++qf) sc[kk][qf][r] = -INFINITY;
                    }
                }
        }
        float tmax[QF];                                      // max of (s - mb), mb = what the accumulators started from
        const bool first = (hh == 0);
        bool grow = first;
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
                const float mb = first ? 0.f : mrun[qf];
                const float mnew = vmax3(mrun[qf], group4_max(tmax[qf]) + mb, -1e30f);   // column max over the 4 lane groups
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

    // (2) ONE basic block: the exponentials / row sums / bf16 packing of half-tile hh (VALU + transcendental) and,
    // when there is a next half-tile, the 16 MFMAs of its S^T -- independent work, interleaved by the scheduler
    // directives below so the matrix pipe runs under the softmax instead of after it.
    auto exp_and_next_qk = [&](auto has_next_c, f32x4_t (&sc)[2][QF], uint4 (&pfrag)[2][QF], f32x4_t (&sn)[2][QF], int hn, v4u_t (&kf)[2][2]) {
        constexpr bool has_next = decltype(has_next_c)::value;      // compile-time: the steady-state region has no branch
        if constexpr (has_next) qk_half(sn, hn, kf);
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
            if constexpr (sizeof(T) == 2) {
                pfrag[0][qf] = pack_p<bf16_t>(sc[0][qf], sc[1][qf]);
            } else {
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
                    pfrag[kk][qf] = make_uint4(__float_as_uint(sc[kk][qf][0]), __float_as_uint(sc[kk][qf][1]),
                                               __float_as_uint(sc[kk][qf][2]), __float_as_uint(sc[kk][qf][3]));
            }
        }
        if constexpr (sizeof(T) == 2 && EXP2 && has_next) {
            {
                // 4 K-fragment reads, then 16 x {1 MFMA, 2 transcendental}; the pack / row-sum VALU depend on exps of later groups
                // and are left to the scheduler (a VALU group inside the pattern makes it infeasible and it is dropped whole)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x400, 2, 0);
                }
            }
        }
    };

    // (3) O^T += V^T . P^T for half-tile hh
    auto pv_half = [&](uint4 (&pfrag)[2][QF], int hh) {
        const int t = hh >> 1, pc = hh & 1;
        const unsigned char* Vl = lds + (t % 3) * STAGE_BYTES + TILE_BYTES;
        if constexpr (sizeof(T) == 2) {
            (void)Vl;
            const unsigned va = (pc ? vfrag_lane1 : vfrag_lane0) + (unsigned)(t % 3) * STAGE_BYTES;
            v4u_t vf[4];
            DSRX(vf[0], va, 0 * 2048); DSRX(vf[1], va, 1 * 2048); DSRX(vf[2], va, 2 * 2048); DSRX(vf[3], va, 3 * 2048);
            LGKM_N(3, vf[0]);
#pragma unroll
            for (int qf = 0; qf < QF; ++qf) Mma<T>::run(o[0][qf], __builtin_bit_cast(uint4, vf[0]), pfrag[0][qf]);
            LGKM_N(2, vf[1]);
#pragma unroll
            for (int qf = 0; qf < QF; ++qf) Mma<T>::run(o[1][qf], __builtin_bit_cast(uint4, vf[1]), pfrag[0][qf]);
            LGKM_N(1, vf[2]);
#pragma unroll
            for (int qf = 0; qf < QF; ++qf) Mma<T>::run(o[2][qf], __builtin_bit_cast(uint4, vf[2]), pfrag[0][qf]);
            LGKM_N(0, vf[3]);
#pragma unroll
            for (int qf = 0; qf < QF; ++qf) Mma<T>::run(o[3][qf], __builtin_bit_cast(uint4, vf[3]), pfrag[0][qf]);
        } else {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int df = 0; df < 4; ++df) {
                    const uint4 vfrag = lds_chunk<T>(Vl, df * 16 + l15, (2 * pc + kk) * 4 + g);
#pragma unroll
                    for (int qf = 0; qf < QF; ++qf) Mma<T>::run(o[df][qf], vfrag, pfrag[kk][qf]);
                }
        }
    };

    // entering tile tn (called while the previous tile's second half is still to be consumed): its DMA has landed
    // and is published by the barrier; the barrier also proves every wave is done with tile tn-2, whose stage the
    // DMA of tile tn+1 now reuses (3-stage ring)
    auto enter_tile = [&](int tn) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tn + 1 < ntiles) {
            if constexpr (sizeof(T) == 2) stage_tiles_bf16(lds + ((tn + 1) % 3) * STAGE_BYTES, Kr, Vr, kvoff, vvoff, (unsigned)v_row_bytes, tn + 1, wave_u);
            else stage_tiles<T>(lds + ((tn + 1) % 3) * STAGE_BYTES, Kbh, Vbh, v_row_bytes, tn + 1, wave_u, lane);
        }
        if (tn * KT + KT > Nkv) {
            zero_ragged_v<T>(lds + (tn % 3) * STAGE_BYTES + TILE_BYTES, tn * KT, Nkv, tid);
            __syncthreads();
        }
    };

    if constexpr (sizeof(T) == 2) stage_tiles_bf16(lds, Kr, Vr, kvoff, vvoff, (unsigned)v_row_bytes, 0, wave_u);
    else stage_tiles<T>(lds, Kbh, Vbh, v_row_bytes, 0, wave_u, lane);
    (void)LOADS_PER_TILE;
    enter_tile(0);

    // Software pipeline over half-tiles: the MFMAs of S^T(h+1) are independent of the softmax VALU work on S^T(h),
    // so the two interleave inside one wave; two named S buffers alternate (static register indexing).
    f32x4_t sA[2][QF], sB[2][QF];
    uint4 pfrag[2][QF];
    constexpr std::true_type kNext{};
    constexpr std::false_type kLast{};
    v4u_t kf[2][2];
    k_issue(kf, 0);
    qk_half(sA, 0, kf);
    int hs = 0;
    for (; hs + 2 < nhalves; hs += 2) {                                  // steady state: both following halves exist
        k_issue(kf, hs + 1);                                            // same tile: the row max runs under the reads
        rowmax_rescale(sA, hs);
        exp_and_next_qk(kNext, sA, pfrag, sB, hs + 1, kf);              // S^T(hs+1): same tile, second half
        pv_half(pfrag, hs);
        enter_tile((hs + 2) >> 1);                                      // S^T(hs+2) opens the next tile
        k_issue(kf, hs + 2);
        rowmax_rescale(sB, hs + 1);
        exp_and_next_qk(kNext, sB, pfrag, sA, hs + 2, kf);
        pv_half(pfrag, hs + 1);
    }
    if (hs + 1 < nhalves) {                                             // tail: one or two halves left
        k_issue(kf, hs + 1);
        rowmax_rescale(sA, hs);
        exp_and_next_qk(kNext, sA, pfrag, sB, hs + 1, kf);
        pv_half(pfrag, hs);
        rowmax_rescale(sB, hs + 1);
        exp_and_next_qk(kLast, sB, pfrag, sA, 0, kf);
        pv_half(pfrag, hs + 1);
    } else {
        rowmax_rescale(sA, hs);
        exp_and_next_qk(kLast, sA, pfrag, sB, 0, kf);
        pv_half(pfrag, hs);
    }

    // ---- finalize: O = O^T / l, head-major inside the output row
    float inv[QF];
#pragma unroll
    for (int qf = 0; qf < QF; ++qf) {      // cross-lane steps first, outside any divergent region
        inv[qf] = 1.0f / group4_sum(lrun[qf]);
    }
    if constexpr (sizeof(T) == 2) {
        // bf16: the wave's 64 output rows go through the (now idle) K / V^T ring, so that every global store instruction
        // writes 8 whole 128-byte rows (non-temporal) instead of 16 x 4 pieces of 8 bytes at a row stride
        constexpr int RS = 144;                                // staged row: 64 bf16 + pad, 16-B aligned, conflict-free
        __syncthreads();                                       // every wave is done reading the ring
        unsigned char* obuf = lds + wave * (64 * RS);
#pragma unroll
        for (int qf = 0; qf < QF; ++qf)
#pragma unroll
            for (int df = 0; df < 4; ++df)
                *reinterpret_cast<uint2*>(obuf + (qf * 16 + l15) * RS + (df * 16 + g * 4) * 2) =
                    make_uint2(pack_bf16x2(o[df][qf][0] * inv[qf], o[df][qf][1] * inv[qf]), pack_bf16x2(o[df][qf][2] * inv[qf], o[df][qf][3] * inv[qf]));
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int it = 0; it < QF * 2; ++it) {                  // 8 rows x 128 B per store instruction
            const int r = it * 8 + (lane >> 3), c16 = lane & 7, q = q0 + r;
            if (q < Nq) {
                typedef unsigned nt_v4u __attribute__((ext_vector_type(4)));
                const uint4 v = *reinterpret_cast<const uint4*>(obuf + r * RS + c16 * 16);
                __builtin_nontemporal_store(nt_v4u{v.x, v.y, v.z, v.w},
                                            reinterpret_cast<nt_v4u*>(out + ((size_t)b * Nq + q) * ldo + h * DH + c16 * 8));
            }
        }
    } else {
#pragma unroll
        for (int qf = 0; qf < QF; ++qf) {
            const int q = q0 + qf * 16 + l15;
            if (q < Nq) {
                T* orow = out + ((size_t)b * Nq + q) * ldo + h * DH;
#pragma unroll
                for (int df = 0; df < 4; ++df)
                    store4(orow + df * 16 + g * 4, o[df][qf][0] * inv[qf], o[df][qf][1] * inv[qf],
                           o[df][qf][2] * inv[qf], o[df][qf][3] * inv[qf]);
            }
        }
    }
}

#undef DSRX
#undef LGKM_N
