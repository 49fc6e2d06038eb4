// The keys of the CHOICE forms of the re-masking kernels (sample.hip), included into the body of each of them in
// front of remask_select.h: ONE copy of the perturbed confidence, compiled into every kernel exactly as if it were written there.
// In scope where it is included: E, xs[NP] (LDS), base = threadIdx.x * E, sc (the image's scores), N, noise, ic (ImageChoice: t, seed,
// step, base).  Leaves key[E] and mine[E] for remask_select.h.
    // one element at a time (a Philox and three logf each: unrolled E = 16 times they would not fit the registers), through the
    // thread's own E words of xs, which nobody else touches before the first barrier
#pragma unroll 1
    for (int e = 0; e < E; ++e) {
        const int i = base + e;
        unsigned long long k = 0ull;
        if (i < N) {
            float s = sc[i];
            if (ic.t != 0.f && !(s < 0.f)) {
                float u;
                if (noise) {
                    u = noise[(size_t)blockIdx.x * N + i];
                } else {
                    const uint64_t grow = ic.base + (uint64_t)i;
                    const uint4 rnd = philox4x32_10(make_uint4((uint32_t)grow, (uint32_t)(grow >> 32), 0xFFFFFFFFu, ic.step),
                                                    make_uint2((uint32_t)ic.seed, (uint32_t)(ic.seed >> 32)));
                    u = (float)(rnd.x >> 8) * (1.0f / 16777216.0f);
                }
                const float ph = 1.0f - s;
                const float conf = logf(fmaxf(ph, 0x1p-24f));
                s = -fmaf(ic.t, gumbel_from_uniform(u), conf);
            }
            k = remask_key(s, i);
        }
        xs[i] = k;
    }
    unsigned long long key[E], mine[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        key[e] = xs[base + e];
        mine[e] = key[e];
    }
