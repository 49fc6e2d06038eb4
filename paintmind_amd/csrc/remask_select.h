// The selection of the re-masking kernels (sample.hip), included into the body of each of them: ONE copy of the bitonic network, the
// threshold and the store, compiled into every kernel exactly as if it were written there.  In scope where it is included:
//   E, NP = THREADS * E, xs[NP] (LDS), base = threadIdx.x * E, key[E] (sorted in place), mine[E] (a copy that stays), num_mask, N, ids,
//   mask_id.
// A bitonic compare-exchange with distance j is in-thread for j < E, a wave shuffle for j < 64*E and goes through LDS (two barriers)
// only beyond that: 3 of the 55 stages at N = 1024.
#pragma unroll
    for (int k = 2; k <= NP; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j < E) {                                   // both elements in this thread
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if ((e & j) == 0) {
                        const bool desc = ((base + e) & k) == 0;
                        const unsigned long long a = key[e], b = key[e | j];
                        const bool swap = desc ? (a < b) : (a > b);
                        key[e] = swap ? b : a;
                        key[e | j] = swap ? a : b;
                    }
                }
            } else {
                unsigned long long other[E];
                if (j < 64 * E) {                          // the partner thread is in this wave
#pragma unroll
                    for (int e = 0; e < E; ++e) other[e] = __shfl_xor(key[e], j / E, 64);
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e) xs[base + e] = key[e];
                    __syncthreads();
#pragma unroll
                    for (int e = 0; e < E; ++e) other[e] = xs[(base + e) ^ j];
                    __syncthreads();
                }
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int i = base + e;
                    const bool want_max = ((i & j) == 0) == ((i & k) == 0);   // descending block: the lower index keeps the larger key
                    const unsigned long long a = key[e], b = other[e];
                    key[e] = want_max ? (a > b ? a : b) : (a < b ? a : b);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) xs[base + e] = key[e];
    __syncthreads();
    const int nm = num_mask < 1 ? 1 : (num_mask > N ? N : num_mask);
    const unsigned long long thr = xs[nm - 1];
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (base + e < N && mine[e] >= thr) ids[(size_t)blockIdx.x * N + base + e] = mask_id;
