// The prologue the selection kernels of sample.hip share (sample_wide_kernel, sample_nucleus_kernel; DESIGN.md sections 4n, 4o),
// included into the kernel body like remask_select.h: one copy of the text, and each kernel compiles as if it were written out.
// In scope: the kernel's parameters (logits, ldl, topk, temperature, seed, step, row_base, M, V, gp, period, slots, tokens,
// top_p_dev) and NV4, PERIOD, SLOTS; for the SLOTS form also CLS, the kernel's class (common.h pm_sample_class), and a float top_p
// that takes the slot's nucleus mass: topk and top_p then are the slot's, wave-uniform like the arguments they replace.
// Leaves behind: lane, row, rs, lrow, the normaliser (mx, se), the row's keys key[NV4][4] and (tau, last) -- an element is among
// the first top-k of (value desc, column asc) iff key > tau, or key == tau and its column <= last; no column >= V is.
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (row >= M) return;                                  // whole wave exits together
    const RowStep rs = row_step<SLOTS>(RowStep{topk, temperature, seed, step, row_base, false}, row, gp, slots, tokens);
    if constexpr (SLOTS) {                                 // a per-image launch: the rows of class CLS only; top-k and top_p are the slot's
        if (!slot_in_class(CLS, rs, row, tokens, top_p_dev, top_p)) return;
        topk = rs.topk;
    }
    const int lr = PERIOD ? row % period : row;
    const float* lrow = logits + (size_t)lr * ldl;

    float4 x[NV4];
#pragma unroll
    for (int g = 0; g < NV4; ++g) {
        const int col = (g * 64 + lane) * 4;
        x[g] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        if (col < V) x[g] = *reinterpret_cast<const float4*>(lrow + col);
    }
    // ---- softmax normaliser of the UNfiltered row: sample_rows_kernel's expressions, in its order
    float mx = -INFINITY;
#pragma unroll
    for (int g = 0; g < NV4; ++g) mx = fmaxf(mx, fmaxf(fmaxf(x[g].x, x[g].y), fmaxf(x[g].z, x[g].w)));
    mx = wave_max(mx);
    float se = 0.f;
#pragma unroll
    for (int g = 0; g < NV4; ++g)
        se += (__expf(x[g].x - mx) + __expf(x[g].y - mx)) + (__expf(x[g].z - mx) + __expf(x[g].w - mx));
    se = wave_sum(se);

    // ---- 1. keys in place of the values
    uint32_t key[NV4][4];
#pragma unroll
    for (int g = 0; g < NV4; ++g) {
        const bool in = (g * 64 + lane) * 4 < V;
        key[g][0] = in ? orderable(x[g].x + 0.f) : 0u;
        key[g][1] = in ? orderable(x[g].y + 0.f) : 0u;
        key[g][2] = in ? orderable(x[g].z + 0.f) : 0u;
        key[g][3] = in ? orderable(x[g].w + 0.f) : 0u;
    }
    // kept: key > tau, or key == tau and column <= last.  As they stand: every column < V (its key is above 0), none beyond.
    // An element's column is (g * 64 + lane) * 4 + e = lane * 4 + (g * 256 + e): a bound on it is compared with the constant
    // part after one subtraction per lane, so no column sits in a register.
    uint32_t tau = 0u;
    int last = V - 1;
    if (topk < V) {                                        // wave-uniform
        // ---- 2. the k-th largest key: the largest t with #(key >= t) >= k
#pragma unroll 1
        for (uint32_t bit = 0x80000000u; bit; bit >>= 1) {
            const uint32_t trial = tau | bit;
            int n = 0;
#pragma unroll
            for (int g = 0; g < NV4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) n += key[g][e] >= trial;
            if (__builtin_amdgcn_readfirstlane(wave_count(n)) >= topk) tau = trial;
        }
        int above = 0, equal = 0;
#pragma unroll
        for (int g = 0; g < NV4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                above += key[g][e] > tau;
                equal += key[g][e] == tau;
            }
        const int need = topk - __builtin_amdgcn_readfirstlane(wave_count(above));     // >= 1: tau is the k-th largest
        // ---- 3. the plateau straddles position k: the need-th lowest column of it = the largest c with #(equal, column < c) < need
        if (need < __builtin_amdgcn_readfirstlane(wave_count(equal))) {
            int c = 0;
#pragma unroll 1
            for (int bit = NV4 * 128; bit; bit >>= 1) {
                const int trial = c | bit, mine = trial - lane * 4;
                int n = 0;
#pragma unroll
                for (int g = 0; g < NV4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) n += key[g][e] == tau && g * 256 + e < mine;
                if (__builtin_amdgcn_readfirstlane(wave_count(n)) < need) c = trial;
            }
            last = min(c, V - 1);
        }
    }
