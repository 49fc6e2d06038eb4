// The draw the selection kernels of sample.hip share, included into the kernel body behind sample_select_prologue.h.  In scope:
// what the prologue left, the mask words kept[NW] (bit s = g * 4 + e of the lane's elements, none of them a column >= V; consumed
// here), noise and the kernel's outputs.
    // ---- 5. the draw: every lane among its own kept elements, lowest column first
    Cand best{-INFINITY, 0x7fffffff};
    float raw = -INFINITY;
    for (;;) {
        int s = -1;
#pragma unroll
        for (int w = NW - 1; w >= 0; --w)
            if (kept[w]) s = w * 32 + __ffs((int)kept[w]) - 1;
        if (s < 0) break;
#pragma unroll
        for (int w = 0; w < NW; ++w)
            if ((s >> 5) == w) kept[w] &= kept[w] - 1u;
        const int col = (((s >> 2) * 64 + lane) << 2) + (s & 3);          // < V: step 4 kept no other
        const float v = lrow[col];
        const float pv = perturbed(v, col, row, V, rs, noise);
        if (before(pv, col, best.v, best.i)) { best.v = pv; best.i = col; raw = v; }
    }
    const Cand win = wave_best(best);
    const int owner = __builtin_amdgcn_readfirstlane((win.i >> 2) & 63);   // the lane that holds the winner's column
    raw = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(raw), owner));
    if (lane == 0) store_outcome(row, true, win.i, expf(raw - mx) / se, ids_in, mask_id, pred_out, ids_out, score_out);
