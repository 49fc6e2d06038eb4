// Canvases beyond the token grid: overlapping model-sized windows over a larger canvas, fused where they
// overlap.  Two gathers, both without atomics -- every output element knows its sources, one writer each, two launches the same bits.
//
// pmhip_window_logits: the canvas logits from the window logits.  For canvas row (b, t) and the entries k = 0 .. K - 1 of its cover
//     e_k = cover[t][k]      the row w * g^2 + local inside canvas b's block of Rw = W * g^2 window rows, or -1
//     x_k = win[b * Rw + e_k]                                   or   fma(scale, rn(c_k - u_k), u_k): pmhip_guidance_combine's
//     out = rn(w_0 x_0), then fma(w_k, x_k, out), k ascending over the entries with 0 <= e_k < Rw
// An entry outside [0, Rw) is tested IN FRONT of its load and skipped: it is never an address, and the weight beside it never
// enters a result.  A canvas row without a valid entry is written as 0.  K = 1 with weight 1 is an exact copy (1 * x = x).
//
// HBM-bound streaming: a 64 x 64-token canvas at stride 16 reads 9 x 1024 rows of 8192 f32 (288 MiB, twice that guided) and writes
// 4096 rows (128 MiB).  16 bytes a lane; a row's columns are contiguous across the LANES lanes that serve it (the workgroup's 256
// for V > 1024, one wave for a narrower row: four rows per workgroup); the grid is capped at 2048 workgroups with a grid-stride over
// rows; no LDS.  A wave serves one row, so the row index is wave-uniform: the cover entries and weights of a chunk of four sources are
// scalar loads, waited for on the scalar counter before the chunk's first row load; the entries are tested and the valid ones moved to
// the front by scalar selects, and the chunk runs as straight-line code for its count.  The sources of a row are independent: the
// row loads of a chunk (up to four, eight with the second operand) are issued with no branch and no wait between them, then the
// chunk is accumulated in order.  The window logits are read once: non-temporal loads.  The canvas logits are read next by the sampler:
// plain stores.  Row offsets are 64-bit: B * W * g^2 * V passes 2^32 at ordinary sizes.
//
// pmhip_window_pixels: the canvas image from the decoded window images, img [B * W, C, S, S] -> out [B, C, Hc, Wc].  Per canvas row y
// up to four (window on the y axis, weight) pairs, per column x likewise; with jy ascending outside and jx ascending inside
//     w = rn(ay ax)      out = rn(w p) for the first pair, then fma(w, p, out)      p = img[b * W + jy * nx + jx][c][y - oy][x - ox]
// and finally the clamp of unpatchify_clamp (a NaN stays a NaN).  An entry outside its axis' windows, or whose local coordinate
// falls outside [0, S), is tested in front of the load and skipped.  A pixel one window covers is that window's pixel, bit for bit.
// One pixel a thread, x fastest: a few megabytes once per image, far from the loop.
#include <cmath>

#include "common.h"

// the order above is the contract: no contraction but the fused multiply-adds written as calls
#pragma clang fp contract(off)

namespace {

constexpr int CHUNK = 4;                                       // sources of a row whose loads are in flight together

__device__ __forceinline__ f32x4_t load_once(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p)); }
__device__ __forceinline__ float combine(float c, float u, float scale) { return fmaf(scale, c - u, u); }       // guidance_body's

// N sources of one chunk, in order: their row loads issued together, then accumulated -- rn(w x) for a row's first term, fma behind
template <int N, bool GUIDED>
__device__ __forceinline__ void chunk(const float* base, const float* base_u, int64_t ldw, int col, const int (&ce)[4], const float (&cw)[4],
                                      float scale, f32x4_t& acc, bool& first) {
    f32x4_t x[N], u[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        x[j] = load_once(base + (int64_t)ce[j] * ldw + col);
        if (GUIDED) u[j] = load_once(base_u + (int64_t)ce[j] * ldw + col);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        f32x4_t v = x[j];
        if (GUIDED) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = combine(x[j][i], u[j][i], scale);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = first ? cw[j] * v[i] : fmaf(cw[j], v[i], acc[i]);
        first = false;
    }
}

template <int LANES, bool GUIDED>
__global__ __launch_bounds__(256) void window_logits_kernel(const float* __restrict__ win, const float* __restrict__ win_u, float scale,
                                                            int64_t ldw, const int32_t* __restrict__ cover,
                                                            const float* __restrict__ weight, int K, int Rw, float* __restrict__ out,
                                                            int64_t ldo, int64_t rows, int Nc, int V) {
    constexpr int ROWS = 256 / LANES;                          // canvas rows a workgroup serves at a time
    const int lane = threadIdx.x % LANES, sub = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES);
    for (int64_t row = (int64_t)blockIdx.x * ROWS + sub; row < rows; row += (int64_t)gridDim.x * ROWS) {
        const int64_t b = row / Nc;
        const int t = (int)(row - b * Nc);
        const float* base = win + b * Rw * ldw;
        const float* base_u = GUIDED ? win_u + b * Rw * ldw : nullptr;
        float* o = out + row * ldo;
        // One row per wave: t is wave-uniform, so the chunk's cover entries and weights are scalar loads (their wait is not the
        // vector loads' counter) and the tests are scalar branches.
        const int32_t* cov = cover + (int64_t)t * K;
        const float* wgt = weight + (int64_t)t * K;
        for (int col = lane * 4; col < V; col += LANES * 4) {
            f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
            bool first = true;
            for (int k0 = 0; k0 < K; k0 += CHUNK) {
                int e[CHUNK];
                float w[CHUNK];
#pragma unroll
                for (int j = 0; j < CHUNK; ++j) {                  // the chunk's table entries first: nothing below waits on them again
                    const bool in = k0 + j < K;
                    const int ek = in ? cov[k0 + j] : -1;
                    w[j] = in ? wgt[k0 + j] : 0.f;
                    e[j] = ek >= 0 && ek < Rw ? ek : -1;           // outside [0, Rw): never an address
                }
                // The valid entries move to the front in order (scalar selects), and the chunk runs as straight-line code for its
                // count: no branch, and so no wait, stands between its row loads.
                int ce[CHUNK] = {0, 0, 0, 0}, n = 0;
                float cw[CHUNK] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < CHUNK; ++j) {
                    const bool on = e[j] >= 0;
#pragma unroll
                    for (int s = 0; s <= j; ++s) {
                        ce[s] = on && s == n ? e[j] : ce[s];
                        cw[s] = on && s == n ? w[j] : cw[s];
                    }
                    n += on;
                }
                switch (n) {
                    case 1: chunk<1, GUIDED>(base, base_u, ldw, col, ce, cw, scale, acc, first); break;
                    case 2: chunk<2, GUIDED>(base, base_u, ldw, col, ce, cw, scale, acc, first); break;
                    case 3: chunk<3, GUIDED>(base, base_u, ldw, col, ce, cw, scale, acc, first); break;
                    case 4: chunk<4, GUIDED>(base, base_u, ldw, col, ce, cw, scale, acc, first); break;
                    default: break;
                }
            }
            *reinterpret_cast<f32x4_t*>(o + col) = acc;
        }
    }
}

__device__ __forceinline__ float clamp_keep_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }     // rowops.hip's

__global__ __launch_bounds__(256) void window_pixels_kernel(const float* __restrict__ img, const int32_t* __restrict__ ywin,
                                                            const float* __restrict__ yw, const int32_t* __restrict__ xwin,
                                                            const float* __restrict__ xw, const int32_t* __restrict__ yoff,
                                                            const int32_t* __restrict__ xoff, float* __restrict__ out, int B, int C, int S,
                                                            int ny, int nx, int Hc, int Wc) {
    const int64_t total = (int64_t)B * C * Hc * Wc;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wc), y = (int)(i / Wc % Hc), c = (int)(i / ((int64_t)Wc * Hc) % C);
        const int64_t b = i / ((int64_t)Wc * Hc * C);
        float acc = 0.f;
        bool first = true;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int jy = ywin[y * 4 + a];
            if (jy < 0 || jy >= ny) continue;
            const int ly = y - yoff[jy];
            if (ly < 0 || ly >= S) continue;
            const float ay = yw[y * 4 + a];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int jx = xwin[x * 4 + d];
                if (jx < 0 || jx >= nx) continue;
                const int lx = x - xoff[jx];
                if (lx < 0 || lx >= S) continue;
                const float w = ay * xw[x * 4 + d];
                const float p = img[(((b * ny + jy) * nx + jx) * C + c) * S * S + (int64_t)ly * S + lx];
                acc = first ? w * p : fmaf(w, p, acc);
                first = false;
            }
        }
        out[i] = clamp_keep_nan(acc, -1.f, 1.f);
    }
}

template <int LANES>
void launch_logits(const float* win, const float* win_u, float scale, int64_t ldw, const int32_t* cover, const float* weight, int K, int Rw,
                   float* out, int64_t ldo, int64_t rows, int Nc, int V, hipStream_t s) {
    constexpr int ROWS = 256 / LANES;
    const int64_t groups = (rows + ROWS - 1) / ROWS;
    const dim3 grid((unsigned)(groups < 2048 ? groups : 2048)), block(256);
    if (win_u != nullptr)
        hipLaunchKernelGGL((window_logits_kernel<LANES, true>), grid, block, 0, s, win, win_u, scale, ldw, cover, weight, K, Rw, out, ldo, rows,
                           Nc, V);
    else
        hipLaunchKernelGGL((window_logits_kernel<LANES, false>), grid, block, 0, s, win, win_u, scale, ldw, cover, weight, K, Rw, out, ldo, rows,
                           Nc, V);
}

}  // namespace

extern "C" int pmhip_window_logits(const float* win, const float* win_u, float scale, int ldw, const int32_t* cover, const float* weight,
                                   int K, int window_rows, float* out, int ldo, int B, int Nc, int V, pmhip_stream stream) {
    PM_REQUIRE(win && cover && weight && out, "window_logits: win, cover, weight or out is NULL");
    PM_REQUIRE(B > 0 && Nc > 0 && window_rows > 0, "window_logits: B=%d, Nc=%d and window_rows=%d must be positive", B, Nc, window_rows);
    PM_REQUIRE(K >= 1 && K <= 16, "window_logits: K=%d must be in 1..16", K);
    PM_REQUIRE(V > 0 && V % 4 == 0, "window_logits: V=%d must be a positive multiple of 4", V);
    PM_REQUIRE(ldw % 4 == 0 && ldw >= V, "window_logits: ldw=%d must be a multiple of 4 and at least V=%d", ldw, V);
    PM_REQUIRE(ldo % 4 == 0 && ldo >= V, "window_logits: ldo=%d must be a multiple of 4 and at least V=%d", ldo, V);
    PM_REQUIRE(pm_aligned(16, {win, win_u, out}), "window_logits: win, win_u and out must be 16-byte aligned (float4 accesses)");
    PM_REQUIRE(win_u == nullptr || std::isfinite(scale), "window_logits: scale=%f must be finite (win_u is given)", (double)scale);
    hipStream_t s = (hipStream_t)stream;
    PmTimer tm(FAM_SAMPLE, s);
    const int64_t rows = (int64_t)B * Nc;
    if (V <= 1024) launch_logits<64>(win, win_u, scale, ldw, cover, weight, K, window_rows, out, ldo, rows, Nc, V, s);
    else launch_logits<256>(win, win_u, scale, ldw, cover, weight, K, window_rows, out, ldo, rows, Nc, V, s);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

extern "C" int pmhip_window_pixels(const float* img, const int32_t* ywin, const float* yw, const int32_t* xwin, const float* xw,
                                   const int32_t* yoff, const int32_t* xoff, float* out, int B, int C, int S, int ny, int nx, int Hc, int Wc,
                                   pmhip_stream stream) {
    PM_REQUIRE(img && ywin && yw && xwin && xw && yoff && xoff && out, "window_pixels: a pointer is NULL");
    PM_REQUIRE(B > 0 && C > 0 && S > 0 && ny > 0 && nx > 0, "window_pixels: B=%d, C=%d, S=%d, ny=%d and nx=%d must be positive", B, C, S, ny, nx);
    PM_REQUIRE(Hc >= S && Wc >= S, "window_pixels: the canvas %d x %d is smaller than a window (S=%d)", Hc, Wc, S);
    hipStream_t s = (hipStream_t)stream;
    PmTimer tm(FAM_ROWOPS, s);
    const int64_t total = (int64_t)B * C * Hc * Wc, groups = (total + 255) / 256;
    hipLaunchKernelGGL(window_pixels_kernel, dim3((unsigned)(groups < 2048 ? groups : 2048)), dim3(256), 0, s, img, ywin, yw, xwin, xw, yoff,
                       xoff, out, B, C, S, ny, nx, Hc, Wc);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}
