// Bias gradients of the BitFit runs (`--unfreeze_bias`, trainer_base.py:469-475: every parameter whose name contains "bias" trains),
// produced where the data already is:
//
//   colsum_seg    column sums of a STRIDED matrix x [M, n] (row stride ld >= n) whose n = S * w columns are S segments of w, each segment
//                 going to its own fp32 destination (or nowhere): the q | k | v bias gradients of a fused projection, the k_proj biases
//                 of all decoder layers over the shared cross-key gradient, a column block of a wider buffer.  Pass 1 = per-workgroup
//                 partials [tail_blocks(M)][n] (colsum_partial_kernel's walk: a wave owns a row, lanes own 16-byte pieces, the next row
//                 is requested before the current one is added) with the columns split over blockIdx.y in chunks of at most 4 pieces
//                 per lane, so that n = 6,144 costs no more registers than n = 2,048; pass 2 = tail_reduce_kernel's sum with the
//                 segment's pointer picked per column.
//   act_bwd_cols  dx = dy * mask / (1 - p) * act'(x) (actdrop.hip's backward, the same expression and the same mask) by lanes that own
//                 a group of 8 columns and walk rows, so that each lane can also keep the column sums of what it stores: the fc1 bias
//                 gradient without a second read of the [M, ffn] gradient.  Partials [gy][n_cols], reduced by tail_reduce_kernel.
//
// No atomics; every sum's order is a function of the shape alone.
#include "common.h"
#include "kernels.h"
#include "rowops.h"
#include "rng.h"
#include "vec8.h"
#include "act_math.h"

constexpr int BG_WAVES = 4;                 // waves per workgroup of both first passes (= tail.hip's TAIL_WAVES: tail_blocks counts rows in fours)
constexpr int SEG_NP_MAX = 4;               // 16-byte pieces per lane and column chunk

// a + b as ONE rounded addition: with contraction allowed the compiler may fold the product that formed b into the sum, which would
// then be the sum of the UNROUNDED values (fp32 IO; at bf16 the conversion separates the two)
__device__ __forceinline__ float add_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// ------------------------------------------------------------------------------------------------------------------ colsum_seg
// Loads are unconditional: a lane past the last piece reads the last piece again and a wave past the last row the last row (clamped
// indices, tail.hip round 5: loads under a branch make the compiler wait for every outstanding request before the use of any).
template <typename IO, int NP>
__global__ __launch_bounds__(BG_WAVES * 64) void colsum_seg_partial_kernel(const void* __restrict__ xin, int64_t M, int n, int64_t ld,
                                                                           float* __restrict__ part) {
    using P = Piece<IO>;
    constexpr int E = P::E;
    __shared__ float acc[BG_WAVES][64 * 8];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pieces = n / E;
    const int base = (int)blockIdx.y * NP * 64;                    // first piece of this column chunk
    const uint8_t* x = reinterpret_cast<const uint8_t*>(xin);
    const int64_t rstride = (int64_t)gridDim.x * BG_WAVES;
    int pc[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) { const int p = base + lane + 64 * k; pc[k] = p < pieces ? p : pieces - 1; }
    float s[NP][E];
#pragma unroll
    for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int j = 0; j < E; ++j) s[k][j] = 0.f;
    u32x4 cur[NP];
    auto load_row = [&](int64_t r, u32x4 (&rd)[NP]) {
        if (r >= M) r = M - 1;
        const int64_t o = r * ld * (int64_t)sizeof(IO);
#pragma unroll
        for (int k = 0; k < NP; ++k) rd[k] = P::load_raw_nt(x + o + (int64_t)pc[k] * 16);
    };
    const int64_t r0 = (int64_t)blockIdx.x * BG_WAVES + wave;
    load_row(r0, cur);
    for (int64_t row = r0; row < M; row += rstride) {
        u32x4 nxt[NP];
        load_row(row + rstride, nxt);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            float v[E];
            P::from_raw(cur[k], v);
#pragma unroll
            for (int j = 0; j < E; ++j) s[k][j] += v[j];
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) cur[k] = nxt[k];
    }
    float* dst = part + (size_t)blockIdx.x * n;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int p = base + lane + 64 * k;
#pragma unroll
        for (int j = 0; j < E; ++j) acc[wave][lane * 8 + j] = s[k][j];
        __syncthreads();
        if (wave == 0 && p < pieces) {
#pragma unroll
            for (int j = 0; j < E; ++j) {
                float t = 0.f;
#pragma unroll
                for (int w = 0; w < BG_WAVES; ++w) t += acc[w][lane * 8 + j];
                dst[p * E + j] = t;
            }
        }
        __syncthreads();
    }
}

// partials [nb][n] -> segment s of w columns into out.p[s] (nullptr: not wanted).  tail_reduce_kernel's order: a workgroup owns 64
// columns, its 16 waves take every 16th partial row, LDS combines them.
__global__ __launch_bounds__(1024) void colsum_seg_reduce_kernel(const float* __restrict__ part, int nb, int n, int w, SegOut out) {
    __shared__ float acc[16][64];
    __shared__ float* dstp[VLPET_COLSUM_SEGS];
    const int c = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + c;
#pragma unroll
    for (int k = 0; k < VLPET_COLSUM_SEGS; ++k)
        if ((int)threadIdx.x == k) dstp[k] = out.p[k];              // (constant indices into the kernel arguments)
    float v = 0.f;
    if (col < n) {
        const float* src = part + col;
        int r = s;
        for (; r + 48 < nb; r += 64) {
            const float a0 = src[(size_t)r * n], a1 = src[(size_t)(r + 16) * n], a2 = src[(size_t)(r + 32) * n],
                        a3 = src[(size_t)(r + 48) * n];
            v += (a0 + a1) + (a2 + a3);
        }
        for (; r < nb; r += 16) v += src[(size_t)r * n];
    }
    acc[s][c] = v;
    __syncthreads();
    if (s == 0 && col < n) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += acc[k][c];
        const int sg = col / w;
        float* dst = dstp[sg];
        if (dst != nullptr) dst[col - sg * w] = t;
    }
}

// column chunks of n: the fewest chunks of at most SEG_NP_MAX pieces per lane, evenly sized
static void seg_chunks(int pieces, int* np, int* chunks) {
    const int rounds = (pieces + 63) / 64;
    *chunks = (rounds + SEG_NP_MAX - 1) / SEG_NP_MAX;
    *np = (rounds + *chunks - 1) / *chunks;
}

template <typename IO>
static hipError_t launch_seg_partial(const void* x, int64_t M, int n, int64_t ld, float* part, int blocks, hipStream_t stream) {
    int np, chunks;
    seg_chunks(n / Piece<IO>::E, &np, &chunks);
    const dim3 g(blocks, chunks), b(BG_WAVES * 64);
    if (np <= 1) hipLaunchKernelGGL((colsum_seg_partial_kernel<IO, 1>), g, b, 0, stream, x, M, n, ld, part);
    else if (np <= 2) hipLaunchKernelGGL((colsum_seg_partial_kernel<IO, 2>), g, b, 0, stream, x, M, n, ld, part);
    else if (np <= 3) hipLaunchKernelGGL((colsum_seg_partial_kernel<IO, 3>), g, b, 0, stream, x, M, n, ld, part);
    else hipLaunchKernelGGL((colsum_seg_partial_kernel<IO, 4>), g, b, 0, stream, x, M, n, ld, part);
    return hipGetLastError();
}

size_t colsum_seg_ws_floats(int64_t M, int n) { return (size_t)tail_blocks(M) * (size_t)n; }

hipError_t launch_colsum_seg(const void* x, int64_t M, int n, int64_t ld, int w, const SegOut& out, float* part, int io_fp32,
                             hipStream_t stream) {
    const int blocks = tail_blocks(M);
    hipError_t e = io_fp32 ? launch_seg_partial<float>(x, M, n, ld, part, blocks, stream)
                           : launch_seg_partial<__bf16>(x, M, n, ld, part, blocks, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(colsum_seg_reduce_kernel, dim3((n + 63) / 64), dim3(1024), 0, stream, part, blocks, n, w, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- act_bwd_cols
// Lane (blockIdx.x, lane) owns column group cg = 64 blockIdx.x + lane (8 columns); wave w of workgroup row-slice y walks rows
// 4 y + w, + 4 gridDim.y, ...  A wave reads and writes 64 x 16 bytes (bf16) of one row at a time, the next row's x and dy requested
// before the current row's arithmetic.  The generator group of (row, cg) is row * n_cols / 8 + cg: the flat index / 8 of actdrop.hip.
// A lane past the last column group works on the last group again (clamped index: unconditional loads) and stores nothing.
template <typename IO, int ACT, bool DROP>
__global__ __launch_bounds__(BG_WAVES * 64) void act_bwd_cols_kernel(ActColsArgs a) {
    __shared__ float acc[BG_WAVES][64 * 8];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t gpr = a.n_cols >> 3;
    const int64_t cg = (int64_t)blockIdx.x * 64 + lane;
    const bool mine = cg < gpr;
    const int64_t cgc = mine ? cg : gpr - 1;
    const uint64_t seed = DROP ? vlpet_eff_seed(a.seed, a.seed_ctr) : 0;
    const int64_t rstride = (int64_t)gridDim.y * BG_WAVES;
    const int64_t r0 = (int64_t)blockIdx.y * BG_WAVES + wave;
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.f;
    Vec8<IO> cx, cdy;
    {
        const int64_t r = r0 < a.M ? r0 : a.M - 1;
        cx.load(a.x, r * gpr + cgc);
        cdy.load(a.dy, r * gpr + cgc);
    }
    for (int64_t row = r0; row < a.M; row += rstride) {
        Vec8<IO> nx, ndy;
        {
            const int64_t r = row + rstride < a.M ? row + rstride : a.M - 1;
            nx.load(a.x, r * gpr + cgc);
            ndy.load(a.dy, r * gpr + cgc);
        }
        const int64_t g = row * gpr + cgc;
        uint32_t bits = 0xffu;
        if constexpr (DROP) bits = keep8(g, seed, a.thr);
        Vec8<IO> o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float k = ((bits >> j) & 1u) ? a.keep_scale : 0.f;
            o.set(j, cdy.get(j) * k * act_df<ACT>(cx.get(j)));
        }
        if (mine) o.store(a.dx, g);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = add_rounded(s[j], o.get(j));      // dx AS STORED (rounded to the IO dtype)
        cx = nx; cdy = ndy;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[wave][lane * 8 + j] = s[j];
    __syncthreads();
    if (wave == 0 && mine) {
        float* dst = a.part + (size_t)blockIdx.y * a.n_cols + cg * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < BG_WAVES; ++w) t += acc[w][lane * 8 + j];
            dst[j] = t;
        }
    }
}

// row slices (= partial rows) of the launch: four rows per workgroup pass, at most ACT_COLS_CAP workgroups over the whole grid
constexpr int ACT_COLS_CAP = 2048;
int act_cols_partials(int64_t M, int n_cols) {
    const int gx = (n_cols / 8 + 63) / 64;
    const int64_t need = (M + BG_WAVES - 1) / BG_WAVES;
    const int64_t cap = ACT_COLS_CAP / gx > 0 ? ACT_COLS_CAP / gx : 1;
    return (int)(need < cap ? need : cap);
}

template <typename IO, int ACT>
static hipError_t launch_act_cols(const ActColsArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n_cols / 8 + 63) / 64), (unsigned)act_cols_partials(a.M, a.n_cols)), blk(BG_WAVES * 64);
    if (a.thr != 0) hipLaunchKernelGGL((act_bwd_cols_kernel<IO, ACT, true>), grid, blk, 0, stream, a);
    else hipLaunchKernelGGL((act_bwd_cols_kernel<IO, ACT, false>), grid, blk, 0, stream, a);
    return hipGetLastError();
}

template <typename IO>
static hipError_t launch_act_cols_io(const ActColsArgs& a, hipStream_t stream) {
    switch (a.act) {
        case VLPET_ACT_GELU: return launch_act_cols<IO, VLPET_ACT_GELU>(a, stream);
        case VLPET_ACT_GELU_NEW: return launch_act_cols<IO, VLPET_ACT_GELU_NEW>(a, stream);
        case VLPET_ACT_RELU: return launch_act_cols<IO, VLPET_ACT_RELU>(a, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_act_dropout_bwd_cols(const ActColsArgs& a, int io_fp32, hipStream_t stream) {
    return io_fp32 ? launch_act_cols_io<float>(a, stream) : launch_act_cols_io<__bf16>(a, stream);
}
