// The joint encoder's input assembly with a prompt in front (prompt tuning: src/prompt/prompt_modeling.py InputPrompts,
// src/modeling_bart.py:776-833, src/modeling_t5.py:236-327):
//     x[b] = dropout(cat([pre, a[b], v[b]], dim = 0), p)      pre [P, d] (the SAME rows for every batch item), a [B, La, d], v [B, Lv, d]
// The reference expands the prompt to [B, P, d] before its MLP, so every layer above it works on B * P rows and autograd sums B * P
// gradient rows back; here the prompt stays [P, d] up to this pass.  The three-segment form of cat_dropout_kernel (actdrop.hip): same
// generator, same counter (the 8-element group index of the row-major x), so the mask is dropout_spec.keep_mask(B * (P + La + Lv), d).
//
// Forward: one pass, 16-byte accesses; pre is read with the default cache policy (P * d distinct elements serve B * P * d stores: they stay
// in L2 / the vector cache), a and v non-temporal like every stream these kernels read once.
// Backward: ONE launch does both halves --
//   blocks [0, nS):  da / dv = masked, scaled slices of dx (as cat_dropout_kernel's backward);
//   blocks [nS, ..): dpre partials.  B is split into NC chunks of CS batch items (prefix_cat_split: a function of B alone); thread
//                    (chunk c, group pg of the [P, d / 8] prefix) adds keep * scale * dx[b, pg] over its chunk's items in b order, fp32,
//                    and writes its eight sums to ws[c][pg];
// then a small second launch adds the NC partials of every group in chunk order and rounds once to the IO dtype.  No atomics, and the
// order of every sum is a function of (B, P, d) only, so dpre is bitwise repeatable.  (Two launches, not the in-launch arrival pattern of
// cols_reduce.h: the partials are NC * P * d * 4 bytes -- 3.9 MB at B = 500, P = 40, d = 768 -- and the second launch reads them from L2;
// profiles/r16_prompt.md has the times.)
#include "common.h"
#include "kernels.h"
#include "rng.h"
#include "vec8.h"

// Vec8 load with the default (cached) policy
__device__ __forceinline__ void load8_cached(Vec8<__bf16>& o, const void* p, int64_t g) { o.v = reinterpret_cast<const bf16x8*>(p)[g]; }
__device__ __forceinline__ void load8_cached(Vec8<float>& o, const void* p, int64_t g) {
    o.a = reinterpret_cast<const f32x4*>(p)[2 * g];
    o.b = reinterpret_cast<const f32x4*>(p)[2 * g + 1];
}

void prefix_cat_split(int64_t B, int* cs, int* nc) {
    const int64_t c = (B + PREFIX_CAT_MAX_CHUNKS - 1) / PREFIX_CAT_MAX_CHUNKS;       // batch items per chunk
    *cs = (int)c;
    *nc = (int)((B + c - 1) / c);
}

template <typename IO, bool DROP>
__global__ __launch_bounds__(256) void prefix_cat_fwd_kernel(PrefixCatArgs c) {
    const int gpr = c.d >> 3, L = c.P + c.La + c.Lv;
    const int64_t groups = c.B * (int64_t)L * gpr;
    const uint64_t seed = DROP ? vlpet_eff_seed(c.seed, c.seed_ctr) : 0;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = g / gpr;
        const int col = (int)(g - row * gpr);
        const int64_t b = row / L;
        const int t = (int)(row - b * L);
        Vec8<IO> in, o;
        if (t < c.P) load8_cached(in, c.pre, (int64_t)t * gpr + col);
        else if (t < c.P + c.La) in.load(c.a, (b * c.La + (t - c.P)) * (int64_t)gpr + col);
        else in.load(c.v, (b * c.Lv + (t - c.P - c.La)) * (int64_t)gpr + col);
        uint32_t bits = 0xffu;
        if constexpr (DROP) bits = keep8(g, seed, c.thr);
#pragma unroll
        for (int j = 0; j < 8; ++j) o.set(j, ((bits >> j) & 1u) ? in.get(j) * c.keep_scale : 0.f);
        o.store(c.x, g);
    }
}

template <typename IO, bool DROP>
__global__ __launch_bounds__(256) void prefix_cat_bwd_kernel(PrefixCatArgs c, int n_stream) {
    const int gpr = c.d >> 3, L = c.P + c.La + c.Lv, Ls = c.La + c.Lv;
    const uint64_t seed = DROP ? vlpet_eff_seed(c.seed, c.seed_ctr) : 0;
    if ((int)blockIdx.x < n_stream) {                       // ---- da, dv
        const int64_t groups = c.B * (int64_t)Ls * gpr;
        for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < groups; s += (int64_t)n_stream * blockDim.x) {
            const int64_t row = s / gpr;
            const int col = (int)(s - row * gpr);
            const int64_t b = row / Ls;
            const int t = (int)(row - b * Ls);
            const bool text = t < c.La;
            void* side = const_cast<void*>(text ? c.a : c.v);
            if (side == nullptr) continue;
            const int64_t sg = text ? (b * c.La + t) * (int64_t)gpr + col : (b * c.Lv + (t - c.La)) * (int64_t)gpr + col;
            const int64_t g = (b * L + c.P + t) * (int64_t)gpr + col;
            uint32_t bits = 0xffu;
            if constexpr (DROP) bits = keep8(g, seed, c.thr);
            Vec8<IO> in, o;
            in.load(c.x, g);
#pragma unroll
            for (int j = 0; j < 8; ++j) o.set(j, ((bits >> j) & 1u) ? in.get(j) * c.keep_scale : 0.f);
            o.store(side, sg);
        }
        return;
    }
    // ---- dpre partials: thread = (chunk, prefix group)
    const int64_t pgroups = (int64_t)c.P * gpr;
    const int64_t idx = (int64_t)(blockIdx.x - n_stream) * blockDim.x + threadIdx.x;
    if (idx >= pgroups * c.NC) return;
    const int chunk = (int)(idx / pgroups);
    const int64_t pg = idx - chunk * pgroups;
    const int64_t b0 = (int64_t)chunk * c.CS;
    const int64_t b1 = b0 + c.CS < c.B ? b0 + c.CS : c.B;
    const int64_t bstride = (int64_t)L * gpr;               // groups between the same prefix group of consecutive batch items
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t b = b0; b < b1; b += 4) {                  // four items' loads in flight before the first add; b order kept
        Vec8<IO> in[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (b + u < b1) in[u].load(c.x, (b + u) * bstride + pg);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (b + u >= b1) break;
            uint32_t bits = 0xffu;
            if constexpr (DROP) bits = keep8((b + u) * bstride + pg, seed, c.thr);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += ((bits >> j) & 1u) ? in[u].get(j) * c.keep_scale : 0.f;
        }
    }
    f32x4* w = reinterpret_cast<f32x4*>(c.ws) + 2 * idx;
    w[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
    w[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
}

// dpre group pg = sum over chunks 0, 1, .. of ws[chunk][pg], rounded once
template <typename IO>
__global__ __launch_bounds__(256) void prefix_cat_sum_kernel(const float* ws, void* dpre, int64_t pgroups, int NC) {
    const int64_t pg = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pg >= pgroups) return;
    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
    const f32x4* w = reinterpret_cast<const f32x4*>(ws) + 2 * pg;
    for (int k = 0; k < NC; ++k) {
        lo += w[2 * k * pgroups];
        hi += w[2 * k * pgroups + 1];
    }
    Vec8<IO> o;
#pragma unroll
    for (int j = 0; j < 4; ++j) { o.set(j, lo[j]); o.set(4 + j, hi[j]); }
    o.store(dpre, pg);
}

template <typename IO>
static hipError_t launch_prefix_cat_io(const PrefixCatArgs& c, bool bwd, hipStream_t stream) {
    const int gpr = c.d >> 3;
    const bool drop = c.thr != 0;
    const dim3 blk(256);
    if (!bwd) {
        const int64_t groups = c.B * (int64_t)(c.P + c.La + c.Lv) * gpr;
        int64_t blocks = (groups + 255) / 256;
        if (blocks > 256 * 16) blocks = 256 * 16;           // 16 workgroups per CU, grid-stride beyond
        const dim3 grid((unsigned)blocks);
        if (drop) hipLaunchKernelGGL((prefix_cat_fwd_kernel<IO, true>), grid, blk, 0, stream, c);
        else hipLaunchKernelGGL((prefix_cat_fwd_kernel<IO, false>), grid, blk, 0, stream, c);
        return hipGetLastError();
    }
    int64_t n_stream = 0, n_part = 0;
    if (c.a != nullptr || c.v != nullptr) {
        n_stream = (c.B * (int64_t)(c.La + c.Lv) * gpr + 255) / 256;
        if (n_stream > 256 * 16) n_stream = 256 * 16;
    }
    const int64_t pgroups = (int64_t)c.P * gpr;
    if (c.dpre != nullptr) n_part = (pgroups * c.NC + 255) / 256;
    if (n_stream + n_part > 0x7fffffff || (pgroups + 255) / 256 > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(n_stream + n_part));
    if (drop) hipLaunchKernelGGL((prefix_cat_bwd_kernel<IO, true>), grid, blk, 0, stream, c, (int)n_stream);
    else hipLaunchKernelGGL((prefix_cat_bwd_kernel<IO, false>), grid, blk, 0, stream, c, (int)n_stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || c.dpre == nullptr) return e;
    hipLaunchKernelGGL((prefix_cat_sum_kernel<IO>), dim3((unsigned)((pgroups + 255) / 256)), blk, 0, stream, c.ws, c.dpre, pgroups, c.NC);
    return hipGetLastError();
}

hipError_t launch_prefix_cat(const PrefixCatArgs& c, bool bwd, int io_fp32, hipStream_t stream) {
    return io_fp32 ? launch_prefix_cat_io<float>(c, bwd, stream) : launch_prefix_cat_io<__bf16>(c, bwd, stream);
}
