// FFN activation + dropout of the frozen backbone, the step between fc1 and fc2 in the sublayer that K1 / K5 close:
//     out = dropout(act(x), p)           act = gelu (erf form, F.gelu) | gelu_new (tanh form) | relu
// (my_transformers/modeling_bart.py:1264-1265, 1750-1756; my_transformers/modeling_t5.py:262-265).  In the reference this
// is two elementwise passes forward (activation, dropout) and two backward, and autograd keeps x, act(x) and a byte mask
// alive; here one pass each way over [M, d_ff], only x is kept, and the mask comes from the same counter-based generator
// as K5 / K3 (rng.h): group of 8 consecutive elements -> one Philox call, regenerated in the backward.
// Pure streaming: 2 B in + 2 B out per element forward, 4 B in + 2 B out backward (bf16).
#include "common.h"
#include "kernels.h"
#include "rng.h"
#include "vec8.h"
#include "act_math.h"      // act_f / act_df: shared with the column-summing backward of biasgrad.hip

template <typename IO, int ACT, bool DROP, bool BWD>
__global__ __launch_bounds__(256) void act_dropout_kernel(ActDropArgs a) {
    const int64_t groups = a.n >> 3;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t seed = DROP ? vlpet_eff_seed(a.seed, a.seed_ctr) : 0;
    // two groups per thread and iteration, both loads (four in the backward) issued before the arithmetic of either
    for (int64_t g0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g0 < groups; g0 += 2 * stride) {
        const int64_t g1 = g0 + stride;
        const bool two = g1 < groups;
        Vec8<IO> x[2], dy[2];
        x[0].load(a.x, g0);
        if (two) x[1].load(a.x, g1);
        if constexpr (BWD) {
            dy[0].load(a.dy, g0);
            if (two) dy[1].load(a.dy, g1);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u == 1 && !two) break;
            const int64_t g = u == 0 ? g0 : g1;
            Vec8<IO> o;
            uint32_t bits = 0xffu;
            if constexpr (DROP) bits = keep8(g, seed, a.thr);
            if constexpr (BWD) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float k = ((bits >> j) & 1u) ? a.keep_scale : 0.f;
                    o.set(j, dy[u].get(j) * k * act_df<ACT>(x[u].get(j)));
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float k = ((bits >> j) & 1u) ? a.keep_scale : 0.f;
                    o.set(j, act_f<ACT>(x[u].get(j)) * k);
                }
                if (a.keep_out != nullptr) drop_export8(a.keep_out, g << 3, bits);
            }
            o.store(a.out, g);
        }
    }
}

template <typename IO, int ACT>
static hipError_t launch_act(const ActDropArgs& a, bool bwd, hipStream_t stream) {
    const int64_t groups = a.n >> 3;
    if (groups == 0) return hipSuccess;
    int64_t blocks = (groups + 255) / 256;
    const int64_t cap = 256 * 16;                     // 16 workgroups per CU, grid-stride beyond
    if (blocks > cap) blocks = cap;
    const bool drop = a.thr != 0;
    const dim3 grid((unsigned)blocks), blk(256);
    if (bwd) {
        if (drop) hipLaunchKernelGGL((act_dropout_kernel<IO, ACT, true, true>), grid, blk, 0, stream, a);
        else hipLaunchKernelGGL((act_dropout_kernel<IO, ACT, false, true>), grid, blk, 0, stream, a);
    } else {
        if (drop) hipLaunchKernelGGL((act_dropout_kernel<IO, ACT, true, false>), grid, blk, 0, stream, a);
        else hipLaunchKernelGGL((act_dropout_kernel<IO, ACT, false, false>), grid, blk, 0, stream, a);
    }
    return hipGetLastError();
}

template <typename IO>
static hipError_t launch_act_io(const ActDropArgs& a, bool bwd, hipStream_t stream) {
    switch (a.act) {
        case VLPET_ACT_GELU: return launch_act<IO, VLPET_ACT_GELU>(a, bwd, stream);
        case VLPET_ACT_GELU_NEW: return launch_act<IO, VLPET_ACT_GELU_NEW>(a, bwd, stream);
        case VLPET_ACT_RELU: return launch_act<IO, VLPET_ACT_RELU>(a, bwd, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_act_dropout(const ActDropArgs& a, bool bwd, int io_fp32, hipStream_t stream) {
    return io_fp32 ? launch_act_io<float>(a, bwd, stream) : launch_act_io<__bf16>(a, bwd, stream);
}

// ------------------------------------------------------------------------------------------------ joint-encoder input assembly
// x = dropout(cat([a, v], dim = 1), p): a [B, La, d] (the embedded, layer-normed text), v [B, Lv, d] (the visual embedding, K4's output),
// x [B, La + Lv, d] -- src/modeling_bart.py:804-820 (JointEncoder.forward: inputs_embeds = cat([inputs_embeds, vis_embeds], dim=1), then
// F.dropout); T5: src/modeling_t5.py:263, 300.  The library chain is a concatenation pass, a dropout pass that also writes a byte mask,
// and in the backward a masked-scale pass plus one copy per slice of the gradient; here one pass each way, the mask regenerated
// (rng.h, keyed by the element index of x).  BWD: dx -> da, dv (either may be nullptr: no gradient wanted).
struct CatDropArgs {
    const void* a; const void* v; void* x;      // forward: a, v in, x out.  backward: x = dx in, a / v = da / dv out
    int64_t B; int La, Lv, d;
    uint32_t thr; float keep_scale; uint64_t seed; const uint64_t* seed_ctr;
};
template <typename IO, bool DROP, bool BWD>
__global__ __launch_bounds__(256) void cat_dropout_kernel(CatDropArgs c) {
    const int gpr = c.d >> 3, L = c.La + c.Lv;                     // groups of 8 elements per row
    const int64_t groups = c.B * (int64_t)L * gpr;
    const uint64_t seed = DROP ? vlpet_eff_seed(c.seed, c.seed_ctr) : 0;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = g / gpr;
        const int col = (int)(g - row * gpr);
        const int64_t b = row / L;
        const int t = (int)(row - b * L);
        const bool text = t < c.La;
        const int64_t sg = text ? (b * c.La + t) * (int64_t)gpr + col : (b * c.Lv + (t - c.La)) * (int64_t)gpr + col;     // group index inside a / v
        void* side = const_cast<void*>(text ? c.a : c.v);
        uint32_t bits = 0xffu;
        if constexpr (DROP) bits = keep8(g, seed, c.thr);
        Vec8<IO> in, o;
        if constexpr (BWD) {
            if (side == nullptr) continue;
            in.load(c.x, g);
        } else in.load(side, sg);
#pragma unroll
        for (int j = 0; j < 8; ++j) o.set(j, ((bits >> j) & 1u) ? in.get(j) * c.keep_scale : 0.f);
        if constexpr (BWD) o.store(side, sg);
        else o.store(c.x, g);
    }
}
hipError_t launch_cat_dropout(const void* a, const void* v, void* x, int64_t B, int La, int Lv, int d, uint32_t thr, float keep_scale,
                              uint64_t seed, const uint64_t* seed_ctr, bool bwd, int io_fp32, hipStream_t stream) {
    CatDropArgs c{a, v, x, B, La, Lv, d, thr, keep_scale, seed, seed_ctr};
    const int64_t groups = B * (int64_t)(La + Lv) * (d >> 3);
    if (groups == 0) return hipSuccess;
    int64_t blocks = (groups + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const dim3 grid((unsigned)blocks), blk(256);
    const bool drop = thr != 0;
#define VLPET_CD(IO) \
    if (bwd) { if (drop) hipLaunchKernelGGL((cat_dropout_kernel<IO, true, true>), grid, blk, 0, stream, c); \
               else hipLaunchKernelGGL((cat_dropout_kernel<IO, false, true>), grid, blk, 0, stream, c); } \
    else { if (drop) hipLaunchKernelGGL((cat_dropout_kernel<IO, true, false>), grid, blk, 0, stream, c); \
           else hipLaunchKernelGGL((cat_dropout_kernel<IO, false, false>), grid, blk, 0, stream, c); }
    if (io_fp32) { VLPET_CD(float) } else { VLPET_CD(__bf16) }
#undef VLPET_CD
    return hipGetLastError();
}
