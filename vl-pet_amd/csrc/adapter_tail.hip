// Sequential adapter + residual + norm of one sublayer in ONE launch, inference form (no dropout, nothing saved):
//
//   out = N( res + h + s * ( up( gelu_new( down(h) + b_d ) ) + b_u ) )        N = LayerNorm(gamma, beta, eps) | identity
//
// Reference op chains replaced: adapters/adapter_controller.py:149-162 (``adapter(z) + inputs``) followed by
// my_transformers/modeling_bart.py:1259-1261 / :1660-1661, 1717-1718, 1759-1760 (dropout off, residual add, LayerNorm) or
// my_transformers/modeling_t5.py:363-364, 779-780, 886-887 (residual add).  Composed it is K2 (pet_fwd.hip) + K5 (tail.hip): two
// launches and an [M, d] round trip in the IO dtype between them.  This form is for the cached decode step, where M = batch (x beams)
// rows and every launch is a fixed latency.
//
// Structure: workgroup = 8 waves x ONE 16-row tile on v_mfma_f32_16x16x32_bf16, so that a few hundred rows still spread over
// 16 .. 32 workgroups.  Operand fragments of both products are 8 contiguous elements of a row of h / W_down / W_up: read straight from
// global memory (the weights are the adapter's own parameters in their own dtype -- no packed image, nothing derived to keep fresh).
//   1. down: the waves split K = d; each keeps a [16 x r] partial in registers, the eight partials meet in LDS and are summed in
//      the fixed order w0, w1, .. w7; + b_d, gelu_new in fp32, rounded to the operand planes, left in LDS as the A operand;
//   2. up:   the waves split the d output columns; s * (u + b_u) goes to an fp32 [16 x d] LDS tile (it aliases the partials);
//   3. rows: wave w owns rows 2w, 2w + 1: v = (res + h) + tile in fp32, two-pass statistics by a butterfly over the wave, whole
//      512-byte (bf16: 4 elements per lane) row segments stored.
// Roundings (tests/adapter_tail_spec.py restates them): bf16 IO -- h and both weights as bf16 (fp32 parameters are rounded once on
// load), z rounded to bf16, everything else fp32, the result rounded once.  fp32 IO -- h, the weights and z as bf16 hi + lo planes,
// three MFMAs per product (hi*hi + hi*lo + lo*hi), as in the other PET kernels (common.h).
// No atomics, no waits on other workgroups, no host reads: a row's bits depend on that row and the parameters alone.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int AT_ROWS = 16, AT_WAVES = 8, AT_THREADS = 64 * AT_WAVES;

template <typename IO, int D, int R>
struct AtGeo {
    static constexpr int NS = IoTraits<IO>::NS;
    static constexpr int NTD = (R + 15) / 16;                 // 16-column tiles of the down product
    static constexpr int RPAD = 16 * NTD;
    static constexpr int RP = (R + 31) / 32 * 32;             // K of the up product
    static constexpr int KSD = D / 32;                        // k-steps of the down product ...
    static constexpr int KPW = (KSD + AT_WAVES - 1) / AT_WAVES;   // ... per wave
    static constexpr int KSU = RP / 32;
    static constexpr int NTU = D / 16;                        // 16-column tiles of the up product ...
    static constexpr int NPW = (NTU + AT_WAVES - 1) / AT_WAVES;   // ... per wave
    static constexpr int ZS = RP + 8;                         // z row stride (bf16 elements; 16-byte multiple)
    static constexpr int XS = D + 4;                          // up-tile row stride (floats; 16-byte multiple)
    static constexpr int NJ = (D + 255) / 256;                // 4-element pieces per lane and row
    static constexpr int PART_B = AT_WAVES * AT_ROWS * RPAD * 4;
    static constexpr int X_B = AT_ROWS * XS * 4;
    static constexpr int U_B = PART_B > X_B ? PART_B : X_B;
    static constexpr int Z_B = NS * AT_ROWS * ZS * 2;
    static_assert(D % 64 == 0 && R % 8 == 0 && AT_ROWS % AT_WAVES == 0, "geometry");
    static_assert(U_B + Z_B <= 64 * 1024, "static LDS");
};

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <int NS>
__device__ __forceinline__ f32x4 mfma16_ns(const Frag<NS>& a, const Frag<NS>& b, f32x4 c) {
    if constexpr (NS == 2) {
        c = mfma16(a.p[1], b.p[0], c);
        c = mfma16(a.p[0], b.p[1], c);
    }
    return mfma16(a.p[0], b.p[0], c);
}
template <int NS>
__device__ __forceinline__ Frag<NS> zero_frag() {
    Frag<NS> f;
#pragma unroll
    for (int p = 0; p < NS; ++p)
#pragma unroll
        for (int j = 0; j < 8; ++j) f.p[p][j] = (__bf16)0.f;
    return f;
}
// 8 contiguous elements of either dtype as an operand fragment of NS planes
template <int NS, typename T>
__device__ __forceinline__ Frag<NS> frag8(const T* p) {
    float v[8];
    load8_f32(p, v);
    return frag_from_f32<NS>(v);
}
__device__ __forceinline__ f32x4 load4_f32(const __bf16* p) {
    const bf16x4 t = *reinterpret_cast<const bf16x4*>(p);
    f32x4 v = {(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
    return v;
}
__device__ __forceinline__ f32x4 load4_f32(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void store4_f32(__bf16* p, f32x4 v) {
    bf16x4 t = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    *reinterpret_cast<bf16x4*>(p) = t;
}
__device__ __forceinline__ void store4_f32(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ float wave_sum(float v) {      // butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename IO, typename W, int D, int R>
__global__ __launch_bounds__(AT_THREADS) void adapter_tail_kernel(AdapterTailArgs a) {
    using G = AtGeo<IO, D, R>;
    constexpr int NS = G::NS;
    __shared__ __attribute__((aligned(16))) uint8_t smem[G::U_B + G::Z_B];
    float* part = reinterpret_cast<float*>(smem);             // [wave][16][RPAD]   (phase 1)
    float* xt = reinterpret_cast<float*>(smem);               // [16][XS]           (phases 2, 3: the partials are dead by then)
    __bf16* zt = reinterpret_cast<__bf16*>(smem + G::U_B);    // [plane][16][ZS]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * AT_ROWS;
    const IO* h = reinterpret_cast<const IO*>(a.h);
    const IO* res = reinterpret_cast<const IO*>(a.res);
    IO* out = reinterpret_cast<IO*>(a.out);
    const W* wd = reinterpret_cast<const W*>(a.wd);
    const W* wu = reinterpret_cast<const W*>(a.wu);
    const W* bd = reinterpret_cast<const W*>(a.bd);
    const W* bu = reinterpret_cast<const W*>(a.bu);

    // ---- 1. down product: acc[nt][reg] = partial of pre[row 4g + reg][n = 16 nt + li] over this wave's k-steps
    f32x4 acc[G::NTD];
#pragma unroll
    for (int nt = 0; nt < G::NTD; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
        const int64_t arow = row0 + li < a.M ? row0 + li : a.M - 1;       // rows past M: a copy of the last row, never stored
        const IO* hrow = h + arow * D + 8 * g;
#pragma unroll
        for (int kk = 0; kk < G::KPW; ++kk) {
            const int ks = wave * G::KPW + kk;
            if (ks < G::KSD) {
                const Frag<NS> fa = frag8<NS>(hrow + 32 * ks);
#pragma unroll
                for (int nt = 0; nt < G::NTD; ++nt) {
                    const int n = 16 * nt + li;
                    Frag<NS> fb = zero_frag<NS>();
                    if (n < R) fb = frag8<NS>(wd + (int64_t)n * D + 32 * ks + 8 * g);
                    acc[nt] = mfma16_ns<NS>(fa, fb, acc[nt]);
                }
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < G::NTD; ++nt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) part[(wave * AT_ROWS + 4 * g + reg) * G::RPAD + 16 * nt + li] = acc[nt][reg];
    __syncthreads();
    for (int e = tid; e < AT_ROWS * G::RP; e += AT_THREADS) {
        const int row = e / G::RP, n = e % G::RP;
        float v = 0.f;
        if (n < R) {
            const float* p = part + row * G::RPAD + n;
            float s = p[0];
#pragma unroll
            for (int w = 1; w < AT_WAVES; ++w) s += p[w * AT_ROWS * G::RPAD];      // fixed order: wave 0, 1, ..
            v = gelu_new_f(s + (float)bd[n]);
        }
        const __bf16 hi = (__bf16)v;
        zt[row * G::ZS + n] = hi;
        if constexpr (NS == 2) zt[(AT_ROWS + row) * G::ZS + n] = (__bf16)(v - (float)hi);
    }
    __syncthreads();

    // ---- 2. up product: this wave's NPW column tiles; s * (u + b_u) -> the fp32 tile
    {
        Frag<NS> za[G::KSU];
#pragma unroll
        for (int ks = 0; ks < G::KSU; ++ks)
#pragma unroll
            for (int p = 0; p < NS; ++p)
                za[ks].p[p] = *reinterpret_cast<const bf16x8*>(zt + (p * AT_ROWS + li) * G::ZS + 32 * ks + 8 * g);
#pragma unroll
        for (int t = 0; t < G::NPW; ++t) {
            if (wave * G::NPW + t >= G::NTU) break;              // (wave-uniform: narrow models have fewer tiles than waves)
            const int c = 16 * (wave * G::NPW + t) + li;
            f32x4 u = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < G::KSU; ++ks) {
                const int k0 = 32 * ks + 8 * g;
                Frag<NS> fb = zero_frag<NS>();
                if (k0 < R) fb = frag8<NS>(wu + (int64_t)c * R + k0);
                u = mfma16_ns<NS>(za[ks], fb, u);
            }
            const float b = (float)bu[c];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) xt[(4 * g + reg) * G::XS + c] = a.scale * (u[reg] + b);
        }
    }
    __syncthreads();

    // ---- 3. rows: residual adds, norm, store
    for (int rr = 0; rr < AT_ROWS / AT_WAVES; ++rr) {
        const int row = (AT_ROWS / AT_WAVES) * wave + rr;
        const int64_t grow = row0 + row;
        if (grow >= a.M) break;                                 // (wave-uniform)
        f32x4 v[G::NJ];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < G::NJ; ++j) {
            const int c = 4 * lane + 256 * j;
            v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c < D) {
                const f32x4 r4 = load4_f32(res + grow * D + c), h4 = load4_f32(h + grow * D + c);
                const f32x4 x4 = *reinterpret_cast<const f32x4*>(xt + row * G::XS + c);
                v[j] = (r4 + h4) + x4;
                s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
            }
        }
        float mean = 0.f, rstd = 1.f;
        if (a.norm) {
            mean = wave_sum(s) * (1.0f / D);
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < G::NJ; ++j) {
                if (4 * lane + 256 * j < D) {
                    const f32x4 dv = v[j] - mean;
                    q += (dv[0] * dv[0] + dv[1] * dv[1]) + (dv[2] * dv[2] + dv[3] * dv[3]);
                }
            }
            rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / D) + a.eps);
        }
#pragma unroll
        for (int j = 0; j < G::NJ; ++j) {
            const int c = 4 * lane + 256 * j;
            if (c < D) {
                f32x4 o = v[j];
                if (a.norm) {
                    const f32x4 gm = *reinterpret_cast<const f32x4*>(a.gamma + c);
                    o = (o - mean) * rstd * gm;
                    if (a.beta != nullptr) o += *reinterpret_cast<const f32x4*>(a.beta + c);
                }
                store4_f32(out + grow * D + c, o);
            }
        }
    }
}

template <typename IO, typename W>
hipError_t launch_geo(const AdapterTailArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.M + AT_ROWS - 1) / AT_ROWS)), block(AT_THREADS);
    if (a.d == 768 && a.r == 96) hipLaunchKernelGGL((adapter_tail_kernel<IO, W, 768, 96>), grid, block, 0, stream, a);
    else if (a.d == 64 && a.r == 8) hipLaunchKernelGGL((adapter_tail_kernel<IO, W, 64, 8>), grid, block, 0, stream, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace

int adapter_tail_rows(void) { return AT_ROWS; }

bool adapter_tail_geometry_ok(int d, int r) { return (d == 768 && r == 96) || (d == 64 && r == 8); }

hipError_t launch_adapter_tail(const AdapterTailArgs& a, int io_fp32, int param_fp32, hipStream_t stream) {
    if (io_fp32) return param_fp32 ? launch_geo<float, float>(a, stream) : launch_geo<float, __bf16>(a, stream);
    return param_fp32 ? launch_geo<__bf16, float>(a, stream) : launch_geo<__bf16, __bf16>(a, stream);
}
