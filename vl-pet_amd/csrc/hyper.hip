// Hyperformer's weight generator for one stack: S linear maps applied to the same E embedding rows in ONE launch, and its backward.
//
//   map s: G_s [n_s, P], g_s [n_s] (nn.Linear layout, parameter dtype)       e [E, P] fp32
//   out_s[l, i] = g_s[i] + sum_p G_s[i, p] e[l, p]                            out_s [E, n_s] parameter dtype, fp32 sums
//   dG_s[i, p] = sum_l dout[s][l][i] e[l, p]     dg_s[i] = sum_l dout[s][l][i]     de[l, p] = sum_s sum_i dout[s][l][i] G_s[i, p]
//
// Reference op chain replaced (adapters/adapter_hypernetwork.py: AdapterLayersHyperNet.forward -- per layer and block four
// nn.Linear(P -> r d | r | d) generators on one embedding row, each followed by a view): every layer's row of every generator here.
// Row l of a weight generator's output, viewed [r, d] or [d, r], is the nn.Linear layout K2 / K1 / adapter_tail take.
//
// Structure, both directions: a streaming kernel, no matrix cores (at P = 8 a row of G_s is 32 bytes; each is read once).  A workgroup
// owns HYP_ROWS consecutive rows i of ONE map (the grid is the row slabs of map 0, then those of map 1, ..); a lane owns one row, read
// with 16-byte loads where the row is a multiple of 16 bytes, and keeps it in registers.  e (<= 4,096 floats) sits in LDS and is read
// at wave-uniform addresses.
//   forward:   the lane forms the E sums of P products (p ascending, then the bias) and stores out_s[l, i]: along i across the lanes.
//   backward:  dG_s[i, :] and dg_s[i] are complete inside the lane (l ascending) and stored into the caller's sinks;
//              the slab's part of de[l, :] is reduced over the lanes of a wave by a halving butterfly (the lanes trade halves of the
//              P values at distances 32, 16, .., then sum what is left at the remaining distances), over the four waves through LDS in
//              the order w0 .. w3, and left in the workspace: [slab][l][p];
//              a second small launch sums the slabs' partials: 16 runs of consecutive slabs, each in slab order, then the runs in order.
// No atomics, no waits on other workgroups, no host reads: the bits depend on the inputs and the geometry alone.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int HYP_SUM_RUNS = 16, HYP_SUM_COLS = 16;        // the second launch: 256 threads = 16 runs of slabs x 16 (l, p) columns

template <bool F32>
__device__ __forceinline__ float hyp_ld(const void* p, size_t i) {
    if constexpr (F32) return reinterpret_cast<const float*>(p)[i];
    else return (float)reinterpret_cast<const __bf16*>(p)[i];
}
template <bool F32>
__device__ __forceinline__ void hyp_st(void* p, size_t i, float v) {
    if constexpr (F32) reinterpret_cast<float*>(p)[i] = v;
    else reinterpret_cast<__bf16*>(p)[i] = (__bf16)v;
}

// the map whose slabs hold workgroup `blk` (S <= 16: a wave-uniform scan of the kernel arguments)
template <class Args>
__device__ __forceinline__ int hyp_map_of(const Args& a, int blk) {
    int s = 0;
#pragma unroll 1
    for (int k = 1; k < a.S; ++k)
        if (blk >= a.m[k].blk0) s = k;
    return s;
}

// row i of G [n, P] -> w[0 .. PMAX) as fp32, zeros from P on; `vec`: the row is a whole number of 16-byte pieces
template <bool F32, int PMAX>
__device__ __forceinline__ void hyp_load_row(const void* G, size_t i, int P, bool vec, float (&w)[PMAX]) {
#pragma unroll
    for (int p = 0; p < PMAX; ++p) w[p] = 0.f;
    if (vec) {
        if constexpr (F32) {
            const float4* src = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(G) + i * P);
#pragma unroll
            for (int c = 0; c < PMAX / 4; ++c)
                if (4 * c < P) {
                    const float4 v = src[c];
                    w[4 * c] = v.x; w[4 * c + 1] = v.y; w[4 * c + 2] = v.z; w[4 * c + 3] = v.w;
                }
        } else {
            const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const __bf16*>(G) + i * P);
#pragma unroll
            for (int c = 0; c < PMAX / 8; ++c)
                if (8 * c < P) {
                    const uint4 v = src[c];
                    const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        w[8 * c + 2 * j] = __uint_as_float(u[j] << 16);
                        w[8 * c + 2 * j + 1] = __uint_as_float(u[j] & 0xffff0000u);
                    }
                }
        }
    } else {
#pragma unroll
        for (int p = 0; p < PMAX; ++p)
            if (p < P) w[p] = hyp_ld<F32>(G, i * P + p);
    }
}

__device__ __forceinline__ void hyp_stage_e(const float* e, int count, float* sE) {
    for (int k = threadIdx.x; k < count; k += HYP_ROWS) sE[k] = e[k];
}

template <bool F32, int PMAX>
__global__ __launch_bounds__(HYP_ROWS) void hyper_gen_fwd_kernel(HyperFwdArgs a) {
    __shared__ float sE[HYP_MAX_E * HYP_MAX_P];
    const int s = hyp_map_of(a, (int)blockIdx.x);
    const HyperFwdMap m = a.m[s];
    const int E = a.E, P = a.P;
    hyp_stage_e(a.e, E * P, sE);
    __syncthreads();
    const int i = ((int)blockIdx.x - m.blk0) * HYP_ROWS + (int)threadIdx.x;
    if (i >= m.n) return;
    float w[PMAX];
    hyp_load_row<F32, PMAX>(m.G, (size_t)i, P, (P * (F32 ? 4 : 2)) % 16 == 0, w);
    const float b = hyp_ld<F32>(m.g, (size_t)i);
    for (int l = 0; l < E; ++l) {
        const float* el = sE + l * P;
        float acc = 0.f;
#pragma unroll
        for (int p = 0; p < PMAX; ++p)
            if (p < P) acc = fmaf(w[p], el[p], acc);
        hyp_st<F32>(m.out, (size_t)l * m.n + i, acc + b);
    }
}

// sum over the 64 lanes of v[p], every p: after the call lane L with (L & (64 / N - 1)) == 0 holds in v[0] the sum of p = L / (64 / N)
// (N = PMAX <= 64, a power of two; H: the values still held, OFF: the lane distance of this step).  N - 1 + log2(64 / N) shuffles
// instead of 6 N.
template <int N, int H, int OFF>
struct HypReduce {
    static __device__ __forceinline__ void run(float (&v)[N], int lane) {
        if constexpr (OFF >= 1) {
            if constexpr (H > 1) {
                constexpr int h = H / 2;
                const bool up = (lane & OFF) != 0;
#pragma unroll
                for (int j = 0; j < h; ++j) {
                    const float keep = up ? v[j + h] : v[j], send = up ? v[j] : v[j + h];
                    v[j] = keep + __shfl_xor(send, OFF, 64);
                }
                HypReduce<N, h, OFF / 2>::run(v, lane);
            } else {
                v[0] += __shfl_xor(v[0], OFF, 64);
                HypReduce<N, 1, OFF / 2>::run(v, lane);
            }
        }
    }
};

template <bool F32, int PMAX>
__global__ __launch_bounds__(HYP_ROWS) void hyper_gen_bwd_kernel(HyperBwdArgs a) {
    __shared__ float sE[HYP_MAX_E * HYP_MAX_P];
    __shared__ float sRed[2][HYP_ROWS / 64][HYP_MAX_P];           // [l & 1][wave][p]
    const int blk = (int)blockIdx.x, s = hyp_map_of(a, blk);
    const HyperBwdMap m = a.m[s];
    const int E = a.E, P = a.P, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    hyp_stage_e(a.e, E * P, sE);
    __syncthreads();
    const int i = (blk - m.blk0) * HYP_ROWS + tid;
    const bool valid = i < m.n;
    float w[PMAX], accG[PMAX];
    if (valid) hyp_load_row<F32, PMAX>(m.G, (size_t)i, P, (P * (F32 ? 4 : 2)) % 16 == 0, w);
    else {
#pragma unroll
        for (int p = 0; p < PMAX; ++p) w[p] = 0.f;
    }
#pragma unroll
    for (int p = 0; p < PMAX; ++p) accG[p] = 0.f;
    float accg = 0.f;
    constexpr int LANES_PER_P = 64 / PMAX;                        // lanes that end up with the same column's sum
    float* part = a.ws + (size_t)blk * E * P;
    const float* const* rows = a.dout + s * E;
    const float* gp = rows[0];
    float gnext = (gp && valid) ? gp[i] : 0.f;
    for (int l = 0; l < E; ++l) {
        const float gv = gnext;
        if (l + 1 < E) {                                          // the next row's element is in flight across this row's barrier
            gp = rows[l + 1];
            gnext = (gp && valid) ? gp[i] : 0.f;
        }
        const float* el = sE + l * P;
        accg += gv;
        float t[PMAX];
#pragma unroll
        for (int p = 0; p < PMAX; ++p) {
            accG[p] = fmaf(gv, p < P ? el[p] : 0.f, accG[p]);
            t[p] = gv * w[p];
        }
        HypReduce<PMAX, PMAX, 32>::run(t, lane);
        const int col = lane / LANES_PER_P;
        if ((lane & (LANES_PER_P - 1)) == 0 && col < P) sRed[l & 1][wave][col] = t[0];
        __syncthreads();                                          // (the other half of sRed is last read before the barrier of row l - 1)
        if (tid < P) {
            const float* q = &sRed[l & 1][0][tid];
            part[l * P + tid] = ((q[0] + q[HYP_MAX_P]) + q[2 * HYP_MAX_P]) + q[3 * HYP_MAX_P];
        }
    }
    if (!valid) return;
    m.dg[i] = accg;
    float* dst = m.dG + (size_t)i * P;
    if (P % 4 == 0) {
#pragma unroll
        for (int c = 0; c < PMAX / 4; ++c)
            if (4 * c < P) reinterpret_cast<float4*>(dst)[c] = make_float4(accG[4 * c], accG[4 * c + 1], accG[4 * c + 2], accG[4 * c + 3]);
    } else {
#pragma unroll
        for (int p = 0; p < PMAX; ++p)
            if (p < P) dst[p] = accG[p];
    }
}

// de[c] (c = l P + p) = the slabs' partials: HYP_SUM_RUNS runs of consecutive slabs, each summed in slab order, then the runs in order
__global__ __launch_bounds__(HYP_SUM_RUNS * HYP_SUM_COLS) void hyper_de_sum_kernel(const float* ws, float* de, int slabs, int EP) {
    __shared__ float sRun[HYP_SUM_RUNS][HYP_SUM_COLS];
    const int cj = (int)threadIdx.x % HYP_SUM_COLS, run = (int)threadIdx.x / HYP_SUM_COLS;
    const int c = (int)blockIdx.x * HYP_SUM_COLS + cj;
    const int per = (slabs + HYP_SUM_RUNS - 1) / HYP_SUM_RUNS;
    const int b0 = run * per, b1 = min(slabs, b0 + per);
    float sum = 0.f;
    if (c < EP)
        for (int b = b0; b < b1; ++b) sum += ws[(size_t)b * EP + c];
    sRun[run][cj] = sum;
    __syncthreads();
    if (run == 0 && c < EP) {
        float tot = sRun[0][cj];
#pragma unroll
        for (int k = 1; k < HYP_SUM_RUNS; ++k) tot += sRun[k][cj];
        de[c] = tot;
    }
}

template <bool F32, class Args>
hipError_t hyp_launch_fwd(const Args& a, int blocks, hipStream_t stream) {
    const int P = a.P;
    if (P <= 8) hipLaunchKernelGGL((hyper_gen_fwd_kernel<F32, 8>), dim3(blocks), dim3(HYP_ROWS), 0, stream, a);
    else if (P <= 16) hipLaunchKernelGGL((hyper_gen_fwd_kernel<F32, 16>), dim3(blocks), dim3(HYP_ROWS), 0, stream, a);
    else if (P <= 32) hipLaunchKernelGGL((hyper_gen_fwd_kernel<F32, 32>), dim3(blocks), dim3(HYP_ROWS), 0, stream, a);
    else hipLaunchKernelGGL((hyper_gen_fwd_kernel<F32, 64>), dim3(blocks), dim3(HYP_ROWS), 0, stream, a);
    return hipGetLastError();
}

template <bool F32, class Args>
hipError_t hyp_launch_bwd(const Args& a, int blocks, hipStream_t stream) {
    const int P = a.P;
    if (P <= 8) hipLaunchKernelGGL((hyper_gen_bwd_kernel<F32, 8>), dim3(blocks), dim3(HYP_ROWS), 0, stream, a);
    else if (P <= 16) hipLaunchKernelGGL((hyper_gen_bwd_kernel<F32, 16>), dim3(blocks), dim3(HYP_ROWS), 0, stream, a);
    else if (P <= 32) hipLaunchKernelGGL((hyper_gen_bwd_kernel<F32, 32>), dim3(blocks), dim3(HYP_ROWS), 0, stream, a);
    else hipLaunchKernelGGL((hyper_gen_bwd_kernel<F32, 64>), dim3(blocks), dim3(HYP_ROWS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_hyper_gen_fwd(const HyperFwdArgs& a, int blocks, int param_fp32, hipStream_t stream) {
    return param_fp32 ? hyp_launch_fwd<true>(a, blocks, stream) : hyp_launch_fwd<false>(a, blocks, stream);
}

hipError_t launch_hyper_gen_bwd(const HyperBwdArgs& a, int blocks, int param_fp32, hipStream_t stream) {
    hipError_t e = param_fp32 ? hyp_launch_bwd<true>(a, blocks, stream) : hyp_launch_bwd<false>(a, blocks, stream);
    if (e != hipSuccess) return e;
    const int EP = a.E * a.P;
    hipLaunchKernelGGL(hyper_de_sum_kernel, dim3((EP + HYP_SUM_COLS - 1) / HYP_SUM_COLS), dim3(HYP_SUM_RUNS * HYP_SUM_COLS), 0, stream,
                       (const float*)a.ws, a.de, blocks, EP);
    return hipGetLastError();
}
