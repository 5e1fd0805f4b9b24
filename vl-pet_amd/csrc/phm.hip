// Compacter's weight expansion for one adapter: the (down, up) pair of PHM layers in ONE launch, and its backward.
//
//   PHMLinear(in, out, n):  rule A [n, n, n],  W [n, k, p]   (k = in / n, p = out / n)
//   H[a k + kk, c p + pp] = sum_i A[i, a, c] W[i, kk, pp]           y = x H + b
//
// Reference op chain replaced (adapters/hypercomplex/layers.py:25-33, kronecker.py:22-33): einsum('bac,bkp->bakcp') -> view -> sum(0),
// then a separate x @ H per layer.  Here only H^T is made, in the nn.Linear layout [out, in] that K2 / K1 / adapter_tail take as
// their weight; the [M, d] work stays in those kernels.
//
// Structure, both directions: a workgroup owns a 32 x 32 (kk, pp) tile of ALL n slices of W of one layer (the grid is the tiles of the
// down layer followed by those of the up layer).  W is contiguous along pp, H^T along kk: the tile goes through LDS once (row stride
// 33 floats), so that global reads of W and global accesses of H^T / dH^T are both along whole lines.  The rule (<= 512 floats) sits in
// LDS and is read at wave-uniform addresses.
//   forward:   grid.y = a: thread (kk, pp) forms the n sums (over c) of n products and stores them at H^T[c p + pp, a k + kk]; the n
//              workgroups of a tile each stage it again (from L2) -- at n >= 4 a layer has only a handful of tiles.
//   backward:  dW[i, kk, pp] = sum_{a, c} A[i, a, c] dH^T[c p + pp, a k + kk]     complete inside the workgroup (registers, then
//                                                                                   through LDS for stores along pp);
//              dA[i, a, c]   = sum_{kk, pp} dH^T[c p + pp, a k + kk] W[i, kk, pp]  each workgroup leaves n^3 partials (lanes by a
//                                                                                   butterfly, the four waves in the order w0 .. w3),
//              a second small launch sums the workgroups' partials in block order.
// No atomics, no waits on other workgroups, no host reads: the bits depend on the inputs and the geometry alone.
// Arithmetic is fp32; parameters are fp32 or bf16 (read once, widened); the forward's outputs take the parameters' dtype.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int PHM_TK = 32, PHM_TP = 32, PHM_THREADS = 256, PHM_MAXN = 8, PHM_LDW = PHM_TP + 1, PHM_PPT = PHM_TP / 8;

template <bool F32>
__device__ __forceinline__ float phm_ld(const void* p, size_t i) {
    if constexpr (F32) return reinterpret_cast<const float*>(p)[i];
    else return (float)reinterpret_cast<const __bf16*>(p)[i];
}
template <bool F32>
__device__ __forceinline__ void phm_st(void* p, size_t i, float v) {
    if constexpr (F32) reinterpret_cast<float*>(p)[i] = v;
    else reinterpret_cast<__bf16*>(p)[i] = (__bf16)v;
}

struct PhmTile { int in, out, k, p, k0, p0; };

// which layer and which tile of it this workgroup owns (tiles of layer 0 first)
__device__ __forceinline__ PhmTile phm_tile(const PhmArgs& a, int tiles0, int li) {
    PhmTile t;
    t.in = li ? a.l[1].in : a.l[0].in;
    t.out = li ? a.l[1].out : a.l[0].out;
    t.k = t.in / a.n;
    t.p = t.out / a.n;
    const int tile = (int)blockIdx.x - (li ? tiles0 : 0);
    const int tps = (t.p + PHM_TP - 1) / PHM_TP;
    t.k0 = (tile / tps) * PHM_TK;
    t.p0 = (tile % tps) * PHM_TP;
    return t;
}

// rule -> sA[n^3], the tile of every slice of W -> sW[i][kk][pp] (zero outside the layer)
template <bool F32>
__device__ __forceinline__ void phm_stage(const void* rule, const void* W, const PhmTile& t, int n, float* sA, float* sW) {
    const int tid = threadIdx.x;
    for (int e = tid; e < n * n * n; e += PHM_THREADS) sA[e] = phm_ld<F32>(rule, e);
    for (int e = tid; e < n * PHM_TK * PHM_TP; e += PHM_THREADS) {
        const int pp = e % PHM_TP, kk = (e / PHM_TP) % PHM_TK, i = e / (PHM_TK * PHM_TP);
        float v = 0.f;
        if (t.k0 + kk < t.k && t.p0 + pp < t.p) v = phm_ld<F32>(W, ((size_t)i * t.k + t.k0 + kk) * t.p + t.p0 + pp);
        sW[(i * PHM_TK + kk) * PHM_LDW + pp] = v;
    }
}

template <bool F32>
__global__ __launch_bounds__(PHM_THREADS) void phm_expand_fwd_kernel(PhmArgs a, int tiles0) {
    __shared__ float sA[PHM_MAXN * PHM_MAXN * PHM_MAXN];
    __shared__ float sW[PHM_MAXN * PHM_TK * PHM_LDW];
    const int li = (int)blockIdx.x >= tiles0;
    const PhmTile t = phm_tile(a, tiles0, li);
    const int n = a.n;
    phm_stage<F32>(li ? a.l[1].rule : a.l[0].rule, li ? a.l[1].W : a.l[0].W, t, n, sA, sW);
    __syncthreads();
    void* wt = li ? a.l[1].wt : a.l[0].wt;
    const int kk = threadIdx.x % PHM_TK, ppb = threadIdx.x / PHM_TK;
    if (t.k0 + kk >= t.k) return;
    const int aa = blockIdx.y;                                    // the n row blocks of H (columns of H^T) are spread over grid.y
    for (int c = 0; c < n; ++c) {
        const int ac = aa * n + c;
#pragma unroll
        for (int j = 0; j < PHM_PPT; ++j) {
            const int pp = ppb + 8 * j;
            if (t.p0 + pp >= t.p) break;
            float s = 0.f;
            for (int i = 0; i < n; ++i) s = fmaf(sA[i * n * n + ac], sW[(i * PHM_TK + kk) * PHM_LDW + pp], s);
            phm_st<F32>(wt, ((size_t)c * t.p + t.p0 + pp) * t.in + (size_t)aa * t.k + t.k0 + kk, s);
        }
    }
}

template <bool F32>
__global__ __launch_bounds__(PHM_THREADS) void phm_expand_bwd_kernel(PhmArgs a, int tiles0) {
    __shared__ float sA[PHM_MAXN * PHM_MAXN * PHM_MAXN];
    __shared__ float sW[PHM_MAXN * PHM_TK * PHM_LDW];
    __shared__ float sRed[PHM_MAXN * PHM_MAXN * 4 * PHM_MAXN];      // [a c][wave][i]
    const int li = (int)blockIdx.x >= tiles0;
    const PhmTile t = phm_tile(a, tiles0, li);
    const int n = a.n, tid = threadIdx.x;
    phm_stage<F32>(li ? a.l[1].rule : a.l[0].rule, li ? a.l[1].W : a.l[0].W, t, n, sA, sW);
    __syncthreads();
    const float* g = li ? a.l[1].dwt : a.l[0].dwt;
    const int kk = tid % PHM_TK, ppb = tid / PHM_TK, lane = tid & 63, wave = tid >> 6;
    const bool kin = t.k0 + kk < t.k;
    float w[PHM_PPT][PHM_MAXN], acc[PHM_PPT][PHM_MAXN];
#pragma unroll
    for (int j = 0; j < PHM_PPT; ++j)
#pragma unroll
        for (int i = 0; i < PHM_MAXN; ++i) {
            w[j][i] = i < n ? sW[(i * PHM_TK + kk) * PHM_LDW + ppb + 8 * j] : 0.f;
            acc[j][i] = 0.f;
        }
    for (int ac = 0; ac < n * n; ++ac) {
        const int aa = ac / n, c = ac % n;
        float gv[PHM_PPT];
#pragma unroll
        for (int j = 0; j < PHM_PPT; ++j) {
            const int pp = ppb + 8 * j;
            gv[j] = (kin && t.p0 + pp < t.p) ? g[((size_t)c * t.p + t.p0 + pp) * t.in + (size_t)aa * t.k + t.k0 + kk] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < PHM_MAXN; ++i) {
            if (i < n) {                                          // (n is uniform: whole waves take the branch together)
                const float ai = sA[i * n * n + ac];
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < PHM_PPT; ++j) {
                    acc[j][i] = fmaf(ai, gv[j], acc[j][i]);
                    s = fmaf(gv[j], w[j][i], s);
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
                if (lane == 0) sRed[(ac * 4 + wave) * PHM_MAXN + i] = s;
            }
        }
    }
    __syncthreads();                                              // every read of sW (w) is done: it now carries dW out
#pragma unroll
    for (int j = 0; j < PHM_PPT; ++j)
#pragma unroll
        for (int i = 0; i < PHM_MAXN; ++i)
            if (i < n) sW[(i * PHM_TK + kk) * PHM_LDW + ppb + 8 * j] = acc[j][i];
    __syncthreads();
    float* dW = li ? a.l[1].dW : a.l[0].dW;
    for (int e = tid; e < n * PHM_TK * PHM_TP; e += PHM_THREADS) {
        const int pp = e % PHM_TP, k2 = (e / PHM_TP) % PHM_TK, i = e / (PHM_TK * PHM_TP);
        if (t.k0 + k2 < t.k && t.p0 + pp < t.p) dW[((size_t)i * t.k + t.k0 + k2) * t.p + t.p0 + pp] = sW[(i * PHM_TK + k2) * PHM_LDW + pp];
    }
    const int n2 = n * n, n3 = n2 * n;
    for (int e = tid; e < n3; e += PHM_THREADS) {
        const int i = e / n2, ac = e % n2;
        const float* q = sRed + ac * 4 * PHM_MAXN + i;
        a.ws[(size_t)blockIdx.x * n3 + e] = ((q[0] + q[PHM_MAXN]) + q[2 * PHM_MAXN]) + q[3 * PHM_MAXN];
    }
}

// drule of layer blockIdx.x: the partials of its workgroups, in block order
__global__ __launch_bounds__(PHM_THREADS) void phm_rule_sum_kernel(PhmArgs a, int tiles0, int tiles1) {
    const int li = blockIdx.x;
    const int first = li ? tiles0 : 0, count = li ? tiles1 : tiles0;
    float* out = li ? a.l[1].drule : a.l[0].drule;
    const int n3 = a.n * a.n * a.n;
    for (int e = threadIdx.x; e < n3; e += PHM_THREADS) {
        float s = 0.f;
        for (int b = 0; b < count; ++b) s += a.ws[(size_t)(first + b) * n3 + e];
        out[e] = s;
    }
}

}  // namespace

int64_t phm_layer_tiles(int in, int out, int n) {
    const int64_t k = in / n, p = out / n;
    return ((k + PHM_TK - 1) / PHM_TK) * ((p + PHM_TP - 1) / PHM_TP);
}

hipError_t launch_phm_expand_fwd(const PhmArgs& a, int param_fp32, hipStream_t stream) {
    const int t0 = (int)phm_layer_tiles(a.l[0].in, a.l[0].out, a.n), t1 = (int)phm_layer_tiles(a.l[1].in, a.l[1].out, a.n);
    if (param_fp32) hipLaunchKernelGGL(phm_expand_fwd_kernel<true>, dim3(t0 + t1, a.n), dim3(PHM_THREADS), 0, stream, a, t0);
    else hipLaunchKernelGGL(phm_expand_fwd_kernel<false>, dim3(t0 + t1, a.n), dim3(PHM_THREADS), 0, stream, a, t0);
    return hipGetLastError();
}

hipError_t launch_phm_expand_bwd(const PhmArgs& a, int param_fp32, hipStream_t stream) {
    const int t0 = (int)phm_layer_tiles(a.l[0].in, a.l[0].out, a.n), t1 = (int)phm_layer_tiles(a.l[1].in, a.l[1].out, a.n);
    if (param_fp32) hipLaunchKernelGGL(phm_expand_bwd_kernel<true>, dim3(t0 + t1), dim3(PHM_THREADS), 0, stream, a, t0);
    else hipLaunchKernelGGL(phm_expand_bwd_kernel<false>, dim3(t0 + t1), dim3(PHM_THREADS), 0, stream, a, t0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(phm_rule_sum_kernel, dim3(2), dim3(PHM_THREADS), 0, stream, a, t0, t1);
    return hipGetLastError();
}
