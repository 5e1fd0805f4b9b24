// The two kernels of a cached greedy decode step (generate() of host/bart.py and host/t5.py; HF 4.2.1 greedy_search as the
// reference runs it: src/multitask.py test_step -> model.generate(num_beams = 1)).
//
//   vlpet_attn_decode  one query row per sequence against a key / value cache: o = softmax(scale * q k^T + bias + mask) v.
//                      With k_new / v_new the kernel first writes them into cache row `pos` and attends over keys 0..pos: the
//                      decoder self-attention step (append + attention in one launch).  Without them it reads Lk keys in place:
//                      the cross-attention step, whose key cache may be a column block of the decoder's fused key projection.
//   vlpet_greedy_pick  the next token of every row from one read of its logits: the reference's greedy logits processors
//                      (min_length, no_repeat_ngram_size) then the argmax (ties to the lowest index, as torch.argmax), finished
//                      rows emit pad, the unfinished flags and a per-step counter of unfinished rows are updated on device.
//
// Work split of the attention (DESIGN.md "Generation"): one wave per (sequence, head), four waves = four consecutive heads of one
// sequence per workgroup.  There is no contraction worth an MFMA (one query row), so the kernel is bound by the bytes of K and V;
// a wave reads each key row of its head as D * 2 contiguous bytes (bf16), the four waves of a workgroup read neighbouring column
// blocks of the same rows.  Inside a wave, D / 8 lanes hold one key (16-byte loads of 8 elements), so a wave step covers
// 64 / (D / 8) keys; every lane keeps an online softmax (max, sum, 8 accumulators) over the keys of its lane group and the groups
// are merged with cross-lane shuffles at the end.  The loads of U steps are issued before any of them is consumed.
#include "common.h"
#include "../../include/vlpet_hip.h"

#include <climits>

namespace {

template <typename IO> struct Raw8;
template <> struct Raw8<__bf16> {
    bf16x8 v;
    __device__ __forceinline__ void load(const __bf16* p) { v = *reinterpret_cast<const bf16x8*>(p); }
    __device__ __forceinline__ void store(__bf16* p) const { *reinterpret_cast<bf16x8*>(p) = v; }
    __device__ __forceinline__ float get(int j) const { return (float)v[j]; }
};
template <> struct Raw8<float> {
    f32x4 a, b;
    __device__ __forceinline__ void load(const float* p) { a = reinterpret_cast<const f32x4*>(p)[0]; b = reinterpret_cast<const f32x4*>(p)[1]; }
    __device__ __forceinline__ void store(float* p) const { reinterpret_cast<f32x4*>(p)[0] = a; reinterpret_cast<f32x4*>(p)[1] = b; }
    __device__ __forceinline__ float get(int j) const { return j < 4 ? a[j] : b[j - 4]; }
};

template <typename IO> __device__ __forceinline__ IO to_io(float f);
template <> __device__ __forceinline__ __bf16 to_io<__bf16>(float f) { return (__bf16)f; }
template <> __device__ __forceinline__ float to_io<float>(float f) { return f; }

struct DecodeAttnArgs {
    const void* q; int64_t ld_q;
    void* k; void* v; int64_t ld_k, bs_k, ld_v, bs_v;
    const void* k_new; const void* v_new; int64_t ld_new; int pos;
    const uint8_t* mask; int64_t ld_mask;
    const float* bias; int64_t ld_bias;
    void* o; int64_t ld_o;
    int B, H, n_keys;
    float scale;
};

#define DEC_WAVES 4

template <typename IO, int D>
__global__ __launch_bounds__(DEC_WAVES * 64) void attn_decode_kernel(DecodeAttnArgs a) {
    constexpr int LPK = D / 8;                  // lanes per key
    constexpr int KPS = 64 / LPK;               // keys per wave step
    constexpr int U = D == 64 ? 4 : 2;          // steps whose loads are in flight together
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * DEC_WAVES + (threadIdx.x >> 6);
    if (pair >= (int64_t)a.B * a.H) return;     // (no barrier below: a wave without a pair just leaves)
    const int64_t b = pair / a.H;
    const int h = (int)(pair % a.H);
    const int sub = lane % LPK, kj = lane / LPK;
    const int64_t col = (int64_t)h * D + sub * 8;

    Raw8<IO> qr;
    qr.load(reinterpret_cast<const IO*>(a.q) + b * a.ld_q + col);
    float qf[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) qf[d] = qr.get(d) * a.scale;

    IO* kc = reinterpret_cast<IO*>(a.k) + b * a.bs_k + col;
    IO* vc = reinterpret_cast<IO*>(a.v) + b * a.bs_v + col;
    const bool append = a.k_new != nullptr;
    Raw8<IO> kn, vn;
    if (append) {
        kn.load(reinterpret_cast<const IO*>(a.k_new) + b * a.ld_new + col);
        vn.load(reinterpret_cast<const IO*>(a.v_new) + b * a.ld_new + col);
        if (kj == 0) {
            kn.store(kc + (int64_t)a.pos * a.ld_k);
            vn.store(vc + (int64_t)a.pos * a.ld_v);
        }
    }
    const int n = a.n_keys;
    const uint8_t* mrow = a.mask != nullptr ? a.mask + b * a.ld_mask : nullptr;
    const float* brow = a.bias != nullptr ? a.bias + (int64_t)h * a.ld_bias : nullptr;

    float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[d] = 0.f;

    for (int j0 = 0; j0 < n; j0 += KPS * U) {
        Raw8<IO> kr[U], vr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = min(j0 + u * KPS + kj, n - 1);        // (clamped: a key past the end is loaded but not counted)
            if (append && j == a.pos) {                          // the appended row comes from registers, not back from memory
                kr[u] = kn;
                vr[u] = vn;
            } else {
                kr[u].load(kc + (int64_t)j * a.ld_k);
                vr[u].load(vc + (int64_t)j * a.ld_v);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * KPS + kj;
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < 8; ++d) s = fmaf(qf[d], kr[u].get(d), s);
#pragma unroll
            for (int o = 1; o < LPK; o <<= 1) s += __shfl_xor(s, o);
            const bool ok = j < n && (mrow == nullptr || mrow[j] != 0);
            if (ok) {
                if (brow != nullptr) s += brow[j];
                const float mn = fmaxf(m, s);
                const float c = __expf(m - mn);                  // (m = -inf before the first key: c = 0)
                const float p = __expf(s - mn);
                l = fmaf(l, c, p);
#pragma unroll
                for (int d = 0; d < 8; ++d) acc[d] = fmaf(acc[d], c, p * vr[u].get(d));
                m = mn;
            }
        }
    }
    // merge the KPS lane groups (lanes with the same `sub`)
#pragma unroll
    for (int o = LPK; o < 64; o <<= 1) {
        const float mo = __shfl_xor(m, o), lo = __shfl_xor(l, o);
        const float M = fmaxf(m, mo);
        const float c1 = m == -INFINITY ? 0.f : __expf(m - M);
        const float c2 = mo == -INFINITY ? 0.f : __expf(mo - M);
        l = l * c1 + lo * c2;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const float ao = __shfl_xor(acc[d], o);
            acc[d] = acc[d] * c1 + ao * c2;
        }
        m = M;
    }
    if (kj == 0) {
        const float inv = l > 0.f ? 1.f / l : 0.f;               // (every key masked: zeros)
        IO* orow = reinterpret_cast<IO*>(a.o) + b * a.ld_o + col;
        if constexpr (sizeof(IO) == 2) {
            bf16x8 w;
#pragma unroll
            for (int d = 0; d < 8; ++d) w[d] = (__bf16)(acc[d] * inv);
            *reinterpret_cast<bf16x8*>(orow) = w;
        } else {
            f32x4 w0, w1;
#pragma unroll
            for (int d = 0; d < 4; ++d) { w0[d] = acc[d] * inv; w1[d] = acc[d + 4] * inv; }
            reinterpret_cast<f32x4*>(orow)[0] = w0;
            reinterpret_cast<f32x4*>(orow)[1] = w1;
        }
    }
}

struct GreedyArgs {
    const void* logits; int64_t ld; int V;
    int64_t* ids; int64_t ld_ids; int pos;
    int* unfinished; int* counter;
    int eos, pad, min_length, ngram;
};

#define GP_THREADS 512
#define GP_MAX_V 65536
#define GP_U 4

__device__ __forceinline__ void better(float& v, int& i, float v2, int i2) {
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

// One workgroup per row.  The banned tokens of the row (eos below min_length, the continuations of every earlier occurrence of the
// last n - 1 tokens) are set in an LDS bitmap before the scan; the scan reads the row once, 16 bytes per lane per load, GP_U loads
// in flight per lane, and skips banned columns with one LDS word per 8 columns.
template <typename IO>
__global__ __launch_bounds__(GP_THREADS) void greedy_pick_kernel(GreedyArgs a) {
    __shared__ uint32_t ban[GP_MAX_V / 32];
    __shared__ float wv[GP_THREADS / 64];
    __shared__ int wi[GP_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t* ids = a.ids + b * a.ld_ids;
    const int cur_len = a.pos + 1;
    const bool ban_eos = a.eos >= 0 && cur_len < a.min_length;
    const bool ngram = a.ngram > 0 && cur_len + 1 >= a.ngram;
    const bool any_ban = ban_eos || ngram;
    if (any_ban) {
        for (int w = tid; w < (a.V + 31) / 32; w += GP_THREADS) ban[w] = 0u;
        __syncthreads();
        if (ban_eos && tid == 0) atomicOr(&ban[a.eos >> 5], 1u << (a.eos & 31));
        if (ngram) {
            const int nm1 = a.ngram - 1, tail = cur_len - nm1;   // the last n - 1 tokens start at `tail`
            for (int i = tid; i + nm1 < cur_len; i += GP_THREADS) {
                bool match = true;
                for (int t = 0; t < nm1; ++t) match = match && ids[i + t] == ids[tail + t];
                if (match) {
                    const int64_t tok = ids[i + nm1];
                    if (tok >= 0 && tok < a.V) atomicOr(&ban[tok >> 5], 1u << (tok & 31));
                }
            }
        }
        __syncthreads();
    }
    const IO* row = reinterpret_cast<const IO*>(a.logits) + b * a.ld;
    const int groups = (a.V + 7) >> 3;
    float best = -INFINITY;
    int bi = INT_MAX;
    for (int g0 = tid; g0 < groups; g0 += GP_THREADS * GP_U) {
        Raw8<IO> x[GP_U];
#pragma unroll
        for (int u = 0; u < GP_U; ++u) x[u].load(row + 8 * (int64_t)min(g0 + u * GP_THREADS, groups - 1));
#pragma unroll
        for (int u = 0; u < GP_U; ++u) {
            const int g = g0 + u * GP_THREADS;
            if (g >= groups) continue;
            const uint32_t bw = any_ban ? (ban[g >> 2] >> ((g & 3) * 8)) & 0xffu : 0u;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = 8 * g + j;
                const float v = x[u].get(j);
                if (c < a.V && !((bw >> j) & 1u) && v > best) { best = v; bi = c; }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) better(best, bi, __shfl_xor(best, o), __shfl_xor(bi, o));
    if ((tid & 63) == 0) { wv[tid >> 6] = best; wi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        float v = wv[0];
        int i = wi[0];
#pragma unroll
        for (int w = 1; w < GP_THREADS / 64; ++w) better(v, i, wv[w], wi[w]);
        int tok = i == INT_MAX ? 0 : i;                          // (every column banned or -inf: index 0, as torch.argmax)
        int unf = a.unfinished[b];
        if (a.eos >= 0) {
            if (!unf) tok = a.pad;
            else if (tok == a.eos) { unf = 0; a.unfinished[b] = 0; }
        }
        a.ids[b * a.ld_ids + cur_len] = tok;
        atomicAdd(a.counter, unf);
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int herr(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }

}  // namespace

extern "C" int vlpet_attn_decode(const void* q, int64_t ld_q, void* k_cache, void* v_cache, int64_t ld_k, int64_t bs_k,
                                 int64_t ld_v, int64_t bs_v, const void* k_new, const void* v_new, int64_t ld_new, int pos,
                                 const uint8_t* key_mask, int64_t ld_mask, const float* bias, int64_t ld_bias, void* o,
                                 int64_t ld_o, int B, int H, int D, int Lk, float scale, int io_dtype, vlpet_stream_t stream) {
    if (!q || !k_cache || !v_cache || !o) return VLPET_E_NULL;
    if ((k_new == nullptr) != (v_new == nullptr)) return VLPET_E_NULL;
    if (io_dtype != VLPET_F32 && io_dtype != VLPET_BF16) return VLPET_E_DTYPE;
    if (B <= 0 || H <= 0 || (D != 16 && D != 64) || Lk <= 0 || Lk > 1024) return VLPET_E_SHAPE;
    const bool append = k_new != nullptr;
    if (append && (pos < 0 || pos >= Lk)) return VLPET_E_SHAPE;
    const int64_t E = (int64_t)H * D;
    if (ld_q < E || ld_k < E || ld_v < E || ld_o < E || (append && ld_new < E)) return VLPET_E_SHAPE;
    if (bs_k < 0 || bs_v < 0 || (key_mask && ld_mask < Lk) || (bias && ld_bias < Lk)) return VLPET_E_SHAPE;
    if (!al16(q) || !al16(k_cache) || !al16(v_cache) || !al16(o) || (append && (!al16(k_new) || !al16(v_new))))
        return VLPET_E_ALIGN;
    if ((ld_q | ld_k | ld_v | bs_k | bs_v | ld_o | (append ? ld_new : 0)) & 7) return VLPET_E_ALIGN;
    if (bias && (reinterpret_cast<uintptr_t>(bias) & 3)) return VLPET_E_ALIGN;
    DecodeAttnArgs a{};
    a.q = q; a.ld_q = ld_q; a.k = k_cache; a.v = v_cache; a.ld_k = ld_k; a.bs_k = bs_k; a.ld_v = ld_v; a.bs_v = bs_v;
    a.k_new = k_new; a.v_new = v_new; a.ld_new = ld_new; a.pos = pos; a.mask = key_mask; a.ld_mask = ld_mask;
    a.bias = bias; a.ld_bias = ld_bias; a.o = o; a.ld_o = ld_o; a.B = B; a.H = H; a.n_keys = append ? pos + 1 : Lk;
    a.scale = scale;
    const int64_t pairs = (int64_t)B * H;
    dim3 grid((unsigned)((pairs + DEC_WAVES - 1) / DEC_WAVES)), block(DEC_WAVES * 64);
    hipStream_t s = (hipStream_t)stream;
    if (io_dtype == VLPET_BF16) {
        if (D == 64) hipLaunchKernelGGL((attn_decode_kernel<__bf16, 64>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((attn_decode_kernel<__bf16, 16>), grid, block, 0, s, a);
    } else {
        if (D == 64) hipLaunchKernelGGL((attn_decode_kernel<float, 64>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((attn_decode_kernel<float, 16>), grid, block, 0, s, a);
    }
    return herr(hipGetLastError());
}

extern "C" int vlpet_greedy_pick(const void* logits, int64_t ld, int V, int64_t* ids, int64_t ld_ids, int pos, int* unfinished,
                                 int* counter, int B, int eos_token_id, int pad_token_id, int min_length, int no_repeat_ngram_size,
                                 int io_dtype, vlpet_stream_t stream) {
    if (!logits || !ids || !unfinished || !counter) return VLPET_E_NULL;
    if (io_dtype != VLPET_F32 && io_dtype != VLPET_BF16) return VLPET_E_DTYPE;
    if (B <= 0 || V <= 0 || V > GP_MAX_V || ld < (int64_t)((V + 7) / 8 * 8) || pos < 0 || (int64_t)pos + 1 >= ld_ids)
        return VLPET_E_SHAPE;
    if (eos_token_id >= V || no_repeat_ngram_size < 0) return VLPET_E_SHAPE;
    if (!al16(logits) || (ld & 7) || (reinterpret_cast<uintptr_t>(ids) & 7) || (reinterpret_cast<uintptr_t>(unfinished) & 3)
        || (reinterpret_cast<uintptr_t>(counter) & 3))
        return VLPET_E_ALIGN;
    GreedyArgs a{};
    a.logits = logits; a.ld = ld; a.V = V; a.ids = ids; a.ld_ids = ld_ids; a.pos = pos; a.unfinished = unfinished;
    a.counter = counter; a.eos = eos_token_id < 0 ? -1 : eos_token_id; a.pad = pad_token_id; a.min_length = min_length;
    a.ngram = no_repeat_ngram_size;
    hipStream_t s = (hipStream_t)stream;
    if (io_dtype == VLPET_BF16) hipLaunchKernelGGL(greedy_pick_kernel<__bf16>, dim3(B), dim3(GP_THREADS), 0, s, a);
    else hipLaunchKernelGGL(greedy_pick_kernel<float>, dim3(B), dim3(GP_THREADS), 0, s, a);
    return herr(hipGetLastError());
}
