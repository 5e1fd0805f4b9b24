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
//
// Every kernel has a second instantiation (AT = true: the vlpet_*_at entry points) that reads the step position from device memory
// instead of its argument block, so that one captured launch serves every step of a replayed generate().  The position is resolved
// at the top of the kernel (device_pos: one uniform 4-byte read, and a launch whose position lies outside 0..pos_limit-1 writes
// nothing); everything the host derives from an int position -- key count, bias row, ping-pong halves, counter slot, forced step --
// is derived there, and the body below is the same code for both forms.
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

// The step position of an _at launch.  The pointer is a kernel argument and nothing in the launch writes the word, so the read is a
// scalar load; readfirstlane makes the uniformity provable where the compiler cannot see it.  False: outside 0..limit-1.
__device__ __forceinline__ bool device_pos(const int* pos_dev, int limit, int& pos) {
    pos = __builtin_amdgcn_readfirstlane(*pos_dev);
    return pos >= 0 && pos < limit;
}

struct DecodeAttnArgs {
    const void* q; int64_t ld_q;
    void* k; void* v; int64_t ld_k, bs_k, ld_v, bs_v;
    const void* k_new; const void* v_new; int64_t ld_new; int pos;
    const uint8_t* mask; int64_t ld_mask;
    const float* bias; int64_t ld_bias;
    void* o; int64_t ld_o;
    int B, H, n_keys;
    float scale;
    int group;                                  // cross caches / key mask: batch (query row) / group
    const int* key_rows; int64_t ld_kr;         // KR: key j of query row b lives in cache batch key_rows[b, j]
    const int* pos_dev; int pos_limit;          // AT: the position word; bias / key_rows are table bases with these strides
    int64_t ps_bias, ps_kr;                     //     (bias row `pos`, key-row half `pos & 1`)
};

#define DEC_WAVES 4

template <typename IO, int D, bool KR = false, bool AT = false>
__global__ __launch_bounds__(DEC_WAVES * 64) void attn_decode_kernel(DecodeAttnArgs a) {
    int pos = a.pos, n = a.n_keys;
    const float* bias = a.bias;
    const int* key_rows = a.key_rows;
    if constexpr (AT) {                         // (append form only: cache row = pos, keys 0..pos)
        if (!device_pos(a.pos_dev, a.pos_limit, pos)) return;
        n = pos + 1;
        if (bias != nullptr) bias += (int64_t)pos * a.ps_bias;
        if constexpr (KR) key_rows += (int64_t)(pos & 1) * a.ps_kr;
    }
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

    const int64_t cb = KR ? b : b / a.group;    // the cache batch of this query row (KR: of its appended key only)
    IO* kc = reinterpret_cast<IO*>(a.k) + cb * a.bs_k + col;
    IO* vc = reinterpret_cast<IO*>(a.v) + cb * a.bs_v + col;
    const bool append = a.k_new != nullptr;
    Raw8<IO> kn, vn;
    if (append) {
        kn.load(reinterpret_cast<const IO*>(a.k_new) + b * a.ld_new + col);
        vn.load(reinterpret_cast<const IO*>(a.v_new) + b * a.ld_new + col);
        if (kj == 0) {
            kn.store(kc + (int64_t)pos * a.ld_k);
            vn.store(vc + (int64_t)pos * a.ld_v);
        }
    }
    const uint8_t* mrow = a.mask != nullptr ? a.mask + (b / a.group) * a.ld_mask : nullptr;
    const int* krow = KR ? key_rows + b * a.ld_kr : nullptr;
    const float* brow = bias != nullptr ? bias + (int64_t)h * a.ld_bias : nullptr;

    float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[d] = 0.f;

    for (int j0 = 0; j0 < n; j0 += KPS * U) {
        Raw8<IO> kr[U], vr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = min(j0 + u * KPS + kj, n - 1);        // (clamped: a key past the end is loaded but not counted)
            if (append && j == pos) {                          // the appended row comes from registers, not back from memory
                kr[u] = kn;
                vr[u] = vn;
            } else if constexpr (KR) {                           // (a batch outside 0..B-1 reads the row's own)
                const int kb = krow[j];
                const int64_t kbb = (unsigned)kb < (unsigned)a.B ? (int64_t)kb - b : 0;
                kr[u].load(kc + kbb * a.bs_k + (int64_t)j * a.ld_k);
                vr[u].load(vc + kbb * a.bs_v + (int64_t)j * a.ld_v);
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
            bool ok = j < n && (mrow == nullptr || mrow[j] != 0);
            if (ok && brow != nullptr) s += brow[j];
            ok = ok && s != -INFINITY;                           // (a -inf bias entry excludes the key, like the mask:
            if (ok) {                                            //  with m = -inf it would make exp(m - mn) a NaN)
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
    const int* pos_dev; int pos_limit;          // AT: the position word; `counter` is the counters' base (slot `pos`)
    int64_t* next_tokens;                       // AT: [B], the token just written to ids[b, pos + 1]
};

#define GP_THREADS 512
#define GP_MAX_V 65536
#define GP_U 4

__device__ __forceinline__ void better(float& v, int& i, float v2, int i2) {
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

// The banned tokens of one row as an LDS bitmap of V bits (greedy_pick, beam_rows): eos while cur_len < min_length, and the
// continuations of every earlier occurrence of the row's last n - 1 tokens (no_repeat_ngram_size = n).  Returns whether any ban is
// on; the bitmap is only written (and the workgroup synchronised) then.  Every thread of the workgroup calls it.
__device__ __forceinline__ bool build_bans(uint32_t* ban, const int64_t* ids, int cur_len, int V, int eos, int min_length,
                                           int ngram_n, int tid, int nthreads) {
    const bool ban_eos = eos >= 0 && cur_len < min_length;
    const bool ngram = ngram_n > 0 && cur_len + 1 >= ngram_n;
    const bool any_ban = ban_eos || ngram;
    if (any_ban) {
        for (int w = tid; w < (V + 31) / 32; w += nthreads) ban[w] = 0u;
        __syncthreads();
        if (ban_eos && tid == 0) atomicOr(&ban[eos >> 5], 1u << (eos & 31));
        if (ngram) {
            const int nm1 = ngram_n - 1, tail = cur_len - nm1;   // the last n - 1 tokens start at `tail`
            for (int i = tid; i + nm1 < cur_len; i += nthreads) {
                bool match = true;
                for (int t = 0; t < nm1; ++t) match = match && ids[i + t] == ids[tail + t];
                if (match) {
                    const int64_t tok = ids[i + nm1];
                    if (tok >= 0 && tok < V) atomicOr(&ban[tok >> 5], 1u << (tok & 31));
                }
            }
        }
        __syncthreads();
    }
    return any_ban;
}

// One workgroup per row.  The banned tokens of the row (eos below min_length, the continuations of every earlier occurrence of the
// last n - 1 tokens) are set in an LDS bitmap before the scan; the scan reads the row once, 16 bytes per lane per load, GP_U loads
// in flight per lane, and skips banned columns with one LDS word per 8 columns.
template <typename IO, bool AT = false>
__global__ __launch_bounds__(GP_THREADS) void greedy_pick_kernel(GreedyArgs a) {
    __shared__ uint32_t ban[GP_MAX_V / 32];
    __shared__ float wv[GP_THREADS / 64];
    __shared__ int wi[GP_THREADS / 64];
    int pos = a.pos;
    int* counter = a.counter;
    if constexpr (AT) {                         // (before any barrier: the whole workgroup leaves)
        if (!device_pos(a.pos_dev, a.pos_limit, pos)) return;
        counter += pos;
    }
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const bool any_ban = build_bans(ban, a.ids + b * a.ld_ids, pos + 1, a.V, a.eos, a.min_length, a.ngram, tid, GP_THREADS);
    const int cur_len = pos + 1;
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
        if constexpr (AT) a.next_tokens[b] = tok;
        atomicAdd(counter, unf);
    }
}

// ---- beam search (HF 4.2.1 beam_search, num_return_sequences = 1): vlpet_beam_rows + vlpet_beam_advance -------------------------
//
// A row's candidates are (value, index) pairs ordered by value, descending, ties to the lower index: -inf values (banned columns,
// every column but eos on BART's forced step) take part, so they fill a top list exactly when HF's topk would reach them.  A thread
// keeps its best T pairs sorted in registers (an unrolled insertion, run only when a pair beats the T-th); a wave merges its lanes'
// lists in T rounds of a shuffle arg-max in which the winning lane pops its head.

__device__ __forceinline__ bool beats(float v, int i, float v2, int i2) { return v > v2 || (v == v2 && i < i2); }

template <int T> struct TopList {
    float v[T];
    int i[T];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < T; ++j) { v[j] = -INFINITY; i[j] = INT_MAX; }
    }
    __device__ __forceinline__ void insert(float cv, int ci) {
        if (!beats(cv, ci, v[T - 1], i[T - 1])) return;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            if (beats(cv, ci, v[j], i[j])) {
                const float tv = v[j]; const int ti = i[j];
                v[j] = cv; i[j] = ci; cv = tv; ci = ti;
            }
        }
    }
    // the wave's best T over every lane's list: round r's pair lands in (rv, ri) of lane r (lanes >= T: unchanged)
    __device__ __forceinline__ void wave_merge(int lane, float& rv, int& ri) {
#pragma unroll
        for (int r = 0; r < T; ++r) {
            float bv = v[0];
            int bi = i[0];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o);
                const int oi = __shfl_xor(bi, o);
                if (beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if (lane == r) { rv = bv; ri = bi; }
            if (i[0] == bi && v[0] == bv) {                      // the winner pops its head (indices are unique; sentinels alike)
#pragma unroll
                for (int j = 0; j + 1 < T; ++j) { v[j] = v[j + 1]; i[j] = i[j + 1]; }
                v[T - 1] = -INFINITY; i[T - 1] = INT_MAX;
            }
        }
    }
};

struct BeamRowsArgs {
    const void* logits; int64_t ld; int V;
    const int64_t* ids; int64_t ld_ids; int pos;
    int eos, min_length, ngram, force_eos;
    int slices, slice_cols;
    float* stats; float* val; int* tok;         // per (row, slice): (max, sum of exp(x - max)); the top T (value, token)
    const int* pos_dev; int pos_limit;          // AT: the position word; `ids` is the ping-pong base (half `pos & 1`, stride ps_ids),
    int64_t ps_ids; int force_eos_pos;          //     the forced step is the one at force_eos_pos (-1: never)
};

#define BR_THREADS 256

// grid (slices, rows).  The slice's columns are read once, 16 bytes per lane per load, GP_U loads in flight per lane.
template <typename IO, int T, bool AT = false>
__global__ __launch_bounds__(BR_THREADS) void beam_rows_kernel(BeamRowsArgs a) {
    int pos = a.pos;
    const int64_t* ids = a.ids;
    bool force_eos = a.force_eos != 0;
    if constexpr (AT) {                         // (before any barrier: the whole workgroup leaves)
        if (!device_pos(a.pos_dev, a.pos_limit, pos)) return;
        ids += (int64_t)(pos & 1) * a.ps_ids;
        force_eos = pos == a.force_eos_pos;
    }
    __shared__ uint32_t ban[GP_MAX_V / 32];
    __shared__ float wm[BR_THREADS / 64], ws[BR_THREADS / 64];
    __shared__ float lv[BR_THREADS / 64][T];
    __shared__ int li[BR_THREADS / 64][T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x;
    const int64_t r = blockIdx.y;
    const bool any_ban = build_bans(ban, ids + r * a.ld_ids, pos + 1, a.V, a.eos, a.min_length, a.ngram, tid, BR_THREADS);
    const IO* row = reinterpret_cast<const IO*>(a.logits) + r * a.ld;
    const int c0 = s * a.slice_cols, c1 = min(a.V, c0 + a.slice_cols);
    const int g_lo = c0 >> 3, g_hi = (c1 + 7) >> 3;             // (slice_cols is a multiple of 8)
    float m = -INFINITY, sum = 0.f;
    TopList<T> top;
    top.clear();
    for (int g0 = g_lo + tid; g0 < g_hi; g0 += BR_THREADS * GP_U) {
        Raw8<IO> x[GP_U];
#pragma unroll
        for (int u = 0; u < GP_U; ++u) x[u].load(row + 8 * (int64_t)min(g0 + u * BR_THREADS, g_hi - 1));
#pragma unroll
        for (int u = 0; u < GP_U; ++u) {
            const int g = g0 + u * BR_THREADS;
            if (g >= g_hi) continue;
            const uint32_t bw = any_ban ? (ban[g >> 2] >> ((g & 3) * 8)) & 0xffu : 0u;
            float xv[8], mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = 8 * g + j;
                const bool in = c < c1 && (!force_eos || c == a.eos);
                xv[j] = in ? x[u].get(j) : -INFINITY;
                mx = fmaxf(mx, xv[j]);
            }
            if (mx > m) { sum = m == -INFINITY ? 0.f : sum * __expf(m - mx); m = mx; }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = 8 * g + j;
                if (xv[j] != -INFINITY) sum += __expf(xv[j] - m);
                if (c < c1) top.insert((bw >> j) & 1u ? -INFINITY : xv[j], c);
            }
        }
    }
    // (max, sum) over the workgroup
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float mo = __shfl_xor(m, o), so = __shfl_xor(sum, o);
        const float M = fmaxf(m, mo);
        sum = (m == -INFINITY ? 0.f : sum * __expf(m - M)) + (mo == -INFINITY ? 0.f : so * __expf(mo - M));
        m = M;
    }
    float rv = -INFINITY;
    int ri = INT_MAX;
    top.wave_merge(lane, rv, ri);
    if (lane == 0) { wm[wave] = m; ws[wave] = sum; }
    if (lane < T) { lv[wave][lane] = rv; li[wave][lane] = ri; }
    __syncthreads();
    if (wave != 0) return;
    TopList<T> w;
    w.clear();
    if (lane < BR_THREADS / 64) {
#pragma unroll
        for (int j = 0; j < T; ++j) { w.v[j] = lv[lane][j]; w.i[j] = li[lane][j]; }
    }
    w.wave_merge(lane, rv, ri);
    const int64_t slot = r * a.slices + s;
    if (lane < T) { a.val[slot * T + lane] = rv; a.tok[slot * T + lane] = ri; }
    if (lane == 0) {
        float M = wm[0], S = ws[0];
#pragma unroll
        for (int q = 1; q < BR_THREADS / 64; ++q) {
            const float M2 = fmaxf(M, wm[q]);
            S = (M == -INFINITY ? 0.f : S * __expf(M - M2)) + (wm[q] == -INFINITY ? 0.f : ws[q] * __expf(wm[q] - M2));
            M = M2;
        }
        a.stats[2 * slot] = M;
        a.stats[2 * slot + 1] = S;
    }
}

struct BeamAdvanceArgs {
    const float* stats; const float* val; const int* tok; int slices; int V; int B;
    float* beam_scores;
    const int64_t* ids_in; int64_t* ids_out; int64_t ld_ids;
    const int* kr_in; int* kr_out; int64_t ld_kr;
    int64_t* next_tokens;
    float* hyp_score; int* hyp_meta; int64_t* hyp_tokens; int64_t ld_hyp;
    float* worst; int* state; int* counter;
    int pos, eos, pad;
    float length_penalty; int early;
    const int* pos_dev; int pos_limit;          // AT: the position word; ids_in / kr_in are the ping-pong bases (read half `pos & 1`,
    int64_t ps_ids, ps_kr;                      //     written half the other one), `counter` the counters' base (slot `pos`)
};

// One wave (= one workgroup) per item.  Every lane runs the scorer's walk on the same values (held in registers alike), so no lane
// waits on another's memory writes; the copies (ids, key rows, a new hypothesis' tokens) are spread over the lanes.
template <int K, bool AT = false>
__global__ __launch_bounds__(64) void beam_advance_kernel(BeamAdvanceArgs a) {
    constexpr int T = 2 * K;
    if constexpr (AT) {                         // resolved into the argument block's own copy: the body reads `a` as in the int form
        int pos;
        if (!device_pos(a.pos_dev, a.pos_limit, pos)) return;
        const int64_t src = pos & 1, dst = src ^ 1;
        int64_t* ids = a.ids_out;               // (the base of both halves)
        a.pos = pos;
        a.ids_in = ids + src * a.ps_ids;
        a.ids_out = ids + dst * a.ps_ids;
        if (a.kr_in) {
            int* kr = a.kr_out;
            a.kr_in = kr + src * a.ps_kr;
            a.kr_out = kr + dst * a.ps_kr;
        }
        a.counter += pos;
    }
    __shared__ float s_lse[K], s_bs[K];
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    const int cur_len = a.pos + 1;
    const int64_t r0 = (int64_t)b * K;
    int* st = a.state + 3 * b;                     // count, insertions so far, done
    const int done0 = st[2];
    if (done0) {                                   // a done item's rows: carried over unchanged, pad appended
        for (int k = 0; k < K; ++k) {
            const int64_t r = r0 + k;
            for (int t = lane; t < cur_len; t += 64) {
                a.ids_out[r * a.ld_ids + t] = a.ids_in[r * a.ld_ids + t];
                if (a.kr_in) a.kr_out[r * a.ld_kr + t] = a.kr_in[r * a.ld_kr + t];
            }
            if (lane == 0) {
                a.ids_out[r * a.ld_ids + cur_len] = a.pad;
                if (a.kr_in) a.kr_out[r * a.ld_kr + cur_len] = (int)r;
                a.next_tokens[r] = a.pad;
            }
        }
        return;
    }
    if (lane < K) {                                // the row's log-sum-exp over its slices
        const int64_t r = r0 + lane;
        float M = -INFINITY, S = 0.f;
        for (int s = 0; s < a.slices; ++s) {
            const float m2 = a.stats[2 * (r * a.slices + s)], s2 = a.stats[2 * (r * a.slices + s) + 1];
            const float Mn = fmaxf(M, m2);
            S = (M == -INFINITY ? 0.f : S * __expf(M - Mn)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - Mn));
            M = Mn;
        }
        s_lse[lane] = M + logf(S);
        s_bs[lane] = a.beam_scores[r];
    }
    __syncthreads();
    TopList<T> top;
    top.clear();
    const int n = K * a.slices * T;
    for (int q = lane; q < n; q += 64) {           // q = (k * slices + s) * T + j: row r0 + k's slice s, rank j
        const int k = q / (a.slices * T);
        const int t = a.tok[r0 * a.slices * T + q];
        if (t == INT_MAX) continue;
        const float v = a.val[r0 * a.slices * T + q];
        top.insert((v - s_lse[k]) + s_bs[k], k * a.V + t);
    }
    float cv = -INFINITY;
    int ci = INT_MAX;
    top.wave_merge(lane, cv, ci);

    // the hypothesis table of the item, alike in every lane
    float hs[K];
    int ho[K];
    int cnt = st[0], nadd = st[1];
    float worst = a.worst[b];
#pragma unroll
    for (int j = 0; j < K; ++j) { hs[j] = a.hyp_score[r0 + j]; ho[j] = a.hyp_meta[2 * (r0 + j) + 1]; }
    const float lpow = powf((float)cur_len, a.length_penalty);
    int slot = 0;
    float my_s = 0.f;
    int my_tok = a.pad, my_src = (int)r0;
    for (int rank = 0; rank < T && slot < K; ++rank) {
        const float sc = __shfl(cv, rank);
        const int flat = __shfl(ci, rank);
        if (flat == INT_MAX) continue;
        const int beam = flat / a.V, tk = flat - beam * a.V;
        const int src = (int)r0 + beam;
        if (tk == a.eos) {
            if (rank >= K) continue;
            const float h = sc / lpow;
            if (cnt < K || h > worst) {
                int at = 0;
                const bool evict = cnt == K;
                if (!evict) {
                    at = cnt++;
                    worst = fminf(h, worst);
                } else {                               // replaces the lowest (score, insertion): HF drops it after appending
#pragma unroll
                    for (int j = 1; j < K; ++j)
                        if (hs[j] < hs[at] || (hs[j] == hs[at] && ho[j] < ho[at])) at = j;
                }
#pragma unroll
                for (int j = 0; j < K; ++j)
                    if (j == at) { hs[j] = h; ho[j] = nadd; }
                if (lane == 0) { a.hyp_score[r0 + at] = h; a.hyp_meta[2 * (r0 + at)] = cur_len; a.hyp_meta[2 * (r0 + at) + 1] = nadd; }
                ++nadd;
                if (evict) {                           // the new worst: the lowest of the K kept
                    worst = hs[0];
#pragma unroll
                    for (int j = 1; j < K; ++j) worst = fminf(worst, hs[j]);
                }
                for (int t = lane; t < cur_len; t += 64)
                    a.hyp_tokens[(r0 + at) * a.ld_hyp + t] = a.ids_in[(int64_t)src * a.ld_ids + t];
            }
        } else {
            if (lane == slot) { my_s = sc; my_tok = tk; my_src = src; }
            ++slot;
        }
    }
    const float best = __shfl(cv, 0);
    const bool done = cnt >= K && (a.early || worst >= best / lpow);
    // the next rows: beam scores, tokens, ids and key rows reordered by source row, the token appended
    if (lane < K) {
        a.beam_scores[r0 + lane] = my_s;
        a.next_tokens[r0 + lane] = my_tok;
    }
    for (int k = 0; k < K; ++k) {
        const int64_t r = r0 + k;
        const int64_t src = __shfl(my_src, k);
        const int64_t tk = __shfl(my_tok, k);
        for (int t = lane; t < cur_len; t += 64) {
            a.ids_out[r * a.ld_ids + t] = a.ids_in[src * a.ld_ids + t];
            if (a.kr_in) a.kr_out[r * a.ld_kr + t] = a.kr_in[src * a.ld_kr + t];
        }
        if (lane == 0) {
            a.ids_out[r * a.ld_ids + cur_len] = tk;
            if (a.kr_in) a.kr_out[r * a.ld_kr + cur_len] = (int)r;
        }
    }
    if (lane == 0) {
        st[0] = cnt; st[1] = nadd; st[2] = done ? 1 : 0;
        a.worst[b] = worst;
        if (!done) atomicAdd(a.counter, 1);
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int herr(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }

inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// An _at entry point's position arguments: no position word or a limit outside 1..capacity (of what `pos` indexes) -> -1.
inline int check_pos_dev(const int* pos_dev, int pos_limit, int64_t capacity) {
    if (!pos_dev) return VLPET_E_SHAPE;
    if (!al4(pos_dev)) return VLPET_E_ALIGN;
    if (pos_limit < 1 || pos_limit > capacity) return VLPET_E_SHAPE;
    return 0;
}

// Checks + launch of the four entry points' two forms.  `at`: the position-dependent checks of the int form run at pos_limit - 1,
// the largest position the kernel's guard lets through, and the launch takes the AT instantiation.

int attn_decode_run(const void* q, int64_t ld_q, void* k_cache, void* v_cache, int64_t ld_k, int64_t bs_k, int64_t ld_v,
                    int64_t bs_v, const void* k_new, const void* v_new, int64_t ld_new, int pos, const uint8_t* key_mask,
                    int64_t ld_mask, const float* bias, int64_t ld_bias, void* o, int64_t ld_o, int B, int H, int D, int Lk,
                    float scale, int group, const int* key_rows, int64_t ld_key_rows, int io_dtype, vlpet_stream_t stream, bool at,
                    const int* pos_dev, int pos_limit, int64_t ps_bias, int64_t ps_kr) {
    if (!q || !k_cache || !v_cache || !o) return VLPET_E_NULL;
    if ((k_new == nullptr) != (v_new == nullptr)) return VLPET_E_NULL;
    if (at && !k_new) return VLPET_E_NULL;                        // (the _at form is the append form)
    if (io_dtype != VLPET_F32 && io_dtype != VLPET_BF16) return VLPET_E_DTYPE;
    if (B <= 0 || H <= 0 || (D != 16 && D != 64) || Lk <= 0 || Lk > 1024 || group <= 0) return VLPET_E_SHAPE;
    int keys = Lk;                                                // what a mask / bias / key-row row must cover
    if (at) {
        const int e = check_pos_dev(pos_dev, pos_limit, Lk);
        if (e) return e;
        if (ps_bias < 0 || ps_kr < 0) return VLPET_E_SHAPE;
        pos = pos_limit - 1;
        keys = pos_limit;
    }
    const bool append = k_new != nullptr;
    if (append && (pos < 0 || pos >= Lk)) return VLPET_E_SHAPE;
    if (append && group != 1) return VLPET_E_SHAPE;               // the appended row goes to batch r: one cache batch per row
    if (key_rows && ld_key_rows < (append ? pos + 1 : Lk)) return VLPET_E_SHAPE;
    const int64_t E = (int64_t)H * D;
    if (ld_q < E || ld_k < E || ld_v < E || ld_o < E || (append && ld_new < E)) return VLPET_E_SHAPE;
    if (bs_k < 0 || bs_v < 0 || (key_mask && ld_mask < keys) || (bias && ld_bias < keys)) return VLPET_E_SHAPE;
    if (!al16(q) || !al16(k_cache) || !al16(v_cache) || !al16(o) || (append && (!al16(k_new) || !al16(v_new))))
        return VLPET_E_ALIGN;
    if ((ld_q | ld_k | ld_v | bs_k | bs_v | ld_o | (append ? ld_new : 0)) & 7) return VLPET_E_ALIGN;
    if ((bias && !al4(bias)) || (key_rows && !al4(key_rows))) return VLPET_E_ALIGN;
    DecodeAttnArgs a{};
    a.q = q; a.ld_q = ld_q; a.k = k_cache; a.v = v_cache; a.ld_k = ld_k; a.bs_k = bs_k; a.ld_v = ld_v; a.bs_v = bs_v;
    a.k_new = k_new; a.v_new = v_new; a.ld_new = ld_new; a.pos = pos; a.mask = key_mask; a.ld_mask = ld_mask;
    a.bias = bias; a.ld_bias = ld_bias; a.o = o; a.ld_o = ld_o; a.B = B; a.H = H; a.n_keys = append ? pos + 1 : Lk;
    a.scale = scale; a.group = group; a.key_rows = key_rows; a.ld_kr = ld_key_rows;
    a.pos_dev = pos_dev; a.pos_limit = pos_limit; a.ps_bias = ps_bias; a.ps_kr = ps_kr;
    const int64_t pairs = (int64_t)B * H;
    dim3 grid((unsigned)((pairs + DEC_WAVES - 1) / DEC_WAVES)), block(DEC_WAVES * 64);
    hipStream_t s = (hipStream_t)stream;
#define DEC_LAUNCH_KR(IO, DD, KR)                                                                                                  \
    do {                                                                                                                           \
        if (at) hipLaunchKernelGGL((attn_decode_kernel<IO, DD, KR, true>), grid, block, 0, s, a);                                 \
        else hipLaunchKernelGGL((attn_decode_kernel<IO, DD, KR, false>), grid, block, 0, s, a);                                   \
    } while (0)
#define DEC_LAUNCH(IO, DD)                                                                                                         \
    do {                                                                                                                           \
        if (key_rows) DEC_LAUNCH_KR(IO, DD, true);                                                                                 \
        else DEC_LAUNCH_KR(IO, DD, false);                                                                                         \
    } while (0)
    if (io_dtype == VLPET_BF16) {
        if (D == 64) DEC_LAUNCH(__bf16, 64);
        else DEC_LAUNCH(__bf16, 16);
    } else {
        if (D == 64) DEC_LAUNCH(float, 64);
        else DEC_LAUNCH(float, 16);
    }
#undef DEC_LAUNCH
#undef DEC_LAUNCH_KR
    return herr(hipGetLastError());
}

int greedy_pick_run(const void* logits, int64_t ld, int V, int64_t* ids, int64_t ld_ids, int pos, int* unfinished, int* counter,
                    int B, int eos_token_id, int pad_token_id, int min_length, int no_repeat_ngram_size, int io_dtype,
                    vlpet_stream_t stream, bool at, const int* pos_dev, int pos_limit, int64_t* next_tokens) {
    if (!logits || !ids || !unfinished || !counter || (at && !next_tokens)) return VLPET_E_NULL;
    if (io_dtype != VLPET_F32 && io_dtype != VLPET_BF16) return VLPET_E_DTYPE;
    if (at) {
        const int e = check_pos_dev(pos_dev, pos_limit, INT_MAX);
        if (e) return e;
        pos = pos_limit - 1;
    }
    if (B <= 0 || V <= 0 || V > GP_MAX_V || ld < (int64_t)((V + 7) / 8 * 8) || pos < 0 || (int64_t)pos + 1 >= ld_ids)
        return VLPET_E_SHAPE;
    if (eos_token_id >= V || no_repeat_ngram_size < 0) return VLPET_E_SHAPE;
    if (!al16(logits) || (ld & 7) || (reinterpret_cast<uintptr_t>(ids) & 7) || !al4(unfinished) || !al4(counter)
        || (reinterpret_cast<uintptr_t>(next_tokens) & 7))
        return VLPET_E_ALIGN;
    GreedyArgs a{};
    a.logits = logits; a.ld = ld; a.V = V; a.ids = ids; a.ld_ids = ld_ids; a.pos = pos; a.unfinished = unfinished;
    a.counter = counter; a.eos = eos_token_id < 0 ? -1 : eos_token_id; a.pad = pad_token_id; a.min_length = min_length;
    a.ngram = no_repeat_ngram_size; a.pos_dev = pos_dev; a.pos_limit = pos_limit; a.next_tokens = next_tokens;
    hipStream_t s = (hipStream_t)stream;
#define GP_LAUNCH(IO)                                                                                                              \
    do {                                                                                                                           \
        if (at) hipLaunchKernelGGL((greedy_pick_kernel<IO, true>), dim3(B), dim3(GP_THREADS), 0, s, a);                           \
        else hipLaunchKernelGGL((greedy_pick_kernel<IO, false>), dim3(B), dim3(GP_THREADS), 0, s, a);                             \
    } while (0)
    if (io_dtype == VLPET_BF16) GP_LAUNCH(__bf16);
    else GP_LAUNCH(float);
#undef GP_LAUNCH
    return herr(hipGetLastError());
}

int beam_rows_run(const void* logits, int64_t ld, int V, const int64_t* ids, int64_t ld_ids, int pos, int rows, int num_beams,
                  int slices, int eos_token_id, int min_length, int no_repeat_ngram_size, int force_eos, float* part_stats,
                  float* part_val, int* part_tok, int io_dtype, vlpet_stream_t stream, bool at, const int* pos_dev, int pos_limit,
                  int64_t ps_ids, int force_eos_pos) {
    if (!logits || !ids || !part_stats || !part_val || !part_tok) return VLPET_E_NULL;
    if (io_dtype != VLPET_F32 && io_dtype != VLPET_BF16) return VLPET_E_DTYPE;
    if (at) {
        const int e = check_pos_dev(pos_dev, pos_limit, INT_MAX);
        if (e) return e;
        if (ps_ids < 0) return VLPET_E_SHAPE;
        pos = pos_limit - 1;
    }
    if (rows <= 0 || V <= 0 || V > GP_MAX_V || ld < (int64_t)((V + 7) / 8 * 8) || pos < 0 || (int64_t)pos + 1 > ld_ids)
        return VLPET_E_SHAPE;
    if (num_beams < 2 || num_beams > 8 || slices < 1 || slices > 64 || rows > 65535) return VLPET_E_SHAPE;
    if (eos_token_id < 0 || eos_token_id >= V || no_repeat_ngram_size < 0) return VLPET_E_SHAPE;
    if (!al16(logits) || (ld & 7) || (reinterpret_cast<uintptr_t>(ids) & 7) || (reinterpret_cast<uintptr_t>(part_stats) & 7)
        || !al4(part_val) || !al4(part_tok))
        return VLPET_E_ALIGN;
    BeamRowsArgs a{};
    a.logits = logits; a.ld = ld; a.V = V; a.ids = ids; a.ld_ids = ld_ids; a.pos = pos; a.eos = eos_token_id;
    a.min_length = min_length; a.ngram = no_repeat_ngram_size; a.force_eos = force_eos ? 1 : 0;
    a.slices = slices; a.slice_cols = ((V + slices - 1) / slices + 7) / 8 * 8;
    a.stats = part_stats; a.val = part_val; a.tok = part_tok;
    a.pos_dev = pos_dev; a.pos_limit = pos_limit; a.ps_ids = ps_ids; a.force_eos_pos = force_eos_pos;
    dim3 grid(slices, rows), block(BR_THREADS);
    hipStream_t s = (hipStream_t)stream;
#define BR_LAUNCH_AT(IO, KK)                                                                                                       \
    do {                                                                                                                           \
        if (at) hipLaunchKernelGGL((beam_rows_kernel<IO, 2 * KK, true>), grid, block, 0, s, a);                                   \
        else hipLaunchKernelGGL((beam_rows_kernel<IO, 2 * KK, false>), grid, block, 0, s, a);                                     \
    } while (0)
#define BR_LAUNCH(KK)                                                                                                              \
    case KK:                                                                                                                       \
        if (io_dtype == VLPET_BF16) BR_LAUNCH_AT(__bf16, KK);                                                                      \
        else BR_LAUNCH_AT(float, KK);                                                                                              \
        break;
    switch (num_beams) { BR_LAUNCH(2) BR_LAUNCH(3) BR_LAUNCH(4) BR_LAUNCH(5) BR_LAUNCH(6) BR_LAUNCH(7) BR_LAUNCH(8) }
#undef BR_LAUNCH
#undef BR_LAUNCH_AT
    return herr(hipGetLastError());
}

int beam_advance_run(const float* part_stats, const float* part_val, const int* part_tok, int slices, int V, int B, int num_beams,
                     float* beam_scores, const int64_t* ids_in, int64_t* ids_out, int64_t ld_ids, const int* key_rows_in,
                     int* key_rows_out, int64_t ld_key_rows, int64_t* next_tokens, float* hyp_score, int* hyp_meta,
                     int64_t* hyp_tokens, int64_t ld_hyp, float* item_worst, int* item_state, int* counter, int pos,
                     int eos_token_id, int pad_token_id, float length_penalty, int early_stopping, vlpet_stream_t stream, bool at,
                     const int* pos_dev, int pos_limit, int64_t ps_ids, int64_t ps_kr) {
    if (!part_stats || !part_val || !part_tok || !beam_scores || !ids_in || !ids_out || !next_tokens || !hyp_score || !hyp_meta
        || !hyp_tokens || !item_worst || !item_state || !counter)
        return VLPET_E_NULL;
    if ((key_rows_in == nullptr) != (key_rows_out == nullptr)) return VLPET_E_NULL;
    if (at) {
        const int e = check_pos_dev(pos_dev, pos_limit, INT_MAX);
        if (e) return e;
        if (ps_ids < 0 || ps_kr < 0) return VLPET_E_SHAPE;
        pos = pos_limit - 1;
    }
    if (B <= 0 || V <= 0 || V > GP_MAX_V || num_beams < 2 || num_beams > 8 || slices < 1 || slices > 64) return VLPET_E_SHAPE;
    if (pos < 0 || (int64_t)pos + 1 >= ld_ids || (int64_t)pos + 1 > ld_hyp || (key_rows_in && (int64_t)pos + 1 >= ld_key_rows))
        return VLPET_E_SHAPE;
    if (eos_token_id < 0 || eos_token_id >= V) return VLPET_E_SHAPE;
    const uintptr_t w8 = reinterpret_cast<uintptr_t>(ids_in) | reinterpret_cast<uintptr_t>(ids_out)
                         | reinterpret_cast<uintptr_t>(next_tokens) | reinterpret_cast<uintptr_t>(hyp_tokens);
    const uintptr_t w4 = reinterpret_cast<uintptr_t>(part_stats) | reinterpret_cast<uintptr_t>(part_val)
                         | reinterpret_cast<uintptr_t>(part_tok) | reinterpret_cast<uintptr_t>(beam_scores)
                         | reinterpret_cast<uintptr_t>(hyp_score) | reinterpret_cast<uintptr_t>(hyp_meta)
                         | reinterpret_cast<uintptr_t>(item_worst) | reinterpret_cast<uintptr_t>(item_state)
                         | reinterpret_cast<uintptr_t>(counter) | reinterpret_cast<uintptr_t>(key_rows_in)
                         | reinterpret_cast<uintptr_t>(key_rows_out);
    if ((w8 & 7) || (w4 & 3)) return VLPET_E_ALIGN;
    BeamAdvanceArgs a{};
    a.stats = part_stats; a.val = part_val; a.tok = part_tok; a.slices = slices; a.V = V; a.B = B; a.beam_scores = beam_scores;
    a.ids_in = ids_in; a.ids_out = ids_out; a.ld_ids = ld_ids; a.kr_in = key_rows_in; a.kr_out = key_rows_out;
    a.ld_kr = ld_key_rows; a.next_tokens = next_tokens; a.hyp_score = hyp_score; a.hyp_meta = hyp_meta;
    a.hyp_tokens = hyp_tokens; a.ld_hyp = ld_hyp; a.worst = item_worst; a.state = item_state; a.counter = counter; a.pos = pos;
    a.eos = eos_token_id; a.pad = pad_token_id; a.length_penalty = length_penalty; a.early = early_stopping ? 1 : 0;
    a.pos_dev = pos_dev; a.pos_limit = pos_limit; a.ps_ids = ps_ids; a.ps_kr = ps_kr;
    hipStream_t s = (hipStream_t)stream;
#define BA_LAUNCH(KK)                                                                                                              \
    case KK:                                                                                                                       \
        if (at) hipLaunchKernelGGL((beam_advance_kernel<KK, true>), dim3(B), dim3(64), 0, s, a);                                  \
        else hipLaunchKernelGGL((beam_advance_kernel<KK, false>), dim3(B), dim3(64), 0, s, a);                                    \
        break;
    switch (num_beams) { BA_LAUNCH(2) BA_LAUNCH(3) BA_LAUNCH(4) BA_LAUNCH(5) BA_LAUNCH(6) BA_LAUNCH(7) BA_LAUNCH(8) }
#undef BA_LAUNCH
    return herr(hipGetLastError());
}

}  // namespace

extern "C" int vlpet_attn_decode(const void* q, int64_t ld_q, void* k_cache, void* v_cache, int64_t ld_k, int64_t bs_k,
                                 int64_t ld_v, int64_t bs_v, const void* k_new, const void* v_new, int64_t ld_new, int pos,
                                 const uint8_t* key_mask, int64_t ld_mask, const float* bias, int64_t ld_bias, void* o,
                                 int64_t ld_o, int B, int H, int D, int Lk, float scale, int io_dtype, vlpet_stream_t stream) {
    return attn_decode_run(q, ld_q, k_cache, v_cache, ld_k, bs_k, ld_v, bs_v, k_new, v_new, ld_new, pos, key_mask, ld_mask, bias,
                           ld_bias, o, ld_o, B, H, D, Lk, scale, 1, nullptr, 0, io_dtype, stream, false, nullptr, 0, 0, 0);
}

extern "C" int vlpet_attn_decode_beam(const void* q, int64_t ld_q, void* k_cache, void* v_cache, int64_t ld_k, int64_t bs_k,
                                      int64_t ld_v, int64_t bs_v, const void* k_new, const void* v_new, int64_t ld_new, int pos,
                                      const uint8_t* key_mask, int64_t ld_mask, const float* bias, int64_t ld_bias, void* o,
                                      int64_t ld_o, int B, int H, int D, int Lk, float scale, int group, const int* key_rows,
                                      int64_t ld_key_rows, int io_dtype, vlpet_stream_t stream) {
    return attn_decode_run(q, ld_q, k_cache, v_cache, ld_k, bs_k, ld_v, bs_v, k_new, v_new, ld_new, pos, key_mask, ld_mask, bias,
                           ld_bias, o, ld_o, B, H, D, Lk, scale, group, key_rows, ld_key_rows, io_dtype, stream, false, nullptr, 0,
                           0, 0);
}

extern "C" int vlpet_attn_decode_at(const void* q, int64_t ld_q, void* k_cache, void* v_cache, int64_t ld_k, int64_t bs_k,
                                    int64_t ld_v, int64_t bs_v, const void* k_new, const void* v_new, int64_t ld_new,
                                    const int* pos_dev, int pos_limit, const uint8_t* key_mask, int64_t ld_mask, const float* bias,
                                    int64_t ld_bias, int64_t pos_stride_bias, void* o, int64_t ld_o, int B, int H, int D, int Lk,
                                    float scale, const int* key_rows, int64_t ld_key_rows, int64_t parity_stride_key_rows,
                                    int io_dtype, vlpet_stream_t stream) {
    return attn_decode_run(q, ld_q, k_cache, v_cache, ld_k, bs_k, ld_v, bs_v, k_new, v_new, ld_new, 0, key_mask, ld_mask, bias,
                           ld_bias, o, ld_o, B, H, D, Lk, scale, 1, key_rows, ld_key_rows, io_dtype, stream, true, pos_dev,
                           pos_limit, pos_stride_bias, parity_stride_key_rows);
}

extern "C" int vlpet_greedy_pick(const void* logits, int64_t ld, int V, int64_t* ids, int64_t ld_ids, int pos, int* unfinished,
                                 int* counter, int B, int eos_token_id, int pad_token_id, int min_length, int no_repeat_ngram_size,
                                 int io_dtype, vlpet_stream_t stream) {
    return greedy_pick_run(logits, ld, V, ids, ld_ids, pos, unfinished, counter, B, eos_token_id, pad_token_id, min_length,
                           no_repeat_ngram_size, io_dtype, stream, false, nullptr, 0, nullptr);
}

extern "C" int vlpet_greedy_pick_at(const void* logits, int64_t ld, int V, int64_t* ids, int64_t ld_ids, const int* pos_dev,
                                    int pos_limit, int* unfinished, int* counters, int64_t* next_tokens, int B, int eos_token_id,
                                    int pad_token_id, int min_length, int no_repeat_ngram_size, int io_dtype,
                                    vlpet_stream_t stream) {
    return greedy_pick_run(logits, ld, V, ids, ld_ids, 0, unfinished, counters, B, eos_token_id, pad_token_id, min_length,
                           no_repeat_ngram_size, io_dtype, stream, true, pos_dev, pos_limit, next_tokens);
}

extern "C" int vlpet_beam_rows(const void* logits, int64_t ld, int V, const int64_t* ids, int64_t ld_ids, int pos, int rows,
                               int num_beams, int slices, int eos_token_id, int min_length, int no_repeat_ngram_size, int force_eos,
                               float* part_stats, float* part_val, int* part_tok, int io_dtype, vlpet_stream_t stream) {
    return beam_rows_run(logits, ld, V, ids, ld_ids, pos, rows, num_beams, slices, eos_token_id, min_length, no_repeat_ngram_size,
                         force_eos, part_stats, part_val, part_tok, io_dtype, stream, false, nullptr, 0, 0, -1);
}

extern "C" int vlpet_beam_rows_at(const void* logits, int64_t ld, int V, const int64_t* ids, int64_t ld_ids,
                                  int64_t parity_stride_ids, const int* pos_dev, int pos_limit, int rows, int num_beams, int slices,
                                  int eos_token_id, int min_length, int no_repeat_ngram_size, int force_eos_pos, float* part_stats,
                                  float* part_val, int* part_tok, int io_dtype, vlpet_stream_t stream) {
    return beam_rows_run(logits, ld, V, ids, ld_ids, 0, rows, num_beams, slices, eos_token_id, min_length, no_repeat_ngram_size, 0,
                         part_stats, part_val, part_tok, io_dtype, stream, true, pos_dev, pos_limit, parity_stride_ids,
                         force_eos_pos);
}

extern "C" int vlpet_beam_advance(const float* part_stats, const float* part_val, const int* part_tok, int slices, int V, int B,
                                  int num_beams, float* beam_scores, const int64_t* ids_in, int64_t* ids_out, int64_t ld_ids,
                                  const int* key_rows_in, int* key_rows_out, int64_t ld_key_rows, int64_t* next_tokens,
                                  float* hyp_score, int* hyp_meta, int64_t* hyp_tokens, int64_t ld_hyp, float* item_worst,
                                  int* item_state, int* counter, int pos, int eos_token_id, int pad_token_id, float length_penalty,
                                  int early_stopping, vlpet_stream_t stream) {
    return beam_advance_run(part_stats, part_val, part_tok, slices, V, B, num_beams, beam_scores, ids_in, ids_out, ld_ids,
                            key_rows_in, key_rows_out, ld_key_rows, next_tokens, hyp_score, hyp_meta, hyp_tokens, ld_hyp,
                            item_worst, item_state, counter, pos, eos_token_id, pad_token_id, length_penalty, early_stopping,
                            stream, false, nullptr, 0, 0, 0);
}

extern "C" int vlpet_beam_advance_at(const float* part_stats, const float* part_val, const int* part_tok, int slices, int V, int B,
                                     int num_beams, float* beam_scores, int64_t* ids, int64_t ld_ids, int64_t parity_stride_ids,
                                     int* key_rows, int64_t ld_key_rows, int64_t parity_stride_key_rows, int64_t* next_tokens,
                                     float* hyp_score, int* hyp_meta, int64_t* hyp_tokens, int64_t ld_hyp, float* item_worst,
                                     int* item_state, int* counters, const int* pos_dev, int pos_limit, int eos_token_id,
                                     int pad_token_id, float length_penalty, int early_stopping, vlpet_stream_t stream) {
    return beam_advance_run(part_stats, part_val, part_tok, slices, V, B, num_beams, beam_scores, ids, ids, ld_ids, key_rows,
                            key_rows, ld_key_rows, next_tokens, hyp_score, hyp_meta, hyp_tokens, ld_hyp, item_worst, item_state,
                            counters, 0, eos_token_id, pad_token_id, length_penalty, early_stopping, stream, true, pos_dev,
                            pos_limit, parity_stride_ids, parity_stride_key_rows);
}
