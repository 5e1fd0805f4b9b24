// Attention backward for sequences of up to 1,024 keys and 1,024 queries (head dim 64, bf16): the training form of csrc/attn_long.hip.
// Everything is recomputed from q, k, v, the forward's output and its log-sum-exp (log2 units):
//   P = exp2(sc2 s + bias + masks - lse),  dPd = dO V^T,  dP = keep dPd / (1 - p),  delta_i = sum_d dO_id O_id,  dS = P (dP - delta),
//   dQ = scale dS K,  dK = scale dS^T Q,  dV = (P keep / (1 - p))^T dO;   keep is regenerated from the hash of csrc/attn_common.h, never stored.
//
// Two launches, each a mirror of the forward, with the arithmetic of the short backward's two work units (attn.hip: bwd_q_unit, bwd_k_unit):
//   attn_long_dq_kernel   a workgroup = four waves = 128 consecutive queries of one (batch, head); a wave keeps the Q and dO fragments of its
//                         32 queries in registers (lane = query, accumulator registers = keys) and the K / V chunks of 64 keys come through
//                         the forward's two-buffer LDS ring, one barrier per chunk: S = K Q^T, dPd = V dO^T, dS elementwise, dQ^T += K^T dS.
//                         delta of its queries comes from the dO row the lane holds and the forward's bf16 output -- and is then made
//                         exact (see below) and written to `delta` [B, H, Lq], scratch of the caller, which the second launch reads.
//   attn_long_dkv_kernel  a workgroup = 128 consecutive keys, a wave keeps the K and V fragments of its 32 keys in registers (lane = key,
//                         registers = queries) and the Q / dO chunks of 64 queries come through the ring; lse, delta and the dropout row key of
//                         every query sit in an LDS table built once.  S = Q K^T, dPd = dO V^T, then dV^T += dO^T P, dK^T += Q^T dS with the
//                         P / dS accumulator registers as the B operand and the dO / Q images read through tr_acc_order.
// delta.  sum_d dO O with the ROUNDED output is off by ~2^-9 |dO| |O| sqrt(64), which is all of dS where the softmax is nearly one-hot and
// dropout scales the kept probability (the true dP - delta cancels; one key is the extreme case).  The rows of P sum to 1, so the sum
// over keys of dS / scale = P (dP - delta~) is exactly the missing delta - delta~: the dQ pass accumulates that row sum in fp32 next to
// a fourth product, PK = P K (same K^T fragments as dQ), and ends with dQ -= scale (delta - delta~) PK and delta = delta~ + the row sum.
// The dK / dV pass reads the corrected delta.  (A row with no visible key: P = 0, row sum 0, delta = delta~ = 0.)
//
// S and dPd are computed twice, PK once (8 products, not 5); in exchange nothing is exchanged between workgroups: no atomics, no partial sums, and
// every sum has an order that is a function of (Lq, Lk) alone -- the gradients are bitwise reproducible and an item's gradients do not
// depend on the batch.  The workgroups of a (batch, head) pair are neighbours in the grid: the pair's operands are read from HBM once.
// Under the causal rule a workgroup walks only the chunks that some (query, key) of it can see (again a function of the lengths alone).
//
// -inf rules (a masked key is an excluded key).  The exponent is x = fma(s, sc2, kval - lse) with kval in {0, -inf} (key mask, keys past
// Lk) and lse finite or +inf (+inf: a row with no visible key, and the table's rows past Lq): kval - lse is finite, -inf - finite,
// finite - inf or -inf - inf = -inf -- never inf - inf -- and the causal bound is a select of -inf afterwards.  So a masked key has
// P = exp2(-inf) = 0 and dS = 0 * (finite) = 0; a row with no visible key has P = 0 on every key, delta = 0 (its forward output is zero),
// a zero dQ row and no contribution to dK / dV; a fully masked item gets exact zeros in all three gradients.
//
// The mask rule, the LDS geometry, the operand readers, the staged row store and the chunk ring's load / store pair are csrc/attn_common.h's,
// shared with csrc/attn.hip and csrc/attn_long.hip.
#include <cstdlib>
#include "common.h"
#include "kernels.h"
#include "rng.h"
#include "attn_common.h"

#define AB_NW 4                        // waves per workgroup = 32-row blocks per workgroup
#define AB_WG (32 * AB_NW)             // queries (dQ pass) / keys (dK dV pass) per workgroup
#define AB_MAXL 1024

namespace {

// ---------------------------------------------------------------------------------------------------------------- dQ (and delta)
// BIAS: a.bias != nullptr -- scores = scale * q k^T + bias[h][i][j]
template <bool BIAS>
__global__ __launch_bounds__(AB_NW * 64, 2) void attn_long_dq_kernel(AttnArgs a, float* delta) {
    __shared__ __attribute__((aligned(16))) uint8_t kv_img[2][2][AT_IMG];       // [buffer][K | V]
    __shared__ __attribute__((aligned(16))) uint8_t stg_all[AB_NW][AT_STG];
    __shared__ __attribute__((aligned(16))) float kval[AB_MAXL];                // per key: 0 / -inf (the key mask and the keys past Lk)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t seed = a.thr ? vlpet_eff_seed(a.seed, a.seed_ctr) : 0;
    const int nqb = (a.Lq + AB_WG - 1) / AB_WG;
    const int bh = blockIdx.x / nqb, qblk = blockIdx.x - bh * nqb;
    const int b = bh / a.H, h = bh - b * a.H;
    const int m = lane & 31, hh = lane >> 5;
    const int64_t rs = (int64_t)a.H * 64, rq = a.ld_q, rk = a.ld_kv, rv = a.ld_v;
    const __bf16* qb_ = a.q + (int64_t)b * a.Lq * rq + h * 64;
    const __bf16* kb_ = a.k + (int64_t)b * a.Lk * rk + h * 64;
    const __bf16* vb_ = a.v + (int64_t)b * a.Lk * rv + h * 64;
    const __bf16* ob_ = a.o + (int64_t)b * a.Lq * rs + h * 64;
    const __bf16* db_ = a.dout + (int64_t)b * a.Lq * rs + h * 64;
    __bf16* dqb_ = a.dq + (int64_t)b * a.Lq * rq + h * 64;
    const uint8_t* km = a.key_mask ? a.key_mask + (int64_t)b * a.Lk : nullptr;
    const int Lkp = (a.Lk + 31) & ~31, Lqp = (a.Lq + 31) & ~31;       // the bias table's padded axes
    const int coff = a.causal ? a.Lk - a.Lq : (1 << 20);             // key j is visible to query i iff j <= i + coff

    // chunks this workgroup walks: all of them, or under the causal rule those up to the last key its last query sees
    const int q0 = AB_WG * qblk, q0w = q0 + 32 * wave;
    const int qlast = (q0 + AB_WG < a.Lq ? q0 + AB_WG : a.Lq) - 1;
    int klast = a.Lk - 1;
    if (a.causal && qlast + coff < klast) klast = qlast + coff;
    const int NC = klast < 0 ? 0 : klast / AT_CK + 1;

    for (int j = tid; j < NC * AT_CK; j += AB_NW * 64) kval[j] = (j < a.Lk && (km == nullptr || km[j] != 0)) ? 0.f : -INFINITY;
    ChunkRegs cr;
    if (NC > 0) {
        chunk_load(cr, kb_, vb_, rk, rv, 0, a.Lk, tid);
        chunk_store(cr, kv_img[0][0], kv_img[0][1], 0, a.Lk, tid);
    }
    const bool has_q = q0w < a.Lq;                                   // (wave-uniform; a wave without a query block only stages)
    const int i = q0w + m;
    const int iq = i < a.Lq ? i : a.Lq - 1;
    bf16x8 qf[4], df[4];
    float l2 = INFINITY, dl = 0.f;                                   // (rows past Lq: lse = +inf, every P = 0)
    uint32_t rkey = 0;
    if (has_q) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qf[ks] = *reinterpret_cast<const bf16x8*>(qb_ + (int64_t)iq * rq + 16 * ks + 8 * hh);
            df[ks] = *reinterpret_cast<const bf16x8*>(db_ + (int64_t)iq * rs + 16 * ks + 8 * hh);
        }
        // delta of the row: this lane and lane ^ 32 hold its two halves
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 of = *reinterpret_cast<const bf16x8*>(ob_ + (int64_t)iq * rs + 16 * ks + 8 * hh);
#pragma unroll
            for (int j = 0; j < 8; ++j) dl = fmaf((float)df[ks][j], (float)of[j], dl);
        }
        dl += __shfl_xor(dl, 32);
        const int64_t row = ((int64_t)b * a.H + h) * a.Lq + iq;
        if (i < a.Lq) l2 = a.lse[row];
        rkey = row_key(seed, row);
    }
    const float sc2 = a.scale * AT_LOG2E, inv_scale = 1.0f / a.scale;
    const float inv_keep = a.thr ? a.inv_keep : 1.0f;
    f32x16 dq0 = zero16(), dq1 = zero16(), pk0 = zero16(), pk1 = zero16();
    float rsum = 0.f;                                                // sum over this lane's keys of P (dP - delta~)
    __syncthreads();

    for (int c = 0; c < NC; ++c) {
        const int key0 = AT_CK * c;
        const bool more = c + 1 < NC;
        if (more) chunk_load(cr, kb_, vb_, rk, rv, key0 + AT_CK, a.Lk, tid);
        const uint8_t* Ks = kv_img[c & 1][0];
        const uint8_t* Vs = kv_img[c & 1][1];
        if (has_q) {
            const int ic = i + coff - 4 * hh - key0;                 // key key0 + 32 t + ir + 4 hh is masked iff 32 t + ir > ic
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (key0 + 32 * t >= a.Lk) continue;                 // (a tile past the last key: every P is 0, and the bias row ends before it)
                f32x16 s, dp = zero16();
                if constexpr (BIAS) s = bias_tile(a.bias + ((int64_t)h * Lqp + i) * Lkp + key0 + 32 * t + 4 * hh, inv_scale);
                else s = zero16();
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    s = mfma32(nat_frag(Ks, 32 * t + m, ks, hh), qf[ks], s);             // D[key][query]
                    dp = mfma32(nat_frag(Vs, 32 * t + m, ks, hh), df[ks], dp);
                }
                const uint32_t kg0 = rkey + (uint32_t)(key0 + 32 * t + 4 * hh) * AT_GOLD;
                const int ict = ic - 32 * t;
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const f32x4 kv = *reinterpret_cast<const f32x4*>(kval + key0 + 32 * t + 8 * q4 + 4 * hh);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * q4 + e, ir = e + 8 * q4;
                        float x = fmaf(s[r], sc2, kv[e] - l2);
                        x = ir > ict ? -INFINITY : x;
                        const float p = fast_exp2(x);
                        const bool kp = hash_elem(kg0 + (uint32_t)ir * AT_GOLD) >= a.thr;
                        const float g = kp ? dp[r] * inv_keep : 0.f;
                        const float ds = p * (g - dl);
                        rsum += ds;
                        s[r] = p;                                    // P (undropped: its rows sum to 1)
                        dp[r] = ds * a.scale;                        // dS in place of dP
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const bf16x8 sf = acc_frag(dp, u), pf = acc_frag(s, u);
                    const bf16x8 kt0 = tr_acc_order(Ks, 32 * t + 16 * u, 0, lane), kt1 = tr_acc_order(Ks, 32 * t + 16 * u, 32, lane);
                    dq0 = mfma32(kt0, sf, dq0);                      // D[d][query] += K^T dS
                    dq1 = mfma32(kt1, sf, dq1);
                    pk0 = mfma32(kt0, pf, pk0);                      // D[d][query] += K^T P
                    pk1 = mfma32(kt1, pf, pk1);
                }
            }
        }
        // the next chunk goes into the buffer whose readers all passed the barrier that ended the previous trip
        if (more) chunk_store(cr, kv_img[(c + 1) & 1][0], kv_img[(c + 1) & 1][1], key0 + AT_CK, a.Lk, tid);
        __syncthreads();
    }
    if (!has_q) return;
    rsum += __shfl_xor(rsum, 32);                                    // = delta - delta~ of the row (both lane halves: the same sum)
    if (hh == 0 && i < a.Lq) delta[((int64_t)b * a.H + h) * a.Lq + i] = dl + rsum;
    const float corr = rsum * a.scale;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dq0[r] = fmaf(-corr, pk0[r], dq0[r]); dq1[r] = fmaf(-corr, pk1[r], dq1[r]); }
    store_rows_T(stg_all[wave], dq0, dq1, dqb_, rq, q0w, a.Lq, lane);
}

// ---------------------------------------------------------------------------------------------------------------- dK, dV
template <bool BIAS>
__global__ __launch_bounds__(AB_NW * 64, 2) void attn_long_dkv_kernel(AttnArgs a, const float* delta) {
    __shared__ __attribute__((aligned(16))) uint8_t qd_img[2][2][AT_IMG];       // [buffer][Q | dO]
    __shared__ __attribute__((aligned(16))) uint8_t stg_all[AB_NW][AT_STG];
    __shared__ __attribute__((aligned(16))) float rowt[3][AB_MAXL];             // per query: lse (+inf past Lq) | delta | dropout row key
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t seed = a.thr ? vlpet_eff_seed(a.seed, a.seed_ctr) : 0;
    const int nkb = (a.Lk + AB_WG - 1) / AB_WG;
    const int bh = blockIdx.x / nkb, kblk = blockIdx.x - bh * nkb;
    const int b = bh / a.H, h = bh - b * a.H;
    const int m = lane & 31, hh = lane >> 5;
    const int64_t rs = (int64_t)a.H * 64, rq = a.ld_q, rk = a.ld_kv, rv = a.ld_v;
    const __bf16* qb_ = a.q + (int64_t)b * a.Lq * rq + h * 64;
    const __bf16* kb_ = a.k + (int64_t)b * a.Lk * rk + h * 64;
    const __bf16* vb_ = a.v + (int64_t)b * a.Lk * rv + h * 64;
    const __bf16* db_ = a.dout + (int64_t)b * a.Lq * rs + h * 64;
    __bf16* dkb_ = a.dk + (int64_t)b * a.Lk * rk + h * 64;
    __bf16* dvb_ = a.dv + (int64_t)b * a.Lk * rv + h * 64;
    const uint8_t* km = a.key_mask ? a.key_mask + (int64_t)b * a.Lk : nullptr;
    const int Lkp = (a.Lk + 31) & ~31, Lqp = (a.Lq + 31) & ~31;       // the bias table's padded axes
    const int coff = a.causal ? a.Lk - a.Lq : (1 << 20);             // key j is visible to query i iff j <= i + coff

    // query chunks this workgroup walks: all of them, or under the causal rule those from the first query that sees its first key
    const int k0 = AB_WG * kblk, k0w = k0 + 32 * wave;
    const int NC = (a.Lq + AT_CK - 1) / AT_CK;
    int c0 = 0;
    if (a.causal && k0 - coff > 0) c0 = (k0 - coff) / AT_CK;
    if (c0 > NC) c0 = NC;

    const int64_t row0 = ((int64_t)b * a.H + h) * a.Lq;
    for (int j = AT_CK * c0 + tid; j < NC * AT_CK; j += AB_NW * 64) {
        const bool live = j < a.Lq;
        const int jj = live ? j : a.Lq - 1;
        rowt[0][j] = live ? a.lse[row0 + jj] : INFINITY;
        rowt[1][j] = live ? delta[row0 + jj] : 0.f;
        rowt[2][j] = __uint_as_float(row_key(seed, row0 + jj));
    }
    ChunkRegs cr;
    if (c0 < NC) {
        chunk_load(cr, qb_, db_, rq, rs, AT_CK * c0, a.Lq, tid);
        chunk_store(cr, qd_img[c0 & 1][0], qd_img[c0 & 1][1], AT_CK * c0, a.Lq, tid);
    }
    const bool has_k = k0w < a.Lk;                                   // (wave-uniform; a wave without a key block only stages)
    const int key = k0w + m;
    const int jk = key < a.Lk ? key : a.Lk - 1;
    bf16x8 kf[4], vf[4];
    float kb = -INFINITY;                                            // 0 / -inf: the key mask and the keys past Lk
    if (has_k) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kf[ks] = *reinterpret_cast<const bf16x8*>(kb_ + (int64_t)jk * rk + 16 * ks + 8 * hh);
            vf[ks] = *reinterpret_cast<const bf16x8*>(vb_ + (int64_t)jk * rv + 16 * ks + 8 * hh);
        }
        if (key < a.Lk && (km == nullptr || km[key] != 0)) kb = 0.f;
    }
    const float sc2 = a.scale * AT_LOG2E, inv_scale = 1.0f / a.scale;
    const float inv_keep = a.thr ? a.inv_keep : 1.0f;
    const uint32_t kg = (uint32_t)key * AT_GOLD;
    const int kc = key - coff - 4 * hh;                              // masked iff key > i + coff with i = q0 + 32 t + ir + 4 hh
    f32x16 dv0 = zero16(), dv1 = zero16(), dk0 = zero16(), dk1 = zero16();
    __syncthreads();

    for (int c = c0; c < NC; ++c) {
        const int q0 = AT_CK * c;
        const bool more = c + 1 < NC;
        if (more) chunk_load(cr, qb_, db_, rq, rs, q0 + AT_CK, a.Lq, tid);
        const uint8_t* Qs = qd_img[c & 1][0];
        const uint8_t* Ds = qd_img[c & 1][1];
        if (has_k) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (q0 + 32 * t >= a.Lq) continue;                   // (a tile past the last query: every P is 0, and the bias table ends before it)
                f32x16 s, dp = zero16();
                if constexpr (BIAS) {
                    // bias[h][i][key] for the lane's key and its 16 queries (a wave instruction reads 32 consecutive keys of two rows)
                    const float* bp = a.bias + ((int64_t)h * Lqp + q0 + 32 * t + 4 * hh) * Lkp + key;
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[r] = bp[(int64_t)((r & 3) + 8 * (r >> 2)) * Lkp] * inv_scale;
                } else {
                    s = zero16();
                }
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    s = mfma32(nat_frag(Qs, 32 * t + m, ks, hh), kf[ks], s);             // D[query][key]
                    dp = mfma32(nat_frag(Ds, 32 * t + m, ks, hh), vf[ks], dp);
                }
                const int kcq = kc - q0 - 32 * t;
                const float* rtp = rowt[0] + q0 + 32 * t + 4 * hh;   // the lane half's queries q0 + 32 t + 8 q4 + 4 hh + e: four runs of four
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const f32x4 ls = *reinterpret_cast<const f32x4*>(rtp + 8 * q4);
                    const f32x4 dl = *reinterpret_cast<const f32x4*>(rtp + AB_MAXL + 8 * q4);
                    const f32x4 rk4 = *reinterpret_cast<const f32x4*>(rtp + 2 * AB_MAXL + 8 * q4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * q4 + e, ir = e + 8 * q4;
                        float x = fmaf(s[r], sc2, kb - ls[e]);
                        x = kcq > ir ? -INFINITY : x;
                        const float p = fast_exp2(x);
                        const bool kp = hash_elem(__float_as_uint(rk4[e]) + kg) >= a.thr;
                        const float g = kp ? dp[r] * inv_keep : 0.f;
                        s[r] = kp ? p * inv_keep : 0.f;              // P after dropout
                        dp[r] = p * (g - dl[e]) * a.scale;           // dS
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const bf16x8 pf = acc_frag(s, u), sf = acc_frag(dp, u);
                    dv0 = mfma32(tr_acc_order(Ds, 32 * t + 16 * u, 0, lane), pf, dv0);    // D[d][key] += dO^T P
                    dv1 = mfma32(tr_acc_order(Ds, 32 * t + 16 * u, 32, lane), pf, dv1);
                    dk0 = mfma32(tr_acc_order(Qs, 32 * t + 16 * u, 0, lane), sf, dk0);    // D[d][key] += Q^T dS
                    dk1 = mfma32(tr_acc_order(Qs, 32 * t + 16 * u, 32, lane), sf, dk1);
                }
            }
        }
        if (more) chunk_store(cr, qd_img[(c + 1) & 1][0], qd_img[(c + 1) & 1][1], q0 + AT_CK, a.Lq, tid);
        __syncthreads();
    }
    if (!has_k) return;
    store_rows_T(stg_all[wave], dv0, dv1, dvb_, rv, k0w, a.Lk, lane);
    store_rows_T(stg_all[wave], dk0, dk1, dkb_, rk, k0w, a.Lk, lane);
}

}  // namespace

hipError_t launch_attn_long_bwd(const AttnArgs& a, float* delta, hipStream_t stream) {
    if (a.Lq <= 0 || a.Lk <= 0 || a.Lq > AB_MAXL || a.Lk > AB_MAXL || delta == nullptr) return hipErrorInvalidValue;
    const int64_t pairs = (int64_t)a.B * a.H;
    const int64_t wq = pairs * ((a.Lq + AB_WG - 1) / AB_WG), wk = pairs * ((a.Lk + AB_WG - 1) / AB_WG);
    if (wq > 0x7fffffffLL || wk > 0x7fffffffLL) return hipErrorInvalidValue;
    // (the workgroups of one (batch, head) pair have consecutive indices: they run together and share the pair's operands in L2.
    //  The second launch reads the delta the first one wrote: same stream, in order.)
    if (a.bias != nullptr) hipLaunchKernelGGL(attn_long_dq_kernel<true>, dim3((unsigned)wq), dim3(AB_NW * 64), 0, stream, a, delta);
    else hipLaunchKernelGGL(attn_long_dq_kernel<false>, dim3((unsigned)wq), dim3(AB_NW * 64), 0, stream, a, delta);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.bias != nullptr) hipLaunchKernelGGL(attn_long_dkv_kernel<true>, dim3((unsigned)wk), dim3(AB_NW * 64), 0, stream, a, (const float*)delta);
    else hipLaunchKernelGGL(attn_long_dkv_kernel<false>, dim3((unsigned)wk), dim3(AB_NW * 64), 0, stream, a, (const float*)delta);
    return hipGetLastError();
}
