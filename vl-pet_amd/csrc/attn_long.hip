// Attention forward for sequences of up to 1,024 keys and 1,024 queries (head dim 64, bf16): softmax(scale * q k^T + bias + masks) v
// with the keys streamed through LDS in chunks and an online softmax -- the video configuration's encoder self-attention (600 text
// tokens + 64 frames = 664) and the cross-attention against it, which csrc/attn.hip (whole sequence on chip, at most 128 keys) does
// not cover.  DROP = false is the inference / no_grad form; DROP = true is the training forward (dropout on the probabilities by the
// short kernels' mask rule, an optional export of the mask); the log-sum-exp is what the backward (csrc/attn_long_bwd.hip) starts from.
//
// Structure: a workgroup is four waves and 128 consecutive queries of one (batch, head); the workgroups of a pair are neighbours in the
// grid, so that the pair's K and V are read from HBM once and from L2 afterwards.  A wave owns a 32-query block with its Q fragments
// in registers and uses the arithmetic of the short forward: K Q^T as 32x32x16 MFMAs in the swapped form (a lane owns a QUERY, its
// accumulator registers are keys), probabilities from the accumulator registers straight into the P V product, V^T through
// ds_read_b64_tr_b16 from a padded row-major image, whole-row stores through a staging tile.  K and V arrive in chunks of 64 keys:
// the chunk after the current one is loaded into registers before the current one is computed and written into the other LDS buffer
// after it, one barrier per chunk.  Running (m, l) per lane -- lane and lane ^ 32 hold the same query and keep identical copies --
// and the O accumulators (lane = query, registers = d) are rescaled by that per-lane scalar.
//
// Every sum has an order that is a function of (Lq, Lk) alone: no atomics, nothing crosses workgroups, a (batch, head) pair never sees
// another pair's data.  The output is bitwise reproducible and independent of the batch.
//
// -inf rules (a masked key is an excluded key): the running maximum starts at -inf; the exponentials are taken against
// m_ref = (m_new == -inf ? 0 : m_new), which is finite, so neither exp2(s - m_ref) nor the rescale factor exp2(m_old - m_ref) ever
// forms -inf - (-inf).  A chunk with no visible key for a row: m_new = m_old, factor exp2(0) = 1 (or 0 on a still-empty row whose l and
// O are 0), every p = 0 -- the row's state is unchanged.  The first visible chunk after masked ones: factor exp2(-inf) = 0 on zeros.
// A row with no visible key at all ends with l = 0: zeros are stored and lse = +inf.
//
// Dropout (DROP): element (b, h, i, j) is kept iff hash_elem(row_key(seed, (b H + h) Lq + i) + j * golden) >= p * 2^32, the one
// rule of csrc/attn_common.h.  l and lse are sums over the UNDROPPED probabilities; the kept ones enter the P V product scaled by 1 / (1 - p).
//
// The mask rule, the LDS geometry, the operand readers, the staged row store and the chunk ring's load / store pair are csrc/attn_common.h's,
// shared with csrc/attn.hip and csrc/attn_long_bwd.hip.
#include <cstdlib>
#include "common.h"
#include "kernels.h"
#include "attn_common.h"

#define AL_NW 4                        // waves per workgroup = 32-query blocks per workgroup
#define AL_QWG (32 * AL_NW)            // queries per workgroup
#define AL_MAXK 1024

namespace {

// BIAS: a.bias != nullptr -- scores = scale * q k^T + bias[h][i][j];  DROP: a.thr != 0 -- the training forward
template <bool BIAS, bool DROP>
__global__ __launch_bounds__(AL_NW * 64, 2) void attn_long_fwd_kernel(AttnArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t kv_img[2][2][AT_IMG];       // [buffer][K | V]
    __shared__ __attribute__((aligned(16))) uint8_t stg_all[AL_NW][AT_STG];
    __shared__ __attribute__((aligned(16))) float kval[AL_MAXK];                // per key: 0 / -inf (the key mask and the keys past Lk)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nqb = (a.Lq + AL_QWG - 1) / AL_QWG;
    const int bh = blockIdx.x / nqb, qblk = blockIdx.x - bh * nqb;
    const int b = bh / a.H, h = bh - b * a.H;
    const int m = lane & 31, hh = lane >> 5;
    const int64_t rs = (int64_t)a.H * 64, rq = a.ld_q, rk = a.ld_kv, rv = a.ld_v;
    const __bf16* qb_ = a.q + (int64_t)b * a.Lq * rq + h * 64;
    const __bf16* kb_ = a.k + (int64_t)b * a.Lk * rk + h * 64;
    const __bf16* vb_ = a.v + (int64_t)b * a.Lk * rv + h * 64;
    __bf16* ob_ = a.o + (int64_t)b * a.Lq * rs + h * 64;
    const uint8_t* km = a.key_mask ? a.key_mask + (int64_t)b * a.Lk : nullptr;
    const int Lkp = (a.Lk + 31) & ~31, Lqp = (a.Lq + 31) & ~31;       // the bias table's padded axes
    const int coff = a.causal ? a.Lk - a.Lq : (1 << 20);             // key j is visible to query i iff j <= i + coff

    // chunks this workgroup walks: all of them, or under the causal rule those up to the last key its last query sees
    const int q0 = AL_QWG * qblk, q0w = q0 + 32 * wave;
    const int qlast = (q0 + AL_QWG < a.Lq ? q0 + AL_QWG : a.Lq) - 1;
    int klast = a.Lk - 1;
    if (a.causal && qlast + coff < klast) klast = qlast + coff;
    const int NC = klast < 0 ? 0 : klast / AT_CK + 1;

    for (int j = tid; j < NC * AT_CK; j += AL_NW * 64) kval[j] = (j < a.Lk && (km == nullptr || km[j] != 0)) ? 0.f : -INFINITY;
    ChunkRegs cr;
    if (NC > 0) {
        chunk_load(cr, kb_, vb_, rk, rv, 0, a.Lk, tid);
        chunk_store(cr, kv_img[0][0], kv_img[0][1], 0, a.Lk, tid);
    }
    const bool has_q = q0w < a.Lq;                                   // (wave-uniform; a wave without a query block only stages)
    const int i = q0w + m;
    const int iq = i < a.Lq ? i : a.Lq - 1;
    bf16x8 qf[4];
    if (has_q) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qb_ + (int64_t)iq * rq + 16 * ks + 8 * hh);
    }
    const float sc2 = a.scale * AT_LOG2E, inv_scale = 1.0f / a.scale;
    float mrun = -INFINITY, lrun = 0.f;
    uint32_t rkey = 0;
    if constexpr (DROP) rkey = row_key(vlpet_eff_seed(a.seed, a.seed_ctr), ((int64_t)b * a.H + h) * a.Lq + iq);
    f32x16 ot0 = zero16(), ot1 = zero16();
    __syncthreads();

    for (int c = 0; c < NC; ++c) {
        const int key0 = AT_CK * c;
        const bool more = c + 1 < NC;
        if (more) chunk_load(cr, kb_, vb_, rk, rv, key0 + AT_CK, a.Lk, tid);
        const uint8_t* Ks = kv_img[c & 1][0];
        const uint8_t* Vs = kv_img[c & 1][1];
        if (has_q) {
            f32x16 st[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                st[t] = zero16();
                if (key0 + 32 * t < Lkp) {                           // (the chunk's second tile may lie past the padded bias row; kval masks it)
                    if constexpr (BIAS) st[t] = bias_tile(a.bias + ((int64_t)h * Lqp + i) * Lkp + key0 + 32 * t + 4 * hh, inv_scale);
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) st[t] = mfma32(nat_frag(Ks, 32 * t + m, ks, hh), qf[ks], st[t]);
                }
            }
            // ---- scores of the chunk in log2 units; masked keys -inf from the table / the causal bound
            float mx = -INFINITY;
            const int ic = i + coff - 4 * hh - key0;                 // key key0 + 32 t + ir + 4 hh is masked iff 32 t + ir > ic
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const f32x4 kv = *reinterpret_cast<const f32x4*>(kval + key0 + 32 * t + 8 * q4 + 4 * hh);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * q4 + e;
                        float s = fmaf(st[t][r], sc2, kv[e]);
                        s = 32 * t + e + 8 * q4 > ic ? -INFINITY : s;
                        st[t][r] = s;
                        mx = fmaxf(mx, s);
                    }
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mnew = fmaxf(mrun, mx);
            const float mref = mnew == -INFINITY ? 0.f : mnew;       // finite: no -inf - (-inf) below
            const float alpha = fast_exp2(mrun - mref);              // 1 when the maximum stays, 0 from a still-empty row
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) { const float p = fast_exp2(st[t][r] - mref); st[t][r] = p; sum += p; }
            }
            sum += __shfl_xor(sum, 32);
            lrun = fmaf(lrun, alpha, sum);
            mrun = mnew;
#pragma unroll
            for (int r = 0; r < 16; ++r) { ot0[r] *= alpha; ot1[r] *= alpha; }
            if constexpr (DROP) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int kt = key0 + 32 * t + 4 * hh;
                    if (a.keep_out != nullptr) {                     // (tests: export of the mask)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int key = kt + (r & 3) + 8 * (r >> 2);
                            if (i < a.Lq && key < a.Lk)
                                a.keep_out[(((int64_t)b * a.H + h) * a.Lq + i) * a.Lk + key] = keep_elem(rkey, key, a.thr) ? 1 : 0;
                        }
                    }
                    const uint32_t kg0 = rkey + (uint32_t)kt * AT_GOLD;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ir = (r & 3) + 8 * (r >> 2);
                        st[t][r] = hash_elem(kg0 + (uint32_t)ir * AT_GOLD) >= a.thr ? st[t][r] * a.inv_keep : 0.f;
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const bf16x8 pf = acc_frag(st[t], u);
                    ot0 = mfma32(tr_acc_order(Vs, 32 * t + 16 * u, 0, lane), pf, ot0);
                    ot1 = mfma32(tr_acc_order(Vs, 32 * t + 16 * u, 32, lane), pf, ot1);
                }
            }
        }
        // the next chunk goes into the buffer whose readers all passed the barrier that ended the previous trip
        if (more) chunk_store(cr, kv_img[(c + 1) & 1][0], kv_img[(c + 1) & 1][1], key0 + AT_CK, a.Lk, tid);
        __syncthreads();
    }
    if (!has_q) return;
    const float inv = lrun > 0.f ? 1.0f / lrun : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { ot0[r] *= inv; ot1[r] *= inv; }
    if (hh == 0 && i < a.Lq) a.lse[((int64_t)b * a.H + h) * a.Lq + i] = lrun > 0.f ? mrun + log2f(lrun) : INFINITY;
    store_rows_T(stg_all[wave], ot0, ot1, ob_, rs, q0w, a.Lq, lane);
}

}  // namespace

hipError_t launch_attn_long_fwd(const AttnArgs& a, hipStream_t stream) {
    if (a.Lq <= 0 || a.Lk <= 0 || a.Lq > AL_MAXK || a.Lk > AL_MAXK) return hipErrorInvalidValue;
    const int nqb = (a.Lq + AL_QWG - 1) / AL_QWG;
    const int64_t wgs = (int64_t)a.B * a.H * nqb;
    if (wgs > 0x7fffffffLL) return hipErrorInvalidValue;
    // (the workgroups of one (batch, head) pair have consecutive indices: they run together and share the pair's K and V in L2)
    // (thr == 0 -- no dropout, the training entry point with p = 0 included -- is the DROP = false kernel: the same bits)
    const dim3 grid((unsigned)wgs), block(AL_NW * 64);
    if (a.thr != 0) {
        if (a.bias != nullptr) hipLaunchKernelGGL((attn_long_fwd_kernel<true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((attn_long_fwd_kernel<false, true>), grid, block, 0, stream, a);
    } else {
        if (a.bias != nullptr) hipLaunchKernelGGL((attn_long_fwd_kernel<true, false>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((attn_long_fwd_kernel<false, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}
