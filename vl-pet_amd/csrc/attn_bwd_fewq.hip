// Short-sequence attention backward for calls with ONE query block (Lq <= 32, Lk <= 128, head dim 64, no score bias): the decoder's
// self-attention (2-20 queries and keys) and cross-attention (2-20 queries against 56-92 encoder tokens).  attn_bwd_kernel (attn.hip)
// gives a (batch, head) pair to a four-wave workgroup and deals T key tiles + NQB query blocks to its waves; with one query block that is
// 2-4 units for 4 waves, the phase-Q wave re-evaluates every score tile the phase-K waves evaluate, and three workgroups per CU run
// stage -> barrier -> compute -> store in sequence.  Here, as in attn_fwd_kernel, a WAVE owns a pair: its LDS images and staging tile are
// private, nothing is synchronised, and a compute unit interleaves eight independent pairs.
//
// The wave loops over the key tiles.  Per tile: S = Q K^T and dP = dO V^T in the UNSWAPPED form (lane = key, registers = queries), P and dS
// elementwise -- each score tile is evaluated once --, dV^T = dO^T P and dK^T = Q^T dS with the accumulator registers as B operands, stored
// before the next tile.  dQ^T += K^T dS contracts over the keys, the lane index of that form: the bf16 dS tile goes through 2.3 KB of the
// wave's LDS ([key][query], 72-byte rows) and comes back transposed by ds_read_b64_tr_b16 in the k order of tr_acc_order(K image); dS is
// rounded to bf16 once and both products take those bits.  dQ^T accumulates in registers across the tiles.
// K is staged one 32-key tile at a time (natural AND transposed reads), the next tile's rows on their way in registers while this one
// is computed; V is only ever read as a natural fragment and goes from global memory straight to registers.
// LDS per wave: Q | dO | K tile images (3 x 4.5 KB) + dS tile + staging tile + row / key tables = 18.9 KB; four waves per workgroup, two
// workgroups per CU.
//
// The arithmetic is attn_bwd_kernel's, operation for operation (tests/attn_spec.py chain(rounded=True)): the same MFMA chains per output
// element, the same elementwise expressions, delta summed in the same order.
#include "common.h"
#include "kernels.h"
#include "attn_common.h"

#define AT_FQ 4                        // waves per workgroup: one (batch, head) pair each
#define AT_DS_ROW 72                   // bytes per row of the dS tile: 32 queries as bf16 + 8 of padding (8-byte aligned; conflict-free 8-byte writes)

struct FewqLds {
    static constexpr size_t IMG = (size_t)32 * AT_ROW;
    static constexpr size_t Q = 0, D = IMG, K = 2 * IMG, DS = 3 * IMG, STG = DS + 32 * AT_DS_ROW;
    static constexpr size_t ROWT = STG + AT_STG;             // [3][32] per query row: lse2 (+inf for rows past Lq) | delta | dropout row key
    static constexpr size_t KVAL = ROWT + 3 * 32 * 4;        // [128] per key: 0 / -inf
    static constexpr size_t wave_bytes = KVAL + 128 * 4;
    static constexpr size_t bytes = AT_FQ * wave_bytes;
};
static_assert(FewqLds::wave_bytes % 16 == 0 && FewqLds::STG % 16 == 0 && FewqLds::ROWT % 16 == 0, "16-byte aligned LDS sections");
static_assert(2 * (FewqLds::bytes + 512) <= (size_t)160 * 1024, "two workgroups per CU");

// the dS tile ([key][query] bf16, AT_DS_ROW bytes per row) as the B operand of dQ^T += K^T dS: lane (c = lane & 31, hh = lane >> 5) gets
// query c of keys kb + 4 hh + {0..3} and kb + 8 + 4 hh + {0..3} -- the k order of tr_acc_order(K image, kb, ...)
__device__ __forceinline__ bf16x8 tr_ds_tile(const uint8_t* img, int kb, int lane) {
    const int g = lane >> 4, sl = lane & 15;
    const uint8_t* p = img + (size_t)(kb + 4 * (g >> 1) + (sl >> 2)) * AT_DS_ROW + (16 * (g & 1) + 4 * (sl & 3)) * 2;
    typedef __attribute__((address_space(3))) v4s16_t lds_v4;
    const v4s16_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(p));
    const v4s16_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(p + 8 * AT_DS_ROW));
    const v8s16_t r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, r);
}

// one 32-row tile of k on its way to the K image (eight 16-byte pieces per row, four per lane) and the same rows of v as natural fragments
struct FewqTile { u32x4 kx[4]; bf16x8 vf[4]; };
__device__ __forceinline__ void fewq_load_tile(FewqTile& r, const __bf16* kb_, const __bf16* vb_, int64_t rk, int64_t rv, int t, int Lk, int lane) {
    const int m = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int idx = lane + 64 * c, row = 32 * t + (idx >> 3), pc = idx & 7;
        const int rr = row < Lk ? row : Lk - 1;                      // (rows past Lk: a valid address; zeros are stored)
        r.kx[c] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kb_ + (int64_t)rr * rk + pc * 8));
    }
    const int j = 32 * t + m, jv = j < Lk ? j : Lk - 1;              // (keys past Lk: P and dS are exact zeros, any finite row will do)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) r.vf[ks] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(vb_ + (int64_t)jv * rv + 16 * ks + 8 * hh));
}

__device__ __forceinline__ void fewq_put_tile(uint8_t* Kt, bf16x8 (&vf)[4], const FewqTile& r, int t, int Lk, int lane) {
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int idx = lane + 64 * c, row = idx >> 3, pc = idx & 7;
        *reinterpret_cast<u32x4*>(Kt + (size_t)row * AT_ROW + pc * 16) = 32 * t + row < Lk ? r.kx[c] : z;
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) vf[ks] = r.vf[ks];
}

__global__ __launch_bounds__(AT_FQ * 64, 2) void attn_bwd_fewq_kernel(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bh = blockIdx.x * AT_FQ + wave;
    if (bh >= a.B * a.H) return;                                     // (the last workgroup's surplus waves; no barrier anywhere below)
    const uint64_t seed = a.thr ? vlpet_eff_seed(a.seed, a.seed_ctr) : 0;
    const int b = bh / a.H, h = bh % a.H;
    const int m = lane & 31, hh = lane >> 5;
    const int T = (a.Lk + 31) >> 5;
    const int64_t rs = (int64_t)a.H * 64, rq = a.ld_q, rk = a.ld_kv, rv = a.ld_v;
    const int64_t ooff = (int64_t)b * a.Lq * rs + h * 64;                                            // o, dout
    const int64_t qoff = (int64_t)b * a.Lq * rq + h * 64, koff = (int64_t)b * a.Lk * rk + h * 64;    // q / dq, k / dk
    const int64_t voff = (int64_t)b * a.Lk * rv + h * 64;                                            // v / dv
    uint8_t* base = smem + (size_t)wave * FewqLds::wave_bytes;
    uint8_t* Qs = base + FewqLds::Q;
    uint8_t* Ds = base + FewqLds::D;                                 // dO
    uint8_t* Kt = base + FewqLds::K;
    uint8_t* dsT = base + FewqLds::DS;
    uint8_t* stg = base + FewqLds::STG;
    float* rowt = reinterpret_cast<float*>(base + FewqLds::ROWT);
    float* kval = reinterpret_cast<float*>(base + FewqLds::KVAL);
    const u32x4 z = {0u, 0u, 0u, 0u};

    FewqTile nx;
    bf16x8 vf[4];
    {
        // every global load of the prologue in flight before the first LDS store, and none of them behind a per-lane branch (rows, keys
        // past the end: a clamped address): 32 rows x 8 pieces = four per lane and tensor
        const bool live_m = m < a.Lq;
        const float lse_m = a.lse[((int64_t)b * a.H + h) * a.Lq + (live_m ? m : a.Lq - 1)];
        uint8_t kmv[2] = {1, 1};
        if (a.key_mask != nullptr) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int key = lane + 64 * c;
                kmv[c] = a.key_mask[(int64_t)b * a.Lk + (key < a.Lk ? key : a.Lk - 1)];
            }
        }
        u32x4 xq[4], xd[4], xo[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int idx = lane + 64 * c, row = idx >> 3, pc = idx & 7;
            const int rr = row < a.Lq ? row : a.Lq - 1;
            xq[c] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.q + qoff + (int64_t)rr * rq + pc * 8));
            xd[c] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.dout + ooff + (int64_t)rr * rs + pc * 8));
            xo[c] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.o + ooff + (int64_t)rr * rs + pc * 8));
        }
        fewq_load_tile(nx, a.k + koff, a.v + voff, rk, rv, 0, a.Lk, lane);
        if (hh == 0) {
            rowt[m] = live_m ? lse_m : INFINITY;
            rowt[64 + m] = __uint_as_float(row_key(seed, ((int64_t)b * a.H + h) * a.Lq + (live_m ? m : a.Lq - 1)));
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int key = lane + 64 * c;
            kval[key] = (key < a.Lk && kmv[c] != 0) ? 0.f : -INFINITY;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int idx = lane + 64 * c, row = idx >> 3, pc = idx & 7;
            const bool live = row < a.Lq;
            *reinterpret_cast<u32x4*>(Qs + (size_t)row * AT_ROW + pc * 16) = live ? xq[c] : z;
            *reinterpret_cast<u32x4*>(Ds + (size_t)row * AT_ROW + pc * 16) = live ? xd[c] : z;
            // delta[row] = sum_d dO[row][d] O[row][d] in attn_bwd_kernel's order: sixteen consecutive products in sequence (the odd piece
            // continues the even piece's sum), then (s0 + s1) + (s2 + s3)
            const bf16x8 fo = __builtin_bit_cast(bf16x8, xo[c]), fd = __builtin_bit_cast(bf16x8, xd[c]);
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += (float)fo[j] * (float)fd[j];
            float acc2 = __shfl_xor(acc, 1);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc2 += (float)fo[j] * (float)fd[j];
            acc2 += __shfl_xor(acc2, 2);                             // (odd pieces hold the sums of sixteen)
            acc2 += __shfl_xor(acc2, 4);
            if (pc == 1) rowt[32 + row] = live ? acc2 : 0.f;
        }
    }
    fewq_put_tile(Kt, vf, nx, 0, a.Lk, lane);
    const float sc2 = a.scale * AT_LOG2E, scale = a.scale, inv_keep = a.thr ? a.inv_keep : 1.0f;
    const uint32_t thr = a.thr;
    const int coff = a.causal ? a.Lk - a.Lq : (1 << 20);             // key j is visible to query i iff j <= i + coff

    f32x16 dq0 = zero16(), dq1 = zero16();
    for (int t = 0; t < T; ++t) {
        // (same-wave LDS accesses are ordered in hardware: no barrier.  The compiler is told not to move the differently typed accesses of
        // the K image, the dS tile and the staging tile across the sections of a trip.)
        asm volatile("" ::: "memory");
        if (t + 1 < T) fewq_load_tile(nx, a.k + koff, a.v + voff, rk, rv, t + 1, a.Lk, lane);

        // ---- the tile, lane = key, registers = queries (attn.hip bwd_k_unit with one query block)
        const int key = 32 * t + m;
        const float kb = kval[key];
        const uint32_t kg = (uint32_t)key * AT_GOLD;
        const int kc = key - coff - 4 * hh;                          // masked iff key > i + coff with i = ir + 4 hh, i.e. kc > ir
        f32x16 s = zero16(), dp = zero16();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            s = mfma32(nat_frag(Qs, m, ks, hh), nat_frag(Kt, m, ks, hh), s);             // D[query][key]
            dp = mfma32(nat_frag(Ds, m, ks, hh), vf[ks], dp);
        }
        const float* rtp = rowt + 4 * hh;                            // the lane half's queries 8 q4 + 4 hh + e: four runs of four
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const f32x4 ls = *reinterpret_cast<const f32x4*>(rtp + 8 * q4);
            const f32x4 dl = *reinterpret_cast<const f32x4*>(rtp + 32 + 8 * q4);
            const f32x4 rkq = *reinterpret_cast<const f32x4*>(rtp + 64 + 8 * q4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * q4 + e, ir = e + 8 * q4;
                float x = fmaf(s[r], sc2, kb - ls[e]);
                x = kc > ir ? -INFINITY : x;
                const float p = fast_exp2(x);
                const bool kp = hash_elem(__float_as_uint(rkq[e]) + kg) >= thr;
                const float g = kp ? dp[r] * inv_keep : 0.f;
                s[r] = kp ? p * inv_keep : 0.f;                      // P after dropout
                dp[r] = p * (g - dl[e]) * scale;                     // dS
            }
        }
        f32x16 dv0 = zero16(), dv1 = zero16(), dk0 = zero16(), dk1 = zero16();
        bf16x8 sf[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bf16x8 pf = acc_frag(s, u);
            sf[u] = acc_frag(dp, u);
            dv0 = mfma32(tr_acc_order(Ds, 16 * u, 0, lane), pf, dv0);                    // D[d][key] += dO^T P
            dv1 = mfma32(tr_acc_order(Ds, 16 * u, 32, lane), pf, dv1);
            dk0 = mfma32(tr_acc_order(Qs, 16 * u, 0, lane), sf[u], dk0);                 // D[d][key] += Q^T dS
            dk1 = mfma32(tr_acc_order(Qs, 16 * u, 32, lane), sf[u], dk1);
        }
        // ---- dQ^T += K^T dS: dS with lane = query
        bf16x8 qf[2];
        {
            // registers 4 g .. 4 g + 3 of the lane's key = queries 8 g + 4 hh + {0..3}: eight bytes of row `key` of the [key][query] tile
            typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const bf16x4_t w = {sf[g >> 1][4 * (g & 1)], sf[g >> 1][4 * (g & 1) + 1], sf[g >> 1][4 * (g & 1) + 2], sf[g >> 1][4 * (g & 1) + 3]};
                *reinterpret_cast<bf16x4_t*>(dsT + (size_t)m * AT_DS_ROW + (8 * g + 4 * hh) * 2) = w;
            }
            asm volatile("" ::: "memory");
#pragma unroll
            for (int u = 0; u < 2; ++u) qf[u] = tr_ds_tile(dsT, 16 * u, lane);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            dq0 = mfma32(tr_acc_order(Kt, 16 * u, 0, lane), qf[u], dq0);                 // D[d][query] += K^T dS
            dq1 = mfma32(tr_acc_order(Kt, 16 * u, 32, lane), qf[u], dq1);
        }
        asm volatile("" ::: "memory");
        // the next tile takes the K image's place BEFORE this tile's stores: the wait for its loads then never has to cover them (the
        // stores sit behind per-lane branches, which a counted wait cannot see through)
        if (t + 1 < T) fewq_put_tile(Kt, vf, nx, t + 1, a.Lk, lane);
        asm volatile("" ::: "memory");
        store_rows_T(stg, dv0, dv1, a.dv + voff, rv, 32 * t, a.Lk, lane);
        store_rows_T(stg, dk0, dk1, a.dk + koff, rk, 32 * t, a.Lk, lane);
    }
    store_rows_T(stg, dq0, dq1, a.dq + qoff, rq, 0, a.Lq, lane);
}

hipError_t launch_attn_bwd_fewq(const AttnArgs& a, hipStream_t stream) {
    if (a.Lq > 32 || a.Lk > 128 || a.bias != nullptr) return hipErrorInvalidValue;
    auto kern = attn_bwd_fewq_kernel;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FewqLds::bytes);
    if (e != hipSuccess) return e;
    const unsigned pairs = (unsigned)(a.B * a.H);
    hipLaunchKernelGGL(kern, dim3((pairs + AT_FQ - 1) / AT_FQ), dim3(AT_FQ * 64), FewqLds::bytes, stream, a);
    return hipGetLastError();
}
