// Device helpers shared by the attention kernels: csrc/attn.hip (whole sequence on chip, at most 128 keys / queries), csrc/attn_long.hip
// and csrc/attn_long_bwd.hip (up to 1,024, keys or queries streamed through LDS in chunks).  One definition each of
//   * the dropout mask rule -- the forward, the short backward, the long dQ pass and the long dK / dV pass regenerate the same mask bit
//     for bit from it; tests/dropout_spec.py is its host statement;
//   * the LDS geometry (padded 144-byte rows, the 16-row staging tile) and the MFMA operand readers built on it;
//   * the staged whole-row store;
//   * the chunk ring's load / store pair of the long kernels.
// Everything here is __device__ __forceinline__: the kernels' code and register allocation do not depend on which file holds the text.
#pragma once
#include "common.h"

#define AT_LD 72                       // bf16 elements per LDS row: 64 + 8 of padding (144 B: 16-byte aligned, conflict-light)
#define AT_ROW (AT_LD * 2)             // bytes
#define AT_LOG2E 1.4426950408889634f
#define AT_GOLD 0x9E3779B9U            // the dropout mask's Weyl step per key: 2^32 / golden ratio

typedef short v4s16_t __attribute__((ext_vector_type(4)));
typedef short v8s16_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }   // v_exp_f32: arguments here are finite or -inf, never NaN

// ---------------------------------------------------------------- the dropout mask
// Element (b, h, i, j) is kept iff hash_elem(row_key(seed, (b H + h) Lq + i) + j * AT_GOLD) >= p * 2^32: a function of the element index
// and the call's seed only, so every kernel that needs the mask regenerates it.
__device__ __forceinline__ uint32_t hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
// per-row key of the dropout mask: rows are (b, h, i) triples.  The seed is hashed down to a 32-bit key before the row index is
// added: the earlier form hashed seed_lo ^ row, so the seeds s and s ^ 1 gave the same rows in swapped pairs (row r of one mask =
// row r ^ 1 of the other).  Once per row, not per element.
__device__ __forceinline__ uint32_t row_key(uint64_t seed, int64_t row) {
    const uint32_t k = hash32((uint32_t)seed ^ hash32((uint32_t)(seed >> 32) + (uint32_t)((uint64_t)row >> 32)));
    return hash32(k + (uint32_t)row);
}
// element (row, j): the row's key plus a Weyl step per column, one multiply-xorshift round, a rotation by 16 and a second multiply
// (v_alignbit_b32 + v_mul_lo_u32 more than the first form; a full hash32 is nine operations -- the backward kernels are bound by
// their instruction count).  The second multiply is needed: with one round the top bits of columns j and j + k stayed nearly a
// constant offset apart, and column pairs of a mask were correlated by up to 0.037 at any number of rows (tests/test_dropout_spec.py;
// independent columns give 0).  The rotation brings the bits the xorshift mixed to the bottom, where the multiply spreads them
// upwards -- and the compiler keeps the three-tile backward kernels within 168 registers with it, where a bare second multiply spilled.
__device__ __forceinline__ uint32_t hash_elem(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15;
    return __builtin_amdgcn_alignbit(x, x, 16) * 0x846ca68bU;
}
__device__ __forceinline__ bool keep_elem(uint32_t rk, int j, uint32_t thr) { return hash_elem(rk + (uint32_t)j * AT_GOLD) >= thr; }

// ---------------------------------------------------------------- MFMA operands
// A operand from a row-major LDS image: lane (c = lane & 31, hh = lane >> 5) gets column cb + c of rows
// kb + 4 hh + {0..3} (slots 0..3) and kb + 8 + 4 hh + {0..3} (slots 4..7) -- the row order in which a 32x32 accumulator
// tile hands its registers 8u .. 8u+7 to the next MFMA (accumulator register r of lane half hh is row (r & 3) + 8 (r >> 2) + 4 hh).
__device__ __forceinline__ bf16x8 tr_acc_order(const uint8_t* img, int kb, int cb, int lane) {
    const int g = lane >> 4, sl = lane & 15;
    const uint8_t* p = img + (size_t)(kb + 4 * (g >> 1) + (sl >> 2)) * AT_ROW + (cb + 16 * (g & 1) + 4 * (sl & 3)) * 2;
    typedef __attribute__((address_space(3))) v4s16_t lds_v4;
    const v4s16_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(p));
    const v4s16_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(p + 8 * AT_ROW));
    const v8s16_t r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, r);
}
// natural operand: row `row` of the image, 8 consecutive columns at 16 ks + 8 hh
__device__ __forceinline__ bf16x8 nat_frag(const uint8_t* img, int row, int ks, int hh) {
    return *reinterpret_cast<const bf16x8*>(img + (size_t)row * AT_ROW + (16 * ks + 8 * hh) * 2);
}
__device__ __forceinline__ bf16x8 acc_frag(const f32x16& t, int u) {
    bf16x8 f;
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (__bf16)t[8 * u + j];
    return f;
}
// accumulator tile initialised with the lane's 16 bias values (four runs of four floats from a padded fp32 row) over the score scale:
// the MFMAs then accumulate q k^T onto it and no extra registers live through the products
__device__ __forceinline__ f32x16 bias_tile(const float* brow, float inv_scale) {
    f32x16 t;
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(brow + 8 * q4);
#pragma unroll
        for (int e = 0; e < 4; ++e) t[4 * q4 + e] = bv[e] * inv_scale;
    }
    return t;
}

// ---------------------------------------------------------------- the staged whole-row store
// accumulator pair D[d][row] (two 32-wide d tiles; lane = row, registers = d) -> global rows through the wave's 16 x 128 B staging
// tile (144-byte rows), sixteen rows at a time with both d tiles, so that every store instruction writes eight WHOLE 128-byte rows.
// (The first version staged one d tile at a time and stored 64 bytes per row: the backward spent 56 of its 118 us at B = 500, S = 56
// writing 129 MB as half lines -- profiles/r04_attnbwd_ablation.txt.  Sixteen rows, not 32: the staging tiles decide how many
// workgroups fit a CU's LDS.)
#define AT_SROW 144
#define AT_STG (16 * AT_SROW)
__device__ __forceinline__ void store_rows_T(uint8_t* stg, const f32x16& t0, const f32x16& t1, __bf16* dst, int64_t rs,
                                             int row0, int n_rows, int lane) {
    const int m = lane & 31, hh = lane >> 5;
    typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if ((m >> 4) == half) {
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const f32x16& t = dt ? t1 : t0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    bf16x4_t w;
#pragma unroll
                    for (int e = 0; e < 4; ++e) w[e] = (__bf16)t[4 * q + e];
                    *reinterpret_cast<bf16x4_t*>(stg + (size_t)(m & 15) * AT_SROW + (32 * dt + 8 * q + 4 * hh) * 2) = w;
                }
            }
        }
        // (same-wave LDS accesses are ordered in hardware: no barrier.  The compiler is told: the tile is written as bf16x4 and read
        // as u32x4, which type-based alias analysis would otherwise let it reorder across the two halves.)
        asm volatile("" ::: "memory");
        u32x4 v[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int idx = lane + 64 * c, row = idx >> 3, pc = idx & 7;
            v[c] = *reinterpret_cast<const u32x4*>(stg + (size_t)row * AT_SROW + pc * 16);
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int idx = lane + 64 * c, row = 16 * half + (idx >> 3), pc = idx & 7;
            if (row0 + row < n_rows) *reinterpret_cast<u32x4*>(dst + (int64_t)(row0 + row) * rs + pc * 8) = v[c];
        }
    }
}

// ---------------------------------------------------------------- the long kernels' chunk ring
#define AT_CK 64                       // rows per streamed chunk
#define AT_IMG (AT_CK * AT_ROW)        // one image of a chunk
// one chunk of two row streams (K and V, or Q and dO) on its way from global memory to an LDS buffer: 64 rows x 8 pieces of 16 bytes per
// image, two per thread of a 256-thread workgroup
struct ChunkRegs { u32x4 x[2], y[2]; };
__device__ __forceinline__ void chunk_load(ChunkRegs& r, const __bf16* xb, const __bf16* yb, int64_t rx, int64_t ry, int row0, int L, int tid) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int idx = tid + 256 * c, row = row0 + (idx >> 3), pc = idx & 7;
        const int rr = row < L ? row : L - 1;                    // (rows past L: a valid address; zeros are stored below)
        r.x[c] = *reinterpret_cast<const u32x4*>(xb + (int64_t)rr * rx + pc * 8);
        r.y[c] = *reinterpret_cast<const u32x4*>(yb + (int64_t)rr * ry + pc * 8);
    }
}
__device__ __forceinline__ void chunk_store(const ChunkRegs& r, uint8_t* Xs, uint8_t* Ys, int row0, int L, int tid) {
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int idx = tid + 256 * c, row = idx >> 3, pc = idx & 7;
        const bool live = row0 + row < L;
        *reinterpret_cast<u32x4*>(Xs + (size_t)row * AT_ROW + pc * 16) = live ? r.x[c] : z;
        *reinterpret_cast<u32x4*>(Ys + (size_t)row * AT_ROW + pc * 16) = live ? r.y[c] : z;
    }
}
