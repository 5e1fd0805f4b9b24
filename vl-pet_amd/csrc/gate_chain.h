// The device header of the chain-split gated K1 kernels: the row kernels of pet_gate_fwd.hip, pet_gate_bwd2.hip and pass 1 of
// pet_gate_bwd3.hip (a 32-row group is carried by two waves on one SIMD, the adapter chain A and the gate chain G), and pass 2 of
// pet_gate_bwd3.hip in its two schedules (pet_gate_cols_kernel, pet_gate_cols2_kernel).  One definition of a piece that more than
// one of these kernels runs -- under the rule of cols_common.h: compile-time geometry is a parameter, a flag that names the caller
// is not, and every kernel still compiles to the listing it had (tools/same_code.py).  That last condition decides what is here:
// these kernels sit at their register limits, and most bodies that were moved out of them came back with their address arithmetic
// in another order (profiles/chain_family_same_code.md lists them).  Scalars that a piece only reads are `const T&` on purpose:
// the pieces replace lambdas that captured them by reference, and with by-value parameters the same bodies compile differently.
// DESIGN.md section 4 has the dispatch table of the family and the list of what is shared and what stays apart.
#pragma once
#include <type_traits>
#include "kernels.h"
#include "pet32.h"

// ================================================================================================== row kernels
// LDS of a chain-split row kernel: weight ring 2 x [A segment | G segment], then three row slots of [t0 | t1] tiles (RG * 32 rows
// of 128 bytes each), then the fp32 biases of both chains.  What a kernel keeps in the row slots is in its own header.
template <typename IO, int RT, int RG>
struct ChainLds {
    static constexpr int NS = Geo4<IO>::NS;
    static constexpr int SEG_KB = 4 * RT;                       // 1 KiB pieces of one chain's weight segment of a stage
    static constexpr int W_B = SEG_KB * 1024 * 2;
    static constexpr int TILE_B = RG * 32 * 128;
    static constexpr int ROW_B = 2 * TILE_B;
    static constexpr int ROW_OFF = 2 * W_B;
    static constexpr int BIAS_OFF = ROW_OFF + 3 * ROW_B;
    static size_t bytes(int d) { return (size_t)BIAS_OFF + (size_t)2 * (32 * RT + d) * 4; }
};
// slot accessors of the backward row kernels: this chain's weight segment of ring slot j, the two tiles of row slot j
template <typename L> __device__ __forceinline__ uint8_t* chain_slot_w(uint8_t* smem, bool isA, int j) {
    return smem + (size_t)j * L::W_B + (isA ? 0 : L::SEG_KB * 1024);
}
template <typename L> __device__ __forceinline__ uint8_t* chain_slot_t0(uint8_t* smem, int j) { return smem + L::ROW_OFF + (size_t)j * L::ROW_B; }
template <typename L> __device__ __forceinline__ uint8_t* chain_slot_t1(uint8_t* smem, int j) { return chain_slot_t0<L>(smem, j) + L::TILE_B; }

// accumulators of an up projection seeded with the lane's bias values: register i of n-tile v <-> b[16 v + i]
template <int NV>
__device__ __forceinline__ void bias_seed(const float* b, f32x16* au) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 tb = *reinterpret_cast<const f32x4*>(b + 16 * v + 4 * q);
            au[v][4 * q] = tb[0]; au[v][4 * q + 1] = tb[1]; au[v][4 * q + 2] = tb[2]; au[v][4 * q + 3] = tb[3];
        }
    }
}
// Projection of a stage, out[v] += W(v, ks) . p[ks], with the fragment reads one k-step ahead of the MFMAs: 2 * NV fragments live
// instead of NV * KT -- for kernels with no registers to spare (pass 2: a wave holds 96 or 192 accumulator registers).
template <int NS, int NV, int KT>
__device__ __forceinline__ void project_ahead(const uint8_t* w, const int& lane, const Frag<NS>* p, f32x16* out) {
    Frag<NS> cur[NV], nxt[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) cur[v] = wfrag<NS>(w, v * KT, lane);
#pragma unroll
    for (int ks = 0; ks < KT; ++ks) {
        if (ks + 1 < KT) {
#pragma unroll
            for (int v = 0; v < NV; ++v) nxt[v] = wfrag<NS>(w, v * KT + ks + 1, lane);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int v = 0; v < NV; ++v) out[v] = mfma_ns<NS>(cur[v], p[ks], out[v]);
        __builtin_amdgcn_sched_barrier(0);
        if (ks + 1 < KT) {
#pragma unroll
            for (int v = 0; v < NV; ++v) cur[v] = nxt[v];
        }
    }
}

// ---- host: the launcher of the row kernels (workgroups of RG * 32 rows, L::bytes(d) of dynamic LDS), and the two switches that
// turn run-time values into template arguments.  f receives std::integral_constant values (and a value of the IO type).
template <typename L, int RG, int THREADS, typename Args>
static hipError_t launch_chain_rows(void (*kern)(Args), const Args& a, hipStream_t stream) {
    const size_t lds = L::bytes(a.d);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const int rows = RG * 32;
    const int blocks = (int)((a.M + rows - 1) / rows);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(THREADS), lds, stream, a);
    return hipGetLastError();
}
// row groups of the backward row kernels by pick_row_groups' cost model (three only where the weight segment splits evenly)
template <int RT, typename F>
static hipError_t with_row_groups(int64_t M, F&& f) {
    switch (pick_row_groups(M, 4, 2)) {
        case 4: return f(std::integral_constant<int, 4>{});
        case 3: if constexpr ((4 * RT) % 3 == 0) return f(std::integral_constant<int, 3>{});   // (else: falls through)
        default: return f(std::integral_constant<int, 2>{});
    }
}
// (io_fp32, RT) -> f(IO{}, integral_constant<RT>): one and three tiles, and six where the form has it (SIX)
template <bool SIX, typename F>
static hipError_t with_io_rt(int io_fp32, int RT, F&& f) {
    if (RT == 1) return io_fp32 ? f(float{}, std::integral_constant<int, 1>{}) : f(__bf16{}, std::integral_constant<int, 1>{});
    if (RT == 3) return io_fp32 ? f(float{}, std::integral_constant<int, 3>{}) : f(__bf16{}, std::integral_constant<int, 3>{});
    if constexpr (SIX) {
        if (RT == 6) return io_fp32 ? f(float{}, std::integral_constant<int, 6>{}) : f(__bf16{}, std::integral_constant<int, 6>{});
    }
    return hipErrorInvalidValue;
}

// ================================================================================================== pass 2 (column-parallel)
struct ColsArgs {
    const void* dy; const void* x1; const void* x2;
    const void* z_a; const void* z_g;       // the forward's saved z  [M, 32*RT]
    const void* dp_a; const void* dp_g;     // pass 1's dpre         [M, 32*RT]
    void* dx1; void* dx2;
    const uint8_t* pk_a; const uint8_t* pk_g;
    int64_t M;
    int d, RT;
    float s2, sd, gs;
    int flags;
    int GS, NG;                             // feature blocks per XCD group, groups per row chunk (S = GS * NG)
    WgradArgs wg;                           // partial layout (job 0 dWd, 1 dWu, 2 dWgd, 3 dWgu), row_chunks, rows_per_chunk
};

template <typename IO, int NRG, int NBUF_>
struct ColsLds {
    using G = Geo4<IO>;
    static constexpr int NBUF = NBUF_;                              // input tile buffers (NBUF - 1 iterations ahead)
    static constexpr int TILE_B = 32 * 128;
    static constexpr int XH_B = 32 * G::FE * 4;                     // fp32 exchange of h: LW values per lane
    static constexpr int RG_B = (3 * NBUF + 2) * TILE_B + XH_B;     // x2, dy, x1 buffers; dh, dq tiles; exchange
    static int w_bytes(int RT) { return 4 * 4 * RT * 1024; }        // [up A | up G | down_t A | down_t G] of one stage
    static size_t bytes(int RT) {
        const size_t main = (size_t)w_bytes(RT) + NRG * RG_B + 2 * G::FE * 4;
        const size_t red = NRG > 1 ? (size_t)4 * (RT * G::NV * 16 + RT + G::NV) * 64 * 4 : 0;     // end-of-kernel reduction over the row groups
        return main > red ? main : red;
    }
};

// identity fragments: natural fragments (lane = row) times these give the transpose in the C/D layout (wgrad.hip's operand
// construction); I0 selects rows 0..15 of the 32, I1 rows 16..31
__device__ __forceinline__ void cols_identity(const int& m, const int& h, bf16x8& I0, bf16x8& I1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        I0[j] = (m == 8 * h + j) ? (__bf16)1.0f : (__bf16)0.0f;
        I1[j] = (m == 16 + 8 * h + j) ? (__bf16)1.0f : (__bf16)0.0f;
    }
}
// The wave's 32 rows from row0t of feature block su: global -> LDS tile (four instructions), and a staged tile -> whole-line
// stores (returns the number of store instructions).  voff = the kernels' row-tile addressing: instruction i of a wave moves rows
// 8i + (lane >> 3), 16-byte piece (lane & 7) ^ swz(row) -- a wave-uniform 64-bit base per block plus a 32-bit per-lane offset
// (full blocks; the ragged last block clamps per lane).  The parameters are the former lambdas' captures spelled as they were
// captured (the argument block, d, su, lane and voff by reference): with `int64_t M` / `const uint32_t* voff` by value the same
// bodies moved the listing of all six pass-2 kernels.
template <typename IO>
__device__ __forceinline__ void cols_load_tile(const uint8_t* src, const int64_t& row0t, const ColsArgs& a, const int& d, const int& su,
                                               const int& lane, const uint32_t (&voff)[4], uint8_t* dst) {
    if (row0t + 32 <= a.M) {
        const uint8_t* base = src + row0t * d * (int64_t)sizeof(IO) + su * 128;
#pragma unroll
        for (int i = 0; i < 4; ++i) glds16_row(base + voff[i], dst + i * 1024);
    } else {
        const RowLanes rl = row_lanes<IO>(row0t, a.M, d, 0, lane);
        glds_rows4(src, rl, su * 128, dst, 0);
    }
}
template <typename IO>
__device__ __forceinline__ int cols_store_tile(uint8_t* base_out, const int64_t& row0t, const ColsArgs& a, const int& d, const int& su,
                                               const int& lane, const uint32_t (&voff)[4], const uint8_t* tile) {
    if (row0t + 32 <= a.M) {
        uint8_t* base = base_out + row0t * d * (int64_t)sizeof(IO) + su * 128;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(tile + ((size_t)(8 * i + (lane >> 3)) * 8 + (lane & 7)) * 16);
            *reinterpret_cast<u32x4*>(base + voff[i]) = v;
        }
        return 4;
    }
    const RowLanes rl = row_lanes<IO>(row0t, a.M, d, 0, lane);
    store_rows4(base_out, rl, su * 128, tile, 0, lane);
    return rl.n_inst;
}

template <int NS>
__device__ __forceinline__ f32x16 transpose32(const Frag<NS>& lo16, const Frag<NS>& hi16, bf16x8 I0, bf16x8 I1) {
    f32x16 t = zero16();
#pragma unroll
    for (int p = 0; p < NS; ++p) {
        t = mfma32(lo16.p[p], I0, t);
        t = mfma32(hi16.p[p], I1, t);
    }
    return t;
}
template <int NS>
__device__ __forceinline__ Frag<NS> zero_frag() {
    Frag<NS> f;
#pragma unroll
    for (int p = 0; p < NS; ++p)
#pragma unroll
        for (int j = 0; j < 8; ++j) f.p[p][j] = (__bf16)0.0f;
    return f;
}
