// The device header of the column-parallel and two-pass kernels (pet_cols.hip, pet_cols6y.hip, pet_cols_ng.hip, pet_dz2.hip,
// pet_dz6.hip, pet_fwd2p.hip, visproj_gemm.hip, visproj_wgrad.hip, the streaming half of wgrad.hip).  First the tools: compile-time
// loops, inline-asm LDS accesses with hand-placed waits (see trread.h for why), counted vmcnt waits, bf16 packing, the LDS swizzles,
// the workgroup -> (group, member) map.  Then the pieces of a step that more than one kernel runs, one definition each ("pieces
// of a step" below).  A piece is here only if no parameter tells it which caller it serves: compile-time geometry (RT, KT, PB,
// PT_B, GRP, offsets) is a parameter, a flag for a caller is not -- and only if every kernel still compiles to the listing it had
// (tools/same_code.py).  DESIGN.md section 4 lists what is shared and what stays apart for either reason.
#pragma once
#include <type_traits>
#include <utility>
#include "pet16.h"
#include "kernels.h"
#include "trread.h"

template <typename F, int... I>
__device__ __forceinline__ void sfor_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void sfor(F&& f) { sfor_impl(f, std::make_integer_sequence<int, N>{}); }

template <int OFF> __device__ __forceinline__ void lds_read16(u32x4& o, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(o) : "v"(addr), "n"(OFF) : "memory");
}
template <int OFF> __device__ __forceinline__ void lds_write16(uint32_t addr, const u32x4& v) {
    asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(addr), "v"(v), "n"(OFF) : "memory");
}
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
template <int OFF> __device__ __forceinline__ void lds_read8(u32x2& o, uint32_t addr) {
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(o) : "v"(addr), "n"(OFF) : "memory");
}
template <int OFF> __device__ __forceinline__ void lds_write8(uint32_t addr, const u32x2& v) {
    asm volatile("ds_write_b64 %0, %1 offset:%2" :: "v"(addr), "v"(v), "n"(OFF) : "memory");
}
__device__ __forceinline__ void lgkm_fence(u32x4& a) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a) :: "memory"); }
__device__ __forceinline__ void lgkm_tie(u32x4& a) { asm volatile("" : "+v"(a) :: "memory"); }
__device__ __forceinline__ bf16x8 as_bf(const u32x4& v) { return __builtin_bit_cast(bf16x8, v); }

// transpose read with separate addresses for the two 4-row halves (their rows carry different swizzles)
template <int OFF> __device__ __forceinline__ void tr_read2(TrOp& o, uint32_t alo, uint32_t ahi) {
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(o.lo) : "v"(alo), "n"(OFF) : "memory");
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(o.hi) : "v"(ahi), "n"(OFF) : "memory");
}
// LDS images (all swizzles are applied on the SOURCE side of the global_load_lds: slot = 16-byte unit of a row):
//   row tiles [32 rows x 128 B]: slot ^= fsw(row), fsw = (q & 1) << 2 | q >> 1 with q = (row >> 1) & 7 -- bit 2 alternates every two
//     rows (the four rows of a transpose read fall into four 64-byte bank windows), the other two bits make the 16 rows of a
//     ds_read_b128 lane group distinct (the row-per-lane reads of dy, x2, dh);
//   bottleneck tiles [32 rows x 64*RT B]: slot ^= (row >> 2) & 3 -- the four rows of a transpose read share it (their native
//     conflict-free pattern is kept), the rows 4 apart of a ds_read_b128 lane group (B fragments, lane = row) do not.
__device__ __forceinline__ int fsw(int row) { const int q = (row >> 1) & 7; return ((q & 1) << 2) | (q >> 1); }
__device__ __forceinline__ int gsw(int row) { return (row >> 2) & 3; }

// at most n vector-memory operations of this wave still in flight (n is wave-uniform)
__device__ __forceinline__ void vm_wait(int n) {
#define VLPET_VMW(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
    switch (n) {
        VLPET_VMW(0) VLPET_VMW(1) VLPET_VMW(2) VLPET_VMW(3) VLPET_VMW(4) VLPET_VMW(5) VLPET_VMW(6) VLPET_VMW(7)
        VLPET_VMW(8) VLPET_VMW(9) VLPET_VMW(10) VLPET_VMW(11) VLPET_VMW(12) VLPET_VMW(13) VLPET_VMW(14) VLPET_VMW(15)
        VLPET_VMW(16) VLPET_VMW(17) VLPET_VMW(18) VLPET_VMW(19) VLPET_VMW(20) VLPET_VMW(21) VLPET_VMW(22) VLPET_VMW(23)
        VLPET_VMW(24) VLPET_VMW(25) VLPET_VMW(26) VLPET_VMW(27) VLPET_VMW(28) VLPET_VMW(29) VLPET_VMW(30)
        default: asm volatile("s_waitcnt vmcnt(30)" ::: "memory"); break;       // more than 30: stricter is safe
    }
#undef VLPET_VMW
}

__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ float bf_at(const u32x4& v, int j) { return (j & 1) ? bf_hi(v[j >> 1]) : bf_lo(v[j >> 1]); }
__device__ __forceinline__ u32x4 pack8(const float* v) {
    bf16x8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = (__bf16)v[j];
    return __builtin_bit_cast(u32x4, t);
}
// sigmoid with one v_exp_f32 and one v_rcp_f32
__device__ __forceinline__ float sigm(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}


// Workgroup -> (group, member) map of the column-parallel passes.  A group = the U workgroups that re-read the same bottleneck
// rows (the column blocks of a row chunk); block b runs on XCD b % 8, and a group's members should share an XCD's L2.  Each XCD
// has 32 CUs = G = 32 / U whole groups (slots j = b / 8 < U * G); the 32 - U * G CUs per XCD that are left over take the
// members of a few more groups, spread over the XCDs (those groups re-read their bottleneck rows through several L2s -- a few
// MB -- but at d = 768 they turn 240 busy CUs into 252: two more row chunks, one step less per workgroup).
__host__ __device__ inline int cols_groups_max(int U) { const int G = 32 / U; return 8 * G + ((32 - U * G) * 8) / U; }
__host__ __device__ inline void cols_decode(int b, int U, int& group, int& member) {
    const int G = 32 / U, main = U * G, x = b & 7, j = b >> 3;
    if (j < main) { member = j % U; group = (j / U) * 8 + x; }
    else { const int l = (j - main) * 8 + x; group = 8 * G + l / U; member = l % U; }
}
__host__ __device__ inline unsigned cols_grid(int U, int ngroups) {
    const int G = 32 / U;
    if (ngroups <= 8 * G) return 8u * (unsigned)U * (unsigned)((ngroups + 7) / 8);
    return 8u * (unsigned)(U * G + ((ngroups - 8 * G) * U + 7) / 8);
}
// Row-chunk plan of a column-parallel pass: at most groups_max chunks (one group of workgroups each, cols_groups_max), a chunk a
// multiple of 32 rows, the chunks as even as that allows: no round quantisation.  cols_plan_groups: the groups of a pass whose
// workgroups own 128 columns ((d / 128) column blocks per row chunk; at most 32 workgroups -- one per CU, the ring takes the LDS --
// on an XCD).  (d < 128: the forms do not apply; the plan only sizes workspaces.)
inline void cols_row_chunks(int64_t M, int groups_max, int* row_chunks, int64_t* rows_per_chunk) {
    int64_t rc = groups_max;
    const int64_t blocks32 = (M + 31) / 32;
    if (rc > blocks32) rc = blocks32;
    if (rc < 1) rc = 1;
    const int64_t per = (blocks32 + rc - 1) / rc;
    rc = (blocks32 + per - 1) / per;
    *row_chunks = (int)rc;
    *rows_per_chunk = per * 32;
}
inline int cols_plan_groups(int d) { const int ncb = d >= 128 ? d / 128 : 1; return cols_groups_max(ncb < 32 ? ncb : 32); }

// ================================================================================================== pieces of a step
// A wave-uniform pointer that the compiler must treat as a fresh scalar.  Every stream's address is sbase(row base) + a per-lane
// 32-bit offset: with the base rebuilt from two readfirstlanes the per-lane part stays a 32-bit loop invariant (otherwise hipcc
// hoists one 64-bit per-lane address per stream out of the loop and spills them).
__device__ __forceinline__ const uint8_t* sbase(const uint8_t* p) {
    const uint64_t u = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    return reinterpret_cast<const uint8_t*>(((uint64_t)hi << 32) | lo);
}
// The ring tail.  The last step of a row chunk may have fewer than 32 rows: a lane whose row lies past the last valid one re-reads
// that one (cols_rows_back = how many rows its source address steps back), and the bottleneck rows past the end are zeroed in LDS
// after they landed, so that their products vanish (NT bottleneck tiles [32 rows x PB bytes] from `pt`; the caller's barrier follows).
__device__ __forceinline__ uint32_t cols_rows_back(int row, int last) { return (uint32_t)(row > last ? row - last : 0); }
template <int NT, int PB>
__device__ __forceinline__ void cols_zero_tail(uint8_t* pt, int tid, int valid) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (int q = tid; q < NT * 32 * (PB / 16); q += 512) {
        const int rr = (q / (PB / 16)) & 31;
        if (rr >= valid) *reinterpret_cast<u32x4*>(pt + (size_t)q * 16) = z;
    }
}
// A fragment whose row (slot k = MFMA row (k & 3) + 8 (k >> 2) = register k of the lanes h = 0) is all ones: D[row][n] = column
// sums of the B operand.  m = lane & 31.  Rebuilt at every use (the empty asm): as loop invariants the fragments cost four
// registers per slot.
__device__ __forceinline__ bf16x8 ones_row(int m, int k) {
    int mm = m;
    asm volatile("" : "+v"(mm));
    const uint32_t w = (mm == (k & 3) + 8 * (k >> 2)) ? 0x3f803f80u : 0u;
    const u32x4 v = {w, w, w, w};
    return __builtin_bit_cast(bf16x8, v);
}
// The gate's elementwise backward of one element: (dh, dq) = the gradients at h and at the gate's pre-activation, from
//     y = gs * h * g (ADD: gs * (h + g)),   g = sigmoid(bgu + Wgu z_g) = gt,   h = s2 * x2 + sd * (bu + Wu z_a)
// in its three forms:
//     plain:  dh = gs dy g,   dq = dh h (1 - g)        hy = h, recomputed by the caller from x2 and the adapter chain
//     YF:     dh = gs dy g,   dq = dy y (1 - g)        hy = the forward's output y (= gs h g, so dy y (1 - g) = dh h (1 - g))
//     ADD:    dh = gs dy,     dq = dh g (1 - g)        hy is not read
// The caller forms the two scaled copies of dy, in this order and before hy: dys = gs * v * dy and (read by YF only) dyl = v * dy,
// v = the row-validity factor, 1 or 0 -- rows past the end of a chunk give dh = dq = 0.  (pet_cols.hip folds gs * v into `gsr`,
// pet_cols6y.hip keeps v as `live` next to it; the row kernels of pass 1 clamp their rows instead: dys = gs * dy, dyl = dy.)  The
// order of the products is part of the contract: the results are rounded to bf16 for the matrix cores, and every kernel is held
// to the code it compiled to before the four copies of this became one (the scaling of dy inside this function changed operand
// orders in k1_cols_kernel, which is why it stays with the callers).
template <bool ADD, bool YF>
__device__ __forceinline__ void gate_bwd_ew(float dys, float dyl, float gt, float hy, float& dh, float& dq) {
    if constexpr (ADD) {
        dh = dys;
        dq = dys * gt * (1.0f - gt);
    } else if constexpr (YF) {
        dh = dys * gt;
        dq = dyl * hy * (1.0f - gt);
    } else {
        dh = dys * gt;
        dq = dh * hy * (1.0f - gt);
    }
}

// ================================================================================================== pass 1, feature-split forms
// What pet_dz2.hip and pet_dz6.hip share.
// Cache policy of pass 1's row loads (dy, x2).  Pass 2 reads both tensors again right after this launch: with the non-temporal policy
// of the other row streams (aux 2) pass 1 discourages exactly the lines pass 2 is about to ask for.
constexpr int P1_AUX = 2;
__device__ __forceinline__ void glds16_p1(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((gmem_cv*)gsrc, (lmem_v*)lds_wave_base, 16, 0, P1_AUX);
}
// The elementwise backward of a lane's 16 values (4 features at a time) once their dy and x2 (YF: y) words are on their way from the
// row tiles: dh, dq come out as bf16 pairs in register order -- the B fragments kappa = 0 (words 0-3) and 1 (words 4-7) of the
// contraction.  aG / aA: the gate's and the adapter chain's up projections (aA is read by the plain form only).  PIN: k1_dz2_kernel
// pins the operands of a group of four in registers at the group's start.
template <bool ADD, bool YF, bool PIN>
__device__ __forceinline__ void dz_ew(u32x2* dyv, u32x2* x2v, f32x16& aG, const f32x16* aA, const float& gs, const float& s2,
                                      const float& sd, uint32_t* bh, uint32_t* bq) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(dyv[0]), "+v"(x2v[0]), "+v"(dyv[1]), "+v"(x2v[1]), "+v"(dyv[2]), "+v"(x2v[2]), "+v"(dyv[3]), "+v"(x2v[3]) :: "memory");
    sfor<4>([&](auto Q) {
        constexpr int q = Q.value;
        if constexpr (PIN)
            asm volatile("" : "+v"(dyv[q]), "+v"(x2v[q]), "+v"(aG[4 * q]), "+v"(aG[4 * q + 1]), "+v"(aG[4 * q + 2]), "+v"(aG[4 * q + 3]) :: "memory");
        float dh[4], dq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = 4 * q + j;
            const float gt = sigm(aG[e]);
            const float dyr = (j & 1) ? bf_hi(dyv[q][j >> 1]) : bf_lo(dyv[q][j >> 1]);
            const float dy_ = gs * dyr;
            const float x2r = (j & 1) ? bf_hi(x2v[q][j >> 1]) : bf_lo(x2v[q][j >> 1]);       // x2, or (YF: the row ring's second tile) y
            gate_bwd_ew<ADD, YF>(dy_, dyr, gt, ADD ? 0.f : YF ? x2r : s2 * x2r + sd * (*aA)[e], dh[j], dq[j]);
        }
        typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
        const bf16x4 th = {(__bf16)dh[0], (__bf16)dh[1], (__bf16)dh[2], (__bf16)dh[3]};
        const bf16x4 tq = {(__bf16)dq[0], (__bf16)dq[1], (__bf16)dq[2], (__bf16)dq[3]};
        const u32x2 uh = __builtin_bit_cast(u32x2, th), uq = __builtin_bit_cast(u32x2, tq);
        bh[2 * q] = uh[0]; bh[2 * q + 1] = uh[1];
        bq[2 * q] = uq[0]; bq[2 * q + 1] = uq[1];
    });
}
// host: (M / 128 row blocks) x (feature blocks) workgroups of THREADS, GEO::bytes(d) of LDS; the feature blocks are summed by a second launch
template <typename GEO, int THREADS, int PR>
static hipError_t launch_dz_form(void (*kern)(PetBwdArgs), const PetBwdArgs& a, hipStream_t stream) {
    const size_t lds = GEO::bytes(a.d);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const unsigned blocks = (unsigned)((a.M + 127) / 128);
    const unsigned nfb = a.fsplit > 1 ? (unsigned)a.fsplit : 1u;
    hipLaunchKernelGGL(kern, dim3(blocks, nfb), dim3(THREADS), lds, stream, a);
    if (nfb > 1) return launch_k1_dz_reduce(a, PR, stream);
    return hipGetLastError();
}
