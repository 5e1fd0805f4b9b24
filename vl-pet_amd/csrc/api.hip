// C ABI of libvlpet_hip.so (declared in include/vlpet_hip.h): argument checking + launch plumbing.
#include <algorithm>
#include <atomic>
#include "../../include/vlpet_hip.h"
#include "common.h"
#include "kernels.h"
#include <cmath>
#include <stdlib.h>
#include <stdio.h>
#include <vector>

#define VLPET_VERSION 690      // 690: vlpet_colsum_seg, vlpet_colsum_seg_workspace_bytes, vlpet_act_dropout_bwd_cols (biasgrad.hip: segmented column sums of a strided matrix and the FFN activation backward that leaves the column partials of its result -- the bias gradients of the BitFit runs); 681: vlpet_hyper_gen_fwd, vlpet_hyper_gen_bwd, vlpet_hyper_gen_workspace_bytes (hyper.hip: Hyperformer's weight generator of one stack, S linear maps on the same E embedding rows, and its backward); 680: vlpet_prefix_concat_dropout_fwd, vlpet_prefix_concat_dropout_bwd, vlpet_prefix_concat_chunks, vlpet_prefix_concat_ws_bytes (prefix_cat.hip: the joint encoder's input assembly with a broadcast prompt in front, prompt tuning); 670: vlpet_phm_expand_pair_fwd, vlpet_phm_expand_pair_bwd, vlpet_phm_workspace_bytes (phm.hip: Compacter's PHM weight expansion of one adapter and its backward); 660: vlpet_adapter_tail_fwd, vlpet_adapter_tail_applies, vlpet_adapter_tail_rows (adapter_tail.hip: sequential adapter + residual + norm in one launch, inference form); 651: vlpet_attn_long_fwd_train, vlpet_attn_long_bwd (attn_long.hip with dropout, attn_long_bwd.hip: the training form of the attention up to 1,024 keys / queries); 650: vlpet_attn_long_fwd (attn_long.hip: attention forward up to 1,024 keys / queries, no dropout); 640: vlpet_attn_decode_at, vlpet_greedy_pick_at, vlpet_beam_rows_at, vlpet_beam_advance_at (decode.hip: the step position read from device memory, for a replayed decode step); 630: vlpet_attn_decode_beam, vlpet_beam_rows, vlpet_beam_advance (decode.hip: beam search); 620: vlpet_attn_decode, vlpet_greedy_pick (decode.hip: cached greedy generation); 610: vlpet_set_in_launch_reduce and vlpet_finalize_defer / _pending / _discard / _flush removed (the in-launch reduce is chosen per call: phases bit 5); 600 (round 6): in-launch reduce-scatter of the K1 backward (cols_reduce.h; vlpet_adapter_gate_bwd_finalize_launch, phases bit 5), K4 give-up repair inside the call (vlpet_visproj_gemm_exchange_bytes; larger workspace), vlpet_test_hold_cus; 500 (round 5): vlpet_visproj_fwd_gemm (K4 as a tiled GEMM + exchanged statistics), vlpet_sublayer_tail_rms_fwd / vlpet_rmsnorm_tail_bwd, vlpet_adapter_gate_bwd_saved_y (backward from the forward's output), vlpet_finalize_defer / _flush; 420: vlpet_lora_delta_fwd_r8 (K3 at rank <= 8 as a streaming kernel, lora8.hip); 410: vlpet_set_seed_counter (dropout seeds under graph replay), two-pass K2 / K3 forward; 400: two-pass K1 forward (pet_fwd2p.hip), vlpet_sublayer_tail_bwd_out;
#define VLPET_VERSION_R3 300      // 300: column-parallel K1 backward pass (pet_cols.hip), phases bits 3 / 4, vlpet_adapter_gate_bwd_form;
#define VLPET_VERSION_R2 221      // 221: vlpet_sublayer_tail_reduce, vlpet_layernorm_bwd_xhat, vlpet_rmsnorm_{fwd,bwd}, vlpet_colsum;  round 2: LoRA dropout generator ABI, sliced AdamW, K3 training form; 210: strided attention entry points, streaming weight gradients; 220: low-rank visual projector

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }
static inline int herr(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }

extern "C" int vlpet_version(void) { return VLPET_VERSION; }
extern "C" int vlpet_debug_build(void) { return VLPET_IS_DEBUG_BUILD; }

// Test instrument (tests/test_gpu_k4.py, tests/test_gpu_cols.py: the in-launch hand-offs under a GPU that is NOT the launch's alone):
// `workgroups` workgroups of 64 threads, each holding `lds_bytes` of LDS (so one sits on a CU and a workgroup needing more than
// 160 KiB - lds_bytes does not fit beside it), poll *release until it is nonzero or `max_ms` milliseconds have passed, whichever is
// first -- the bound (capped at 10 s) makes a forgotten release harmless.
__global__ __launch_bounds__(64) void hold_cus_kernel(unsigned* release, unsigned long long ticks) {
    extern __shared__ __attribute__((aligned(16))) uint8_t hold_smem[];
    typedef __attribute__((address_space(1))) unsigned gu32;
    if (threadIdx.x == 0) {
        hold_smem[0] = 1;
        const unsigned long long t0 = wall_clock64();
        while (__hip_atomic_load((gu32*)release, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u && wall_clock64() - t0 < ticks)
            __builtin_amdgcn_s_sleep(32);
    }
}
extern "C" int vlpet_test_hold_cus(int workgroups, int lds_bytes, void* release_flag, int max_ms, vlpet_stream_t stream) {
    if (!release_flag) return VLPET_E_NULL;
    if (workgroups <= 0 || workgroups > 1024 || lds_bytes < 0 || lds_bytes > 160 * 1024 || max_ms <= 0) return VLPET_E_SHAPE;
    if (max_ms > 10000) max_ms = 10000;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(hold_cus_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return herr(e);
    hipLaunchKernelGGL(hold_cus_kernel, dim3((unsigned)workgroups), dim3(64), (size_t)lds_bytes, (hipStream_t)stream,
                       reinterpret_cast<unsigned*>(release_flag), (unsigned long long)max_ms * 100000ull);     // wall_clock64: 100 MHz
    return herr(hipGetLastError());
}

extern "C" const char* vlpet_error_string(int code) {
    switch (code) {
        case 0: return "success";
        case VLPET_E_SHAPE: return "bad shape (need M > 0, d % 64 == 0, r > 0)";
        case VLPET_E_RANK: return "unsupported bottleneck rank (max 192) or tile count";
        case VLPET_E_ALIGN: return "pointer not 16-byte aligned";
        case VLPET_E_WORKSPACE: return "workspace too small";
        case VLPET_E_NULL: return "required pointer is NULL";
        case VLPET_E_DTYPE: return "unsupported dtype";
        case VLPET_E_ALIAS: return "output overlaps an input";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

extern "C" int vlpet_rank_tiles(int r) {
    if (r <= 0) return VLPET_E_SHAPE;
    if (r <= 32) return 1;
    if (r <= 96) return 3;
    if (r <= 192) return 6;
    return VLPET_E_RANK;
}

static inline bool tiles_ok(int t) { return t == 1 || t == 3 || t == 6; }
static inline bool dtype_ok(int t) { return t == VLPET_F32 || t == VLPET_BF16; }

extern "C" size_t vlpet_packed_bytes(int tiles, int d, int io_dtype) {
    return (size_t)pack_geom(tiles, d, io_dtype == VLPET_F32 ? 2 : 1).total_bytes;
}

extern "C" int vlpet_pack_pair(const void* const* wd_heads, const void* const* bd_heads, int n_heads,
                               const void* wu, const void* bu, int r, int d, int tiles,
                               int param_dtype, int io_dtype, void* packed, vlpet_stream_t stream) {
    if (!wd_heads || !wu || !packed) return VLPET_E_NULL;
    if (r <= 0 || d <= 0 || d % 64 != 0 || n_heads <= 0 || n_heads > VLPET_MAX_HEADS || r % n_heads != 0)
        return VLPET_E_SHAPE;
    if (!tiles_ok(tiles) || r > 32 * tiles) return VLPET_E_RANK;
    if (!dtype_ok(param_dtype) || !dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (!aligned16(packed)) return VLPET_E_ALIGN;
    PackArgs a;
    for (int i = 0; i < VLPET_MAX_HEADS; ++i) {
        a.wd[i] = i < n_heads ? wd_heads[i] : nullptr;
        a.bd[i] = (bd_heads && i < n_heads) ? bd_heads[i] : nullptr;
        if (i < n_heads && a.wd[i] == nullptr) return VLPET_E_NULL;
    }
    a.wu = wu; a.bu = bu;
    a.n_heads = n_heads; a.rows_per_head = r / n_heads;
    a.r = r; a.d = d; a.RT = tiles; a.src_bf16 = param_dtype == VLPET_BF16;
    a.n_packs = 4;
    a.out = reinterpret_cast<uint8_t*>(packed);
    return herr(launch_pack_pair(a, io_dtype == VLPET_F32 ? 2 : 1, (hipStream_t)stream));
}

extern "C" int vlpet_pack_pairs(int n, const void* const* wd_heads_flat, const void* const* bd_heads_flat, int n_heads,
                                const void* const* wu, const void* const* bu, int r, int d, int tiles,
                                int param_dtype, int io_dtype, void* const* packed, vlpet_stream_t stream) {
    if (n <= 0) return 0;
    if (!wd_heads_flat || !wu || !packed) return VLPET_E_NULL;
    if (r <= 0 || d <= 0 || d % 64 != 0 || n_heads <= 0 || n_heads > VLPET_MAX_HEADS || r % n_heads != 0) return VLPET_E_SHAPE;
    if (!tiles_ok(tiles) || r > 32 * tiles) return VLPET_E_RANK;
    if (!dtype_ok(param_dtype) || !dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    for (int i0 = 0; i0 < n; i0 += VLPET_PACK_BATCH) {
        PackBatch b;
        b.n = n - i0 < VLPET_PACK_BATCH ? n - i0 : VLPET_PACK_BATCH;
        for (int k = 0; k < b.n; ++k) {
            PackArgs& a = b.p[k];
            const int idx = i0 + k;
            for (int i = 0; i < VLPET_MAX_HEADS; ++i) {
                a.wd[i] = i < n_heads ? wd_heads_flat[(size_t)idx * n_heads + i] : nullptr;
                a.bd[i] = (bd_heads_flat && i < n_heads) ? bd_heads_flat[(size_t)idx * n_heads + i] : nullptr;
                if (i < n_heads && a.wd[i] == nullptr) return VLPET_E_NULL;
            }
            a.wu = wu[idx]; a.bu = bu ? bu[idx] : nullptr;
            if (!a.wu || !packed[idx]) return VLPET_E_NULL;
            if (!aligned16(packed[idx])) return VLPET_E_ALIGN;
            a.n_heads = n_heads; a.rows_per_head = r / n_heads;
            a.r = r; a.d = d; a.RT = tiles; a.src_bf16 = param_dtype == VLPET_BF16;
            a.n_packs = 4;
            a.out = reinterpret_cast<uint8_t*>(packed[idx]);
        }
        hipError_t e = launch_pack_pairs(b, io_dtype == VLPET_F32 ? 2 : 1, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

static int check_common(int64_t M, int d, int tiles, int io_dtype) {
    if (M <= 0 || d <= 0 || d % 64 != 0) return VLPET_E_SHAPE;
    if (!tiles_ok(tiles)) return VLPET_E_RANK;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    return 0;
}

static int gate_flags(int gate_mode, int* flags) {
    *flags = 0;
    if (gate_mode == VLPET_GATE_MUL) *flags = PET_GATE;
    else if (gate_mode == VLPET_GATE_ADD) *flags = PET_GATE | PET_GATE_ADD;
    else if (gate_mode != VLPET_GATE_NONE) return VLPET_E_SHAPE;
    return 0;
}

// the forward's saved bottleneck activations: four [M, 32*tiles] IO-dtype tensors (z_a, gelu'_a, z_g, gelu'_g)
static size_t saved_stride(int64_t M, int tiles, int io_dtype) {
    return align256((size_t)M * 32 * tiles * (io_dtype == VLPET_F32 ? 4 : 2));
}
extern "C" size_t vlpet_saved_bytes(int64_t M, int tiles, int io_dtype) {
    if (M <= 0 || !tiles_ok(tiles)) return 0;
    return 4 * saved_stride(M, tiles, io_dtype);
}

static const DropSpec NO_DROP = {nullptr, nullptr, nullptr, nullptr, 0, 0, 1.f, nullptr};

// Device step counter mixed into every dropout seed (rng.h vlpet_eff_seed): process-wide, set by the trainer that replays captured
// steps (train.Trainer(graph=True)); nullptr = seeds are used as passed.  The only state the library keeps between calls.
static std::atomic<const uint64_t*> g_seed_ctr{nullptr};
extern "C" int vlpet_set_seed_counter(const uint64_t* device_counter) {
    g_seed_ctr.store(device_counter);
    return 0;
}

// Round 6: pass 2 of the gated K1 backward (r <= 96) sums its row-chunk partials inside the launch (cols_reduce.h) -- unless the call
// sets `phases` bit 5 (32) because OTHER kernels may run beside the backward (gradient collectives on their own stream, a second
// process on the device): a workgroup that waits for partners which cannot start holds its CU for as long as the foreign kernel
// lasts, where the two-launch form simply runs in two rounds.  And only where it was measured ahead
// (profiles/r06_in_launch_reduce_ab.txt, ABBA on one box): the configs[1] step at the full
// batch (15,272-46,648 rows per call) 27.92 / 27.94 k samples/s with it against 27.73 / 27.45 k with the finalize launch, the K1
// backward op 137.5 vs 138.9 us; at the per-rank sizes of an 8-GPU run (1,900-5,800 rows, replayed graph) 5.45 / 5.47 ms per step with it
// against 5.43 / 5.43 without -- so small launches keep the finalize launch
static bool k1_in_launch_reduce(int64_t M) {
    return M >= 8192;
}

// p in [0, 1): explicit mask (keep_mask != NULL) or the in-kernel generator keyed by `seed`; p == 0: no dropout
static int make_drop(const uint8_t* keep_mask, float p, uint64_t seed, uint8_t* keep_out, DropSpec* ds) {
    if (!(p >= 0.f && p < 1.f)) return VLPET_E_SHAPE;
    *ds = NO_DROP;
    if (p == 0.f) return 0;
    ds->keep = keep_mask;
    ds->keep_out = keep_out;
    ds->seed = seed;
    ds->seed_ctr = g_seed_ctr.load();
    double t = (double)p * 65536.0 + 0.5;
    if (t > 65535.0) t = 65535.0;
    ds->thr = (uint32_t)t;
    if (ds->thr == 0 && !keep_mask) { *ds = NO_DROP; return 0; }      // p < 2^-17: the generator never drops
    ds->keep_scale = 1.0f / (1.0f - p);
    return 0;
}

static int run_fwd(const void* xa, const void* res, const void* xg, const void* pk_a, const void* pk_g,
                   const DropSpec& drop, void* out, int64_t M, int d, int tiles,
                   float s2, float sd, float gs, int flags, int io_dtype, vlpet_stream_t stream,
                   void* saved = nullptr) {
    int rc = check_common(M, d, tiles, io_dtype);
    if (rc) return rc;
    if (!xa || !res || !pk_a || !out) return VLPET_E_NULL;
    if (saved && !aligned16(saved)) return VLPET_E_ALIGN;
    if ((flags & PET_GATE) && (!xg || !pk_g)) return VLPET_E_NULL;
    if (!aligned16(xa) || !aligned16(res) || !aligned16(out) || !aligned16(pk_a) ||
        ((flags & PET_GATE) && (!aligned16(xg) || !aligned16(pk_g))) || (drop.keep && !aligned16(drop.keep)) ||
        (drop.keep_out && !aligned16(drop.keep_out)))
        return VLPET_E_ALIGN;
    PetFwdArgs a;
    a.xa = xa; a.res = res; a.xg = xg; a.out = out;
    a.pk_a = reinterpret_cast<const uint8_t*>(pk_a);
    a.pk_g = reinterpret_cast<const uint8_t*>(pk_g);
    a.drop = drop;
    // K3 training form: the packed dropout mask goes into the saved block, right after z
    if (saved && (flags & PET_ACT_IDENTITY) && drop_active(drop))
        a.drop.bits_out = reinterpret_cast<uint8_t*>(saved) + saved_stride(M, tiles, io_dtype);
    a.M = M; a.d = d; a.RT = tiles;
    a.s2 = s2; a.sd = sd; a.gs = gs; a.flags = flags;
    a.save = saved; a.save_stride = (int64_t)saved_stride(M, tiles, io_dtype);
    a.dbg = 0;
    a.dbg_ts = nullptr;
    a.d_in = 0; a.pk_a_dn = nullptr; a.pk_g_dn = nullptr; a.gm = 1.f; a.go = 0.f;
#ifdef VLPET_DEBUG      // ablation bits / cycle stamps: debug builds only (function-static device buffer, synchronises, prints)
    a.dbg = vlpet_tuning().dbg;
    if (a.dbg & 16) {     // debug only: per-phase timestamps of wave 0 of every block, printed at the next call
        static unsigned long long* dev = nullptr;
        static int nblk = 0;
        if (dev) {
            (void)hipDeviceSynchronize();
            std::vector<unsigned long long> h((size_t)nblk * 8);
            (void)hipMemcpy(h.data(), dev, h.size() * 8, hipMemcpyDeviceToHost);
            double acc[8] = {0}; int n = 0;
            for (int b = 0; b < nblk; b += 7) {
                const unsigned long long* t = &h[(size_t)b * 8];
                acc[0] += (double)(t[1] - t[0]); acc[1] += (double)(t[2] - t[1]); acc[2] += (double)(t[3] - t[2]);
                acc[3] += (double)(t[4] - t[3]); acc[4] += (double)(t[6] - t[5]); acc[5] += (double)(t[7] - t[6]);
                ++n;
            }
            fprintf(stderr, "[vlpet ts] cycles: prologue=%.0f down=%.0f act=%.0f up=%.0f | down-stage 5: issue+reads+mfma=%.0f wait+barrier=%.0f (n=%d)\n",
                    acc[0] / n, acc[1] / n, acc[2] / n, acc[3] / n, acc[4] / n, acc[5] / n, n);
        } else {
            (void)hipMalloc(&dev, 4096 * 8 * 8);
        }
        nblk = (int)((M + 127) / 128); if (nblk > 4096) nblk = 4096;
        a.dbg_ts = dev;
    }
#endif
    // training form, bf16: two passes with the weights resident in registers where that form is the faster one
    if (const int f2 = vlpet_tuning().fwd2p; f2 != 0 && k1_fwd2p_applies(a, io_dtype == VLPET_F32) && (f2 > 0 || k1_fwd2p_preferred(a)))
        return herr(launch_k1_fwd2p(a, f2 == 2 ? 1 : f2 == 3 ? 2 : 3, (hipStream_t)stream));
    if (flags & PET_GATE)      // two-chain gate forward: one wave per chain
        return herr(launch_pet_gate_fwd(a, io_dtype == VLPET_F32, (hipStream_t)stream));
    return herr(launch_pet_fwd(a, io_dtype == VLPET_F32, (hipStream_t)stream));
}

// K1 / K2 / K3 forward: one argument check per operator in front of run_fwd.  `save`: the `_save` entry point, whose block is required.
static int k1_fwd(const void* x1, const void* x2, const void* packed_a, const void* packed_g, void* out, void* saved, bool save,
                  int64_t M, int d, int tiles, int gate_mode, float delta_scale, float x2_scale, float gate_scale, int io_dtype,
                  vlpet_stream_t stream) {
    int flags;
    if (gate_flags(gate_mode, &flags)) return VLPET_E_SHAPE;
    if (save && !saved) return VLPET_E_NULL;
    return run_fwd(x2, x2, x1, packed_a, packed_g, NO_DROP, out, M, d, tiles, x2_scale, delta_scale,
                   flags ? gate_scale : 1.f, flags, io_dtype, stream, saved);
}
static int k2_fwd(const void* x, const void* y, const void* packed, void* out, void* saved, bool save, int64_t M, int d, int tiles,
                  float scale, int io_dtype, vlpet_stream_t stream) {
    if (save && !saved) return VLPET_E_NULL;
    return run_fwd(x, y, nullptr, packed, nullptr, NO_DROP, out, M, d, tiles, 1.f, scale, 1.f, 0, io_dtype, stream, saved);
}
static int k3_fwd(const void* x, const void* base, const void* packed, const uint8_t* keep_mask, float p, uint64_t seed,
                  uint8_t* keep_out, void* out, void* saved, bool save, int64_t M, int d, int tiles, float scaling, int io_dtype,
                  vlpet_stream_t stream) {
    if (save && !saved) return VLPET_E_NULL;
    DropSpec ds;
    if (int rc = make_drop(keep_mask, p, seed, keep_out, &ds)) return rc;
    return run_fwd(x, base, nullptr, packed, nullptr, ds, out, M, d, tiles, 1.f, scaling, 1.f, PET_ACT_IDENTITY, io_dtype, stream, saved);
}

extern "C" int vlpet_adapter_gate_fwd(const void* x1, const void* x2, const void* packed_a,
                                      const void* packed_g, void* out, int64_t M, int d, int tiles,
                                      int gate_mode, float delta_scale, float x2_scale, float gate_scale,
                                      int io_dtype, vlpet_stream_t stream) {
    return k1_fwd(x1, x2, packed_a, packed_g, out, nullptr, false, M, d, tiles, gate_mode, delta_scale, x2_scale, gate_scale, io_dtype, stream);
}
extern "C" int vlpet_adapter_gate_fwd_save(const void* x1, const void* x2, const void* packed_a,
                                           const void* packed_g, void* out, void* saved, int64_t M, int d, int tiles,
                                           int gate_mode, float delta_scale, float x2_scale, float gate_scale,
                                           int io_dtype, vlpet_stream_t stream) {
    return k1_fwd(x1, x2, packed_a, packed_g, out, saved, true, M, d, tiles, gate_mode, delta_scale, x2_scale, gate_scale, io_dtype, stream);
}
extern "C" int vlpet_parallel_adapter_fwd(const void* x, const void* y, const void* packed, void* out,
                                          int64_t M, int d, int tiles, float scale, int io_dtype,
                                          vlpet_stream_t stream) {
    return k2_fwd(x, y, packed, out, nullptr, false, M, d, tiles, scale, io_dtype, stream);
}
extern "C" int vlpet_parallel_adapter_fwd_save(const void* x, const void* y, const void* packed, void* out, void* saved,
                                               int64_t M, int d, int tiles, float scale, int io_dtype,
                                               vlpet_stream_t stream) {
    return k2_fwd(x, y, packed, out, saved, true, M, d, tiles, scale, io_dtype, stream);
}
extern "C" int vlpet_lora_delta_fwd(const void* x, const void* base, const void* packed,
                                    const uint8_t* keep_mask, float p, uint64_t seed, uint8_t* keep_out, void* out,
                                    int64_t M, int d, int tiles, float scaling, int io_dtype, vlpet_stream_t stream) {
    return k3_fwd(x, base, packed, keep_mask, p, seed, keep_out, out, nullptr, false, M, d, tiles, scaling, io_dtype, stream);
}
extern "C" int vlpet_lora_delta_fwd_save(const void* x, const void* base, const void* packed,
                                         const uint8_t* keep_mask, float p, uint64_t seed, uint8_t* keep_out, void* out,
                                         void* saved, int64_t M, int d, int tiles, float scaling, int io_dtype,
                                         vlpet_stream_t stream) {
    return k3_fwd(x, base, packed, keep_mask, p, seed, keep_out, out, saved, true, M, d, tiles, scaling, io_dtype, stream);
}

extern "C" size_t vlpet_lora_saved_bytes(int64_t M, int d, int tiles, int io_dtype) {
    if (M <= 0 || d <= 0 || !tiles_ok(tiles)) return 0;
    return saved_stride(M, tiles, io_dtype) + align256((size_t)M * (d / 8));      // z, then 1 bit per element of the mask
}

// K3 at rank <= 8: the streaming form (lora8.hip).  `saved` NULL = inference form; else the training form's saved block
// (vlpet_lora_saved_bytes(M, d, 1, io): z, then the packed mask) exactly as vlpet_lora_delta_fwd_save leaves it.
extern "C" int vlpet_lora_delta_fwd_r8(const void* x, const void* base, const void* packed, const uint8_t* keep_mask, float p,
                                       uint64_t seed, uint8_t* keep_out, void* out, void* saved, int64_t M, int d, int r,
                                       float scaling, int io_dtype, vlpet_stream_t stream) {
    int rc = check_common(M, d, 1, io_dtype);
    if (rc) return rc;
    if (!x || !base || !packed || !out) return VLPET_E_NULL;
    if (!lora8_applies(M, d, r, io_dtype == VLPET_F32)) return VLPET_E_SHAPE;
    if (!aligned16(x) || !aligned16(base) || !aligned16(out) || !aligned16(packed) || (saved && !aligned16(saved)) ||
        (keep_mask && !aligned16(keep_mask)) || (keep_out && !aligned16(keep_out)))
        return VLPET_E_ALIGN;
    Lora8Args a{};
    if (int rd = make_drop(keep_mask, p, seed, keep_out, &a.drop)) return rd;
    if (saved && drop_active(a.drop)) a.drop.bits_out = reinterpret_cast<uint8_t*>(saved) + saved_stride(M, 1, io_dtype);
    a.x = x; a.base = base; a.out = out; a.pk = reinterpret_cast<const uint8_t*>(packed);
    a.save = saved; a.M = M; a.d = d; a.scaling = scaling;
    return herr(launch_lora8_fwd(a, (hipStream_t)stream));
}
extern "C" int vlpet_lora_r8_applies(int64_t M, int d, int r, int io_dtype) {
    return lora8_applies(M, d, r, io_dtype == VLPET_F32) ? 1 : 0;
}

// ------------------------------------------------------------------ backward workspace
struct BwdWs {
    size_t z_a, dp_a, z_g, dp_g, dh, dq, partial, red_ctrl, total;     // red_ctrl: control words of the in-launch reduce-scatter (cols_reduce.h)
    int row_chunks;
    int64_t rows_per_chunk;
};
// The feature-split pass 1 (pet_dz2.hip, pet_dz6.hip: small M) parks its fp32 partial dz, [nfb][M][2][32 * tiles], in the dh / dq area,
// which the two-pass form does not use.  The split is on (the return value: PetBwdArgs::fsplit) where there is more than one block and
// the partials fit the `room` the kernel's own rule allows them; silently off otherwise.
static size_t dz_part_bytes(int nfb, int64_t M, int tiles) { return (size_t)nfb * (size_t)M * 2 * 32 * tiles * 4; }
static int dz_fsplit(int nfb, int64_t M, int tiles, size_t room) { return nfb > 1 && dz_part_bytes(nfb, M, tiles) <= room ? nfb : 0; }

static BwdWs bwd_ws(int64_t M, int d, int tiles, bool gate, int io_dtype) {
    BwdWs w{};
    const size_t esz = io_dtype == VLPET_F32 ? 4 : 2;
    const size_t side = align256((size_t)M * 32 * tiles * esz);
    size_t wide = align256((size_t)M * d * esz);
    // six tiles: the feature blocks of pet_dz6.hip may need more than the two wide tensors have -- half of the partials in each
    if (gate && tiles == 6 && io_dtype != VLPET_F32 && k1_dz6_feature_blocks(M, d) > 1)
        wide = std::max(wide, align256(dz_part_bytes(k1_dz6_feature_blocks(M, d), M, tiles) / 2));
    size_t o = 0;
    w.z_a = o; o += side;
    w.dp_a = o; o += side;
    if (gate) {
        w.z_g = o; o += side;
        w.dp_g = o; o += side;
        w.dh = o; o += wide;
        w.dq = o; o += wide;
    }
    const int njobs = gate ? 4 : 2;
    wgrad_plan(M, njobs, d, &w.row_chunks, &w.rows_per_chunk);
    int chunks = w.row_chunks;
    if (!gate && d % 128 == 0) {                        // the two-pass form without a gate (pet_cols_ng.hip) cuts the rows its own way
        int rcn; int64_t rpcn;
        ng_cols_plan(M, d, &rcn, &rpcn);
        if (rcn > chunks) chunks = rcn;
    }
    if (gate) {     // the two-pass gated backward (pet_gate_bwd3.hip) cuts the rows differently: room for either plan
        int rc3, gs3, ng3; int64_t rpc3;
        gate_bwd3_plan(M, d, io_dtype == VLPET_F32, &rc3, &rpc3, &gs3, &ng3);
        if (rc3 > chunks) chunks = rc3;
        int rc4; int64_t rpc4;                          // ... and the column-parallel pass of pet_cols.hip
        k1_cols_plan(M, d, &rc4, &rpc4);
        if (rc4 > chunks) chunks = rc4;
        k1_cols6_plan(M, d, &rc4, &rpc4);
        if (rc4 > chunks) chunks = rc4;
    }
    w.partial = o;
    o += align256(wgrad_workspace_bytes(njobs, tiles, d, chunks));
    w.red_ctrl = o;
    o += align256((size_t)(d >= 128 ? d / 128 : 1) * COLS_RED_STRIDE * 4);
    w.total = o;
    return w;
}

extern "C" size_t vlpet_bwd_workspace_bytes(int64_t M, int d, int tiles, int has_gate, int io_dtype) {
    if (M <= 0 || d <= 0 || !tiles_ok(tiles)) return 0;
    return bwd_ws(M, d, tiles, has_gate != 0, io_dtype).total;
}

// ------------------------------------------------------------------ backward: what a call launches
// One row of the table in DESIGN.md section 4 (bwd_plan is its source).  `phases` still decides which of the launches a call runs.
// pass 1 / the row kernel:
//   ROWS_PET_BWD    pet_bwd.hip: the one-kernel row pass (every call the forms below do not take)
//   ROWS_GATE_BWD2  pet_gate_bwd2.hip: chain-split row kernel (gated, saved activations, r <= 96); adds dx1_in in its epilogue
//   ROWS_GATE_DZ    pet_gate_bwd3.hip pass 1: dpre only, chain-split
//   ROWS_K1_DZ2     pet_dz2.hip: the same pass, feature-split (bf16, r <= 96); zeroes pass 2's reduce state itself
//   ROWS_K1_DZ6     pet_dz6.hip: the same pass at six tiles
//   ROWS_NG         pet_cols_ng.hip pass 1 (no gate, bf16, saved activations, whole call)
enum BwdRows { ROWS_PET_BWD, ROWS_GATE_BWD2, ROWS_GATE_DZ, ROWS_K1_DZ2, ROWS_K1_DZ6, ROWS_NG };
// pass 2 / the weight gradients:
//   WG_WGRAD        wgrad.hip from the row kernel's side products (vlpet_adapter_gate_bwd_form: 0)
//   WG_GATE_COLS    pet_gate_bwd3.hip pass 2 (form 1)
//   WG_K1_COLS      pet_cols.hip + finalize launch (form 2)
//   WG_K1_COLS_RED  pet_cols.hip, row chunks summed inside the launch (cols_reduce.h; form 2, no finalize launch)
//   WG_K1_COLS6Y    pet_cols6y.hip + finalize launch (form 2)
//   WG_NG           pet_cols_ng.hip pass 2 + finalize launch
enum BwdWgrad { WG_WGRAD, WG_GATE_COLS, WG_K1_COLS, WG_K1_COLS_RED, WG_K1_COLS6Y, WG_NG };
struct BwdPlan {
    BwdRows rows;
    BwdWgrad wgrad;
    int fsplit;             // feature blocks of pass 1 (PetBwdArgs::fsplit; 0: unsplit)
    bool finalize;          // launch_wgrad_finalize follows pass 2 (`phases` bits 3 / 4 split it off)
    int add_dx1;            // 0, or the `phases` bit of the pass after which dx1_in takes a launch_add_inplace of its own (the other forms add it in a kernel)
    bool memset_red;        // the reduce state of WG_K1_COLS_RED needs a memset node: this pass 1 does not zero it
    int row_chunks; int64_t rows_per_chunk; int gs3, ng3;      // the row chunks of pass 2 (gs3, ng3: gate_bwd3_plan's groups)
};

// The only place that asks the *_applies predicates, the tuning switches and the row-chunk plans of the forms.
// Two-pass forms (pass 1: dpre only; pass 2: input gradients + weight gradients from recomputed dh / dq) unless the caller needs the
// input gradients right after phase 1 (`phases` bit 2: weight gradients on a side stream).
static BwdPlan bwd_plan(const PetBwdArgs& b, int phases, int io_dtype, const BwdWs& w) {
    const int f32 = io_dtype == VLPET_F32;
    const bool whole = !(phases & 4);
    BwdPlan p{};
    p.row_chunks = w.row_chunks; p.rows_per_chunk = w.rows_per_chunk;
    // without a gate (K2, adapter-only K1, K3 without dropout), bf16, saved activations, whole call: pass 1 (dpre) + the
    // column-parallel pass of pet_cols_ng.hip (dx and both weight gradients from one read of dy and x)
    // (the in-launch reduce-scatter of cols_reduce.h was built for this pass 2 as well and measured no gain: K2 backward 67.9 / 66.7 us
    //  with it against 66.4 / 67.1 us with the finalize launch in the configs[1] step, profiles/r06_in_launch_reduce_ab.txt -- not kept)
    if (!(b.flags & PET_GATE) && phases == 3 && ng_two_pass_applies(b, f32)) {
        p.rows = ROWS_NG; p.wgrad = WG_NG; p.finalize = true;
        ng_cols_plan(b.M, b.d, &p.row_chunks, &p.rows_per_chunk);
        return p;
    }
    // bf16: pass 1 + the column-parallel pass of pet_cols.hip / pet_cols6y.hip (input gradients + the four weight gradients from one
    // read of dy, x1, x2).  Round 6: at r <= 96 pass 2 sums its row-chunk partials inside the launch -- no finalize launch; `phases`
    // bit 5 keeps the round-3 two-launch form where other kernels may run beside the call (k1_in_launch_reduce; bit-identical results)
    if (whole && k1_cols6_applies(b, f32)) {
        p.wgrad = WG_K1_COLS6Y;
        k1_cols6_plan(b.M, b.d, &p.row_chunks, &p.rows_per_chunk);
    } else if (whole && k1_cols_applies(b, f32)) {
        p.wgrad = !(phases & 32) && k1_in_launch_reduce(b.M) ? WG_K1_COLS_RED : WG_K1_COLS;
        k1_cols_plan(b.M, b.d, &p.row_chunks, &p.rows_per_chunk);
    } else if (whole && pet_gate_bwd3_applies(b)) {
        p.wgrad = WG_GATE_COLS;
        gate_bwd3_plan(b.M, b.d, f32, &p.row_chunks, &p.rows_per_chunk, &p.gs3, &p.ng3);
    } else {
        p.wgrad = WG_WGRAD;
        p.rows = pet_gate_bwd2_applies(b) ? ROWS_GATE_BWD2 : ROWS_PET_BWD;
        p.add_dx1 = p.rows == ROWS_PET_BWD ? 1 : 0;     // (the chain-split row kernel adds dx1_in in its epilogue)
        return p;
    }
    p.finalize = p.wgrad == WG_K1_COLS || p.wgrad == WG_K1_COLS6Y;
    p.add_dx1 = p.wgrad == WG_GATE_COLS ? 2 : 0;        // (dx1 is an output of pass 2 there; pet_cols*.hip take dx1_in themselves)
    if (k1_dz2_applies(b, f32)) {
        p.rows = ROWS_K1_DZ2;
        p.fsplit = dz_fsplit(k1_dz2_feature_blocks(b.M, b.d), b.M, b.RT, 2 * align256((size_t)b.M * b.d * (f32 ? 4 : 2)));
    } else if (vlpet_tuning().dz6 != 0 && k1_dz6_applies(b, f32)) {
        p.rows = ROWS_K1_DZ6;
        p.fsplit = dz_fsplit(k1_dz6_feature_blocks(b.M, b.d), b.M, b.RT, w.dq > w.dh ? 2 * (w.dq - w.dh) : 0);
    } else {
        p.rows = ROWS_GATE_DZ;
    }
    p.memset_red = p.wgrad == WG_K1_COLS_RED && p.rows != ROWS_K1_DZ2;
    return p;
}

// pass 2 of pet_cols.hip / pet_cols6y.hip; b.red_ctrl set: the row chunks are summed inside the launch
static ColzArgs colz_args(const PetBwdArgs& b, const WgradArgs& g, const void* dx1_in) {
    ColzArgs c{};
    c.dy = b.dy; c.x1 = b.xg; c.x2 = b.res; c.dxin = dx1_in; c.y = b.y;
    c.z_a = b.z_a; c.z_g = b.z_g; c.dp_a = b.dp_a; c.dp_g = b.dp_g;
    c.dx1 = b.dxg; c.dx2 = b.dxa;
    c.pk_a = b.pk_a; c.pk_g = b.pk_g;
    c.M = b.M; c.d = b.d; c.s2 = b.s2; c.sd = b.sd; c.gs = b.gs; c.flags = b.flags;
    c.row_chunks = g.row_chunks; c.rows_per_chunk = g.rows_per_chunk;
    const WgradLayout L = wgrad_layout(g);
    for (int j = 0; j < 4; ++j) c.part[j] = g.partial + L.off[j];
    if (b.red_ctrl) {
        // the same workspace bytes, cut differently: [RC][NCB] slabs (= the four [RC][PR][d] blocks), then the column-sum partials
        const int64_t PRl = 32 * b.RT;
        c.red.slab = g.partial;
        c.red.bias_x = g.partial + (int64_t)4 * g.row_chunks * PRl * b.d;
        c.red.bias_p = c.red.bias_x + (int64_t)2 * g.row_chunks * b.d;
        c.red.ctrl = b.red_ctrl;
        c.red.spin_limit = COLS_RED_SPIN_DEFAULT;
        for (int j = 0; j < 4; ++j) {
            const WgradJob& J = g.job[j];
            c.red.job[j] = ColsRedJob{J.out, J.ldo, J.transposed, J.out_rows, J.scale, J.colsum_x, J.colsum_p};
        }
    }
    return c;
}

// Four steps: argument checks, PetBwdArgs, bwd_plan, the launches of the plan that `phases` asks for.
static int run_bwd(const void* dy, const void* xa, const void* res, const void* xg,
                   const void* pk_a, const void* pk_g, const DropSpec& drop,
                   void* dxa, void* dxg,
                   float* dwd, float* dbd, float* dwu, float* dbu,
                   float* dwgd, float* dbgd, float* dwgu, float* dbgu, int r, int rg,
                   void* workspace, size_t workspace_bytes, int64_t M, int d, int tiles,
                   float s2, float sd, float gs, int flags, int io_dtype, vlpet_stream_t stream,
                   int phases = 3 /* bit0: row-parallel kernel, bit1: weight gradients; bit3: skip the finalize of bit1, bit4: finalize only, bit5: no in-launch reduce */,
                   const void* saved = nullptr /* vlpet_adapter_gate_fwd_save's block */,
                   const void* dx1_in = nullptr /* gated K1: added to dxg (must not alias it) */,
                   const void* yout = nullptr /* gated K1: the forward's output (PetBwdArgs::y) */) {
    int rc = check_common(M, d, tiles, io_dtype);
    if (rc) return rc;
    const bool gate = flags & PET_GATE;
    if (!dy || !xa || !pk_a || !dxa || !dwd || !dwu || !workspace) return VLPET_E_NULL;
    if (gate && (!res || !xg || !pk_g || !dxg || !dwgd || !dwgu || !dbgd || !dbgu)) return VLPET_E_NULL;
    if (r <= 0 || r > 32 * tiles || (gate && (rg <= 0 || rg > 32 * tiles))) return VLPET_E_RANK;
    if (!aligned16(dy) || !aligned16(xa) || !aligned16(dxa) || !aligned16(workspace) || !aligned16(pk_a) ||
        (gate && (!aligned16(xg) || !aligned16(res) || !aligned16(dxg) || !aligned16(pk_g))) ||
        (drop.keep && !aligned16(drop.keep)))
        return VLPET_E_ALIGN;
    const BwdWs w = bwd_ws(M, d, tiles, gate, io_dtype);
    if (workspace_bytes < w.total) return VLPET_E_WORKSPACE;
    if (dx1_in && (!gate || !aligned16(dx1_in) || dx1_in == dxg)) return VLPET_E_ALIGN;
    if (yout && (!gate || !saved || !aligned16(yout))) return VLPET_E_ALIGN;
    if (saved && !aligned16(saved)) return VLPET_E_ALIGN;
    uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
    const int f32 = io_dtype == VLPET_F32;
    const hipStream_t st = (hipStream_t)stream;

    PetBwdArgs b;
    b.dy = dy; b.xa = xa; b.res = res; b.xg = xg;
    b.dxa = dxa; b.dxg = dxg; b.dxg_in = nullptr;
    b.z_a = ws + w.z_a; b.dp_a = ws + w.dp_a;
    b.z_g = gate ? ws + w.z_g : nullptr; b.dp_g = gate ? ws + w.dp_g : nullptr;
    b.dh = gate ? ws + w.dh : nullptr; b.dq = gate ? ws + w.dq : nullptr;
    b.pk_a = reinterpret_cast<const uint8_t*>(pk_a);
    b.pk_g = reinterpret_cast<const uint8_t*>(pk_g);
    b.drop = drop; b.drop.keep_out = nullptr; b.drop.bits_out = nullptr;
    if (saved && (flags & PET_ACT_IDENTITY) && drop_active(drop)) {        // the forward's packed mask instead of regenerating it
        b.drop.bits = reinterpret_cast<const uint8_t*>(saved) + saved_stride(M, tiles, io_dtype);
        b.drop.keep = nullptr;
    }
    b.M = M; b.d = d; b.RT = tiles;
    b.s2 = s2; b.sd = sd; b.gs = gs; b.flags = flags;
    b.gm = 1.f; b.go = 0.f; b.fsplit = 0; b.dz_part = nullptr;
    b.y = (flags & PET_GATE_ADD) ? nullptr : yout;
    b.red_ctrl = nullptr; b.red_words = 0;
    b.saved = saved; b.saved_stride = (int64_t)saved_stride(M, tiles, io_dtype);
    if (saved) {        // z comes from the forward; the rows kernel does not write it
        b.z_a = const_cast<uint8_t*>(reinterpret_cast<const uint8_t*>(saved));
        if (gate) b.z_g = const_cast<uint8_t*>(reinterpret_cast<const uint8_t*>(saved)) + 2 * b.saved_stride;
    }

    const BwdPlan p = bwd_plan(b, phases, io_dtype, w);
    if (p.rows == ROWS_GATE_BWD2) b.dxg_in = dx1_in;
    if (p.fsplit) { b.fsplit = p.fsplit; b.dz_part = reinterpret_cast<float*>(ws + w.dh); }
    if (p.wgrad == WG_K1_COLS_RED) { b.red_ctrl = reinterpret_cast<unsigned*>(ws + w.red_ctrl); b.red_words = (d / 128) * COLS_RED_STRIDE; }
    WgradArgs g{};
    g.M = M; g.RT = tiles; g.row_chunks = p.row_chunks; g.rows_per_chunk = p.rows_per_chunk;
    g.partial = reinterpret_cast<float*>(ws + w.partial);
    const int ldp = 32 * tiles;
    auto job = [&](int i, const void* P, const void* X, bool dropped, float scale, float* out, int ldo,
                   int transposed, int out_rows, float* csx, float* csp) {
        WgradJob& J = g.job[i];
        J.P = P; J.ldp = ldp; J.pcols = ldp;
        J.X = X; J.ldx = d; J.xcols = d;
        J.drop = dropped ? b.drop : NO_DROP; J.has_drop = dropped && drop_active(b.drop);
        J.scale = scale; J.out = out; J.ldo = ldo; J.transposed = transposed; J.out_rows = out_rows;
        J.colsum_x = csx; J.colsum_p = csp;
    };
    // down weight:  dWd[c,k] = sum_m dpre[m,c] * xa[m,k];  bias = column sums of dpre
    // (dropout: wgrad.hip applies the mask to xa; pet_cols_ng.hip clears the dropped x itself and leaves 1 / (1 - p) to the scale)
    const bool ng = p.wgrad == WG_NG;
    job(0, b.dp_a, xa, !ng, ng && drop_active(b.drop) ? b.drop.keep_scale : 1.f, dwd, d, 0, r, nullptr, dbd);
    // up weight:    dWu[f,c] = sd * sum_m dh[m,f] * z[m,c]  (X = dh, or dy itself without a gate)
    job(1, b.z_a, gate ? b.dh : dy, false, sd, dwu, r, 1, r, dbu, nullptr);
    g.njobs = 2;
    if (gate) {
        job(2, b.dp_g, xg, false, 1.f, dwgd, d, 0, rg, nullptr, dbgd);
        job(3, b.z_g, b.dq, false, 1.f, dwgu, rg, 1, rg, dbgu, nullptr);
        g.njobs = 4;
    }
    auto add_dx1 = [&](int after) {     // the forms whose kernels do not take dx1_in: one more pass over dx1
        if (!dx1_in || p.add_dx1 != after) return hipSuccess;
        return launch_add_inplace(dxg, dx1_in, M * (int64_t)d, f32, st);
    };

    hipError_t e = hipSuccess;
    if (phases & 1) {
        if (p.memset_red) e = hipMemsetAsync(b.red_ctrl, 0, (size_t)b.red_words * 4, st);
        if (e != hipSuccess) return (int)e;
        switch (p.rows) {
            case ROWS_PET_BWD:   e = launch_pet_bwd(b, f32, st); break;
            case ROWS_GATE_BWD2: e = launch_pet_gate_bwd2(b, f32, st); break;
            case ROWS_GATE_DZ:   e = launch_pet_gate_dz(b, f32, st); break;
            case ROWS_K1_DZ2:    e = launch_k1_dz2(b, st); break;
            case ROWS_K1_DZ6:    e = launch_k1_dz6(b, st); break;
            case ROWS_NG:        e = launch_ng_two_pass(b, g, 1, st); break;
        }
        if (e == hipSuccess) e = add_dx1(1);
        if (e != hipSuccess) return (int)e;
    }
    if (phases & 2) {
        switch (p.wgrad) {
            case WG_WGRAD:       e = launch_wgrad(g, f32, st); break;
            case WG_GATE_COLS:   e = launch_pet_gate_cols(b, g, p.gs3, p.ng3, f32, st); break;
            case WG_K1_COLS:
            case WG_K1_COLS_RED: e = launch_k1_cols(colz_args(b, g, dx1_in), tiles, st); break;
            case WG_K1_COLS6Y:   e = launch_k1_cols6y(colz_args(b, g, dx1_in), st); break;
            case WG_NG:          e = launch_ng_two_pass(b, g, 2, st); break;
        }
        if (e == hipSuccess) e = add_dx1(2);
        if (e != hipSuccess) return (int)e;
    }
    // bit 3 without bit 4 leaves the partial sums in the workspace; bit 4 alone ("finalize only") sums them
    if (p.finalize && (phases & (2 | 16)) && (!(phases & 8) || (phases & 16))) e = launch_wgrad_finalize(g, st);
    return herr(e);
}

// The plan of the default gated call at a shape: the forward's block and its output handed over, the whole call, no `phases` bit 5
static BwdPlan gate_bwd_plan_at(int64_t M, int d, int tiles, int io_dtype) {
    PetBwdArgs b{};
    b.M = M; b.d = d; b.RT = tiles; b.flags = PET_GATE; b.saved = &b; b.drop = NO_DROP; b.y = &b;
    return bwd_plan(b, 3, io_dtype, bwd_ws(M, d, tiles, true, io_dtype));
}

// 2: pass 1 + the column-parallel pass of pet_cols.hip / pet_cols6y.hip; 1: the two passes of pet_gate_bwd3.hip; 0: row kernel + wgrad.hip
extern "C" int vlpet_adapter_gate_bwd_form(int64_t M, int d, int tiles, int io_dtype) {
    if (check_common(M, d, tiles, io_dtype)) return -1;
    const BwdWgrad wg = gate_bwd_plan_at(M, d, tiles, io_dtype).wgrad;
    return wg == WG_WGRAD ? 0 : wg == WG_GATE_COLS ? 1 : 2;
}

// For a call without `phases` bit 5 -- 1: the two-pass form at this shape ends in a separate finalize launch (`phases` bit 4 runs
// it); 0: pass 2 sums its row chunks itself (round 6, cols_reduce.h) or the form is not the two-pass one
extern "C" int vlpet_adapter_gate_bwd_finalize_launch(int64_t M, int d, int tiles, int io_dtype) {
    if (check_common(M, d, tiles, io_dtype)) return -1;
    return gate_bwd_plan_at(M, d, tiles, io_dtype).finalize ? 1 : 0;
}

// K1 / K2 / K3 backward: one argument check per operator in front of run_bwd.
// The five K1 variants differ in what they require (the forward's block, dx1_in, a gate), in the `phases` bits they pass on (`mask`) and
// in those of which one must be set (`any`); `y`, and `dx1_in` where it is not required, may be NULL.
struct K1BwdForm { bool saved, dx1_in, gate; int mask, any; };
static int k1_bwd(const K1BwdForm& f, int phases, const void* dy, const void* x1, const void* x2, const void* y, const void* saved,
                  const void* packed_a, const void* packed_g, const void* dx1_in, void* dx1, void* dx2,
                  float* dwd, float* dbd, float* dwu, float* dbu,
                  float* dwgd, float* dbgd, float* dwgu, float* dbgu, int r, int rg,
                  void* workspace, size_t workspace_bytes, int64_t M, int d, int tiles,
                  int gate_mode, float delta_scale, float x2_scale, float gate_scale,
                  int io_dtype, vlpet_stream_t stream) {
    int flags;
    if (gate_flags(gate_mode, &flags)) return VLPET_E_SHAPE;
    if (!dbd || !dbu || (f.saved && !saved) || (f.dx1_in && !dx1_in) || (f.gate && !flags) || (phases & f.any) == 0) return VLPET_E_NULL;
    return run_bwd(dy, x2, x2, x1, packed_a, packed_g, NO_DROP, dx2, dx1, dwd, dbd, dwu, dbu,
                   dwgd, dbgd, dwgu, dbgu, r, rg, workspace, workspace_bytes, M, d, tiles,
                   x2_scale, delta_scale, flags ? gate_scale : 1.f, flags, io_dtype, stream, phases & f.mask, saved, dx1_in, y);
}
// (`need_saved`: the `_saved` entry point, whose block is required)
static int k2_bwd(const void* dy, const void* x, const void* saved, bool need_saved, const void* packed, void* dx,
                  float* dwd, float* dbd, float* dwu, float* dbu, int r, void* workspace, size_t workspace_bytes, int64_t M, int d,
                  int tiles, float scale, int io_dtype, vlpet_stream_t stream) {
    if (!dbd || !dbu || (need_saved && !saved)) return VLPET_E_NULL;
    return run_bwd(dy, x, nullptr, nullptr, packed, nullptr, NO_DROP, dx, nullptr, dwd, dbd, dwu, dbu,
                   nullptr, nullptr, nullptr, nullptr, r, 0, workspace, workspace_bytes, M, d, tiles,
                   1.f, scale, 1.f, 0, io_dtype, stream, 3, saved);
}
static int k3_bwd(const void* dy, const void* x, const void* saved, bool need_saved, const void* packed, const uint8_t* keep_mask,
                  float p, uint64_t seed, void* dx, float* da, float* db, int r, void* workspace, size_t workspace_bytes,
                  int64_t M, int d, int tiles, float scaling, int io_dtype, vlpet_stream_t stream) {
    if (need_saved && !saved) return VLPET_E_NULL;
    DropSpec ds;
    if (int rc = make_drop(keep_mask, p, seed, nullptr, &ds)) return rc;
    return run_bwd(dy, x, nullptr, nullptr, packed, nullptr, ds, dx, nullptr,
                   da, nullptr, db, nullptr, nullptr, nullptr, nullptr, nullptr, r, 0,
                   workspace, workspace_bytes, M, d, tiles, 1.f, scaling, 1.f, PET_ACT_IDENTITY,
                   io_dtype, stream, 3, saved);
}

extern "C" int vlpet_adapter_gate_bwd(const void* dy, const void* x1, const void* x2,
                                      const void* packed_a, const void* packed_g, void* dx1, void* dx2,
                                      float* dwd, float* dbd, float* dwu, float* dbu,
                                      float* dwgd, float* dbgd, float* dwgu, float* dbgu, int r, int rg,
                                      void* workspace, size_t workspace_bytes, int64_t M, int d, int tiles,
                                      int gate_mode, float delta_scale, float x2_scale, float gate_scale,
                                      int io_dtype, vlpet_stream_t stream) {
    return k1_bwd({false, false, false, 7, 3}, 3, dy, x1, x2, nullptr, nullptr, packed_a, packed_g, nullptr, dx1, dx2, dwd, dbd, dwu, dbu, dwgd, dbgd, dwgu, dbgu, r, rg,
                  workspace, workspace_bytes, M, d, tiles, gate_mode, delta_scale, x2_scale, gate_scale, io_dtype, stream);
}
extern "C" int vlpet_adapter_gate_bwd_phase(int phases, const void* dy, const void* x1, const void* x2,
                                            const void* packed_a, const void* packed_g, void* dx1, void* dx2,
                                            float* dwd, float* dbd, float* dwu, float* dbu,
                                            float* dwgd, float* dbgd, float* dwgu, float* dbgu, int r, int rg,
                                            void* workspace, size_t workspace_bytes, int64_t M, int d, int tiles,
                                            int gate_mode, float delta_scale, float x2_scale, float gate_scale,
                                            int io_dtype, vlpet_stream_t stream) {
    return k1_bwd({false, false, false, 7, 3}, phases, dy, x1, x2, nullptr, nullptr, packed_a, packed_g, nullptr, dx1, dx2, dwd, dbd, dwu, dbu, dwgd, dbgd, dwgu, dbgu, r, rg,
                  workspace, workspace_bytes, M, d, tiles, gate_mode, delta_scale, x2_scale, gate_scale, io_dtype, stream);
}
extern "C" int vlpet_adapter_gate_bwd_saved(int phases, const void* dy, const void* x1, const void* x2, const void* saved,
                                            const void* packed_a, const void* packed_g, void* dx1, void* dx2,
                                            float* dwd, float* dbd, float* dwu, float* dbu,
                                            float* dwgd, float* dbgd, float* dwgu, float* dbgu, int r, int rg,
                                            void* workspace, size_t workspace_bytes, int64_t M, int d, int tiles,
                                            int gate_mode, float delta_scale, float x2_scale, float gate_scale,
                                            int io_dtype, vlpet_stream_t stream) {
    return k1_bwd({true, false, false, 63, 19}, phases, dy, x1, x2, nullptr, saved, packed_a, packed_g, nullptr, dx1, dx2, dwd, dbd, dwu, dbu, dwgd, dbgd, dwgu, dbgu, r, rg,
                  workspace, workspace_bytes, M, d, tiles, gate_mode, delta_scale, x2_scale, gate_scale, io_dtype, stream);
}
extern "C" int vlpet_adapter_gate_bwd_saved_acc(int phases, const void* dy, const void* x1, const void* x2, const void* saved,
                                                const void* packed_a, const void* packed_g, const void* dx1_in, void* dx1, void* dx2,
                                                float* dwd, float* dbd, float* dwu, float* dbu,
                                                float* dwgd, float* dbgd, float* dwgu, float* dbgu, int r, int rg,
                                                void* workspace, size_t workspace_bytes, int64_t M, int d, int tiles,
                                                int gate_mode, float delta_scale, float x2_scale, float gate_scale,
                                                int io_dtype, vlpet_stream_t stream) {
    return k1_bwd({true, true, true, 63, 19}, phases, dy, x1, x2, nullptr, saved, packed_a, packed_g, dx1_in, dx1, dx2, dwd, dbd, dwu, dbu, dwgd, dbgd, dwgu, dbgu, r, rg,
                  workspace, workspace_bytes, M, d, tiles, gate_mode, delta_scale, x2_scale, gate_scale, io_dtype, stream);
}
// The same with the forward's output y at hand (round 5): pass 1 of the two-pass forms then needs the gate chain's up projection
// only (dq = dy * y * (1 - g)); dx1_in is optional here.  y == NULL: exactly vlpet_adapter_gate_bwd_saved / _acc.
extern "C" int vlpet_adapter_gate_bwd_saved_y(int phases, const void* dy, const void* x1, const void* x2, const void* y, const void* saved,
                                              const void* packed_a, const void* packed_g, const void* dx1_in, void* dx1, void* dx2,
                                              float* dwd, float* dbd, float* dwu, float* dbu,
                                              float* dwgd, float* dbgd, float* dwgu, float* dbgu, int r, int rg,
                                              void* workspace, size_t workspace_bytes, int64_t M, int d, int tiles,
                                              int gate_mode, float delta_scale, float x2_scale, float gate_scale,
                                              int io_dtype, vlpet_stream_t stream) {
    return k1_bwd({true, false, true, 63, 19}, phases, dy, x1, x2, y, saved, packed_a, packed_g, dx1_in, dx1, dx2, dwd, dbd, dwu, dbu, dwgd, dbgd, dwgu, dbgu, r, rg,
                  workspace, workspace_bytes, M, d, tiles, gate_mode, delta_scale, x2_scale, gate_scale, io_dtype, stream);
}

extern "C" int vlpet_parallel_adapter_bwd(const void* dy, const void* x, const void* packed, void* dx,
                                          float* dwd, float* dbd, float* dwu, float* dbu, int r,
                                          void* workspace, size_t workspace_bytes, int64_t M, int d,
                                          int tiles, float scale, int io_dtype, vlpet_stream_t stream) {
    return k2_bwd(dy, x, nullptr, false, packed, dx, dwd, dbd, dwu, dbu, r, workspace, workspace_bytes, M, d, tiles, scale, io_dtype, stream);
}
extern "C" int vlpet_parallel_adapter_bwd_saved(const void* dy, const void* x, const void* saved, const void* packed, void* dx,
                                                float* dwd, float* dbd, float* dwu, float* dbu, int r,
                                                void* workspace, size_t workspace_bytes, int64_t M, int d,
                                                int tiles, float scale, int io_dtype, vlpet_stream_t stream) {
    return k2_bwd(dy, x, saved, true, packed, dx, dwd, dbd, dwu, dbu, r, workspace, workspace_bytes, M, d, tiles, scale, io_dtype, stream);
}
extern "C" int vlpet_lora_delta_bwd(const void* dy, const void* x, const void* packed,
                                    const uint8_t* keep_mask, float p, uint64_t seed, void* dx,
                                    float* da, float* db, int r, void* workspace, size_t workspace_bytes,
                                    int64_t M, int d, int tiles, float scaling, int io_dtype,
                                    vlpet_stream_t stream) {
    return k3_bwd(dy, x, nullptr, false, packed, keep_mask, p, seed, dx, da, db, r, workspace, workspace_bytes, M, d, tiles, scaling, io_dtype, stream);
}
extern "C" int vlpet_lora_delta_bwd_saved(const void* dy, const void* x, const void* saved, const void* packed,
                                          const uint8_t* keep_mask, float p, uint64_t seed, void* dx,
                                          float* da, float* db, int r, void* workspace, size_t workspace_bytes,
                                          int64_t M, int d, int tiles, float scaling, int io_dtype,
                                          vlpet_stream_t stream) {
    return k3_bwd(dy, x, saved, true, packed, keep_mask, p, seed, dx, da, db, r, workspace, workspace_bytes, M, d, tiles, scaling, io_dtype, stream);
}

// ------------------------------------------------------------------ K4: visual projection
static inline bool dout_ok(int d) { return d == 64 || d == 128 || d == 768; }

extern "C" size_t vlpet_visproj_packed_bytes(int d_out, int feat_dim, int io_dtype) {
    const int NS = io_dtype == VLPET_F32 ? 2 : 1;
    return align256((size_t)(feat_dim / 16) * (d_out / 32) * NS * 1024 + (size_t)(d_out + feat_dim) * 4);
}

extern "C" int vlpet_visproj_pack(const void* w, const void* b, int d_out, int feat_dim, int param_dtype,
                                  int io_dtype, void* packed, vlpet_stream_t stream) {
    if (!w || !packed) return VLPET_E_NULL;
    if (!dout_ok(d_out) || feat_dim <= 0 || feat_dim % 64 != 0) return VLPET_E_SHAPE;
    if (!dtype_ok(param_dtype) || !dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (!aligned16(packed)) return VLPET_E_ALIGN;
    PackArgs a;
    for (int i = 0; i < VLPET_MAX_HEADS; ++i) { a.wd[i] = nullptr; a.bd[i] = nullptr; }
    a.wd[0] = w; a.bd[0] = b;
    a.wu = nullptr; a.bu = nullptr;
    a.n_heads = 1; a.rows_per_head = d_out;
    a.r = d_out; a.d = feat_dim; a.RT = d_out / 32; a.src_bf16 = param_dtype == VLPET_BF16;
    a.n_packs = 1;
    a.out = reinterpret_cast<uint8_t*>(packed);
    return herr(launch_pack_pair(a, io_dtype == VLPET_F32 ? 2 : 1, (hipStream_t)stream));
}

extern "C" int vlpet_visproj_fwd(const void* feats, const void* packed, const float* gamma, const float* beta,
                                 const void* r, void* out, void* xhat, float* rstd, int64_t M, int feat_dim,
                                 int d_out, float eps, int rms, int io_dtype, vlpet_stream_t stream) {
    if (!feats || !packed || !gamma || !out) return VLPET_E_NULL;
    if (M <= 0 || !dout_ok(d_out) || feat_dim <= 0 || feat_dim % 64 != 0) return VLPET_E_SHAPE;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (!aligned16(feats) || !aligned16(packed) || !aligned16(out) || (r && !aligned16(r)) || (xhat && !aligned16(xhat)))
        return VLPET_E_ALIGN;
    VisprojArgs a;
    a.feats = feats; a.pk = reinterpret_cast<const uint8_t*>(packed); a.gamma = gamma; a.beta = beta;
    a.R = r; a.out = out; a.xhat = xhat; a.rstd = rstd;
    a.M = M; a.F = feat_dim; a.d_out = d_out; a.eps = eps; a.rms = rms;
    return herr(launch_visproj_fwd(a, io_dtype == VLPET_F32, (hipStream_t)stream));
}

// K4 forward as a tiled GEMM (visproj_gemm.hip): bf16, d_out a multiple of 256 (<= 1024), feat_dim a multiple of 64.
extern "C" size_t vlpet_visproj_gemm_workspace_bytes(int64_t M, int feat_dim, int d_out) {
    return visproj_gemm_workspace_bytes(M, feat_dim, d_out);
}
// out = the sum of n tensors of `len` IO-dtype elements (n >= 1 sources as an array of device pointers on the HOST; out may be srcs[0]):
// fp32 accumulation, one rounding per launch of up to eight sources
extern "C" int vlpet_sum_n(const void* const* srcs, int n, void* out, int64_t len, int io_dtype, vlpet_stream_t stream) {
    if (!srcs || !out) return VLPET_E_NULL;
    if (n < 1 || len <= 0 || len % 8 != 0) return VLPET_E_SHAPE;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (!aligned16(out)) return VLPET_E_ALIGN;
    for (int i = 0; i < n; ++i) {
        if (!srcs[i]) return VLPET_E_NULL;
        if (!aligned16(srcs[i])) return VLPET_E_ALIGN;
    }
    const size_t esz = io_dtype == VLPET_F32 ? 4 : 2;
    if (n == 1) {
        if (srcs[0] == out) return 0;
        return herr(hipMemcpyAsync(out, srcs[0], (size_t)len * esz, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    int done = 0;
    while (done < n) {                      // eight sources per launch; later launches start from the running sum
        SumNArgs a{};
        int k = 0;
        if (done > 0) a.src[k++] = out;
        while (k < 8 && done < n) a.src[k++] = srcs[done++];
        a.out = out;
        if (k == 1) break;
        hipError_t e = launch_sum_n(a, k, len, io_dtype == VLPET_F32, (hipStream_t)stream);
        if (e != hipSuccess) return herr(e);
    }
    return 0;
}

// K4's position / order branch (vispos.hip).  table dtypes: VLPET_F32 / VLPET_BF16 each; ids int64 [B or 1, N] with a batch stride of N or 0
// (nullptr: image 0 / object n, the reference's defaults, src/modeling_bart.py:169-177)
extern "C" int vlpet_vispos_applies(int d, int n_img) { return vispos_applies(d, n_img) ? 1 : 0; }
extern "C" size_t vlpet_vispos_bwd_workspace_bytes(int64_t M, int d, int n_img) {
    return (M > 0 && vispos_applies(d, n_img)) ? vispos_bwd_workspace_bytes(M, d, n_img) : 0;
}
static int vispos_common(const float* pos, const float* w, const float* b, const float* gamma, int64_t M, int N, int d, int n_img, int io_dtype) {
    if (!pos || !w || !b || !gamma) return VLPET_E_NULL;
    if (M <= 0 || M >= ((int64_t)1 << 31) || N <= 0 || M % N != 0 || !vispos_applies(d, n_img)) return VLPET_E_SHAPE;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (!aligned16(pos) || !aligned16(w) || !aligned16(b) || !aligned16(gamma)) return VLPET_E_ALIGN;
    return 0;
}
extern "C" int vlpet_vispos_fwd(const float* pos, const float* w, const float* b, const float* gamma, const float* beta,
                                const void* img_table, int img_table_dtype, int n_img, const int64_t* img_ids, int64_t img_ids_bstride,
                                const void* obj_table, int obj_table_dtype, int64_t obj_rows, const int64_t* obj_ids, int64_t obj_ids_bstride,
                                void* out, int64_t M, int N, int d, float eps, int rms, int io_dtype, vlpet_stream_t stream) {
    const bool tabs = img_table != nullptr || obj_table != nullptr;
    if (int rc = vispos_common(pos, w, b, gamma, M, N, d, tabs ? n_img : 0, io_dtype)) return rc;
    if (!out || (!rms && !beta)) return VLPET_E_NULL;
    if (tabs) {
        if (!img_table || !obj_table) return VLPET_E_NULL;              // the reference adds both or neither (use_vis_order_embedding)
        if (n_img < 1 || obj_rows < 1) return VLPET_E_SHAPE;
        if (!dtype_ok(img_table_dtype) || !dtype_ok(obj_table_dtype)) return VLPET_E_DTYPE;
        if (!aligned16(img_table) || !aligned16(obj_table)) return VLPET_E_ALIGN;
    }
    if (!aligned16(out) || (beta && !aligned16(beta))) return VLPET_E_ALIGN;
    VisPosArgs a{};
    a.pos = pos; a.w = w; a.b = b; a.gamma = gamma; a.beta = rms ? nullptr : beta;
    a.img_tab = img_table; a.obj_tab = obj_table; a.img_tab_bf16 = img_table_dtype == VLPET_BF16; a.obj_tab_bf16 = obj_table_dtype == VLPET_BF16;
    a.img_ids = img_ids; a.obj_ids = obj_ids; a.img_bstride = img_ids_bstride; a.obj_bstride = obj_ids_bstride;
    a.n_img = n_img; a.obj_rows = obj_rows; a.out = out; a.M = M; a.N = N; a.d = d; a.eps = eps; a.rms = rms;
    return herr(launch_vispos_fwd(a, io_dtype == VLPET_F32, (hipStream_t)stream));
}
// dout = the gradient of the visual embedding's output (= dR); results are WRITTEN: dw [d, 5], db [d], dgamma [d], dbeta [d] (nullptr with
// rms), dimg [n_img, d] (nullptr / n_img = 0: no image-order table)
extern "C" int vlpet_vispos_bwd(const void* dout, const float* pos, const float* w, const float* b, const float* gamma,
                                int n_img, const int64_t* img_ids, int64_t img_ids_bstride,
                                float* dw, float* db, float* dgamma, float* dbeta, float* dimg,
                                void* workspace, size_t workspace_bytes, int64_t M, int N, int d, float eps, int rms, int io_dtype,
                                vlpet_stream_t stream) {
    if (!dimg) n_img = 0;
    if (int rc = vispos_common(pos, w, b, gamma, M, N, d, n_img, io_dtype)) return rc;
    if (!dout || !dw || !db || !dgamma || !workspace || (!rms && !dbeta)) return VLPET_E_NULL;
    if (!aligned16(dout) || !aligned16(workspace)) return VLPET_E_ALIGN;
    if (workspace_bytes < vispos_bwd_workspace_bytes(M, d, n_img)) return VLPET_E_WORKSPACE;
    VisPosArgs a{};
    a.pos = pos; a.w = w; a.b = b; a.gamma = gamma;
    a.img_ids = img_ids; a.img_bstride = img_ids_bstride; a.n_img = n_img;
    a.dout = dout; a.partial = reinterpret_cast<float*>(workspace);
    a.dw = dw; a.db = db; a.dgamma = dgamma; a.dbeta = rms ? nullptr : dbeta; a.dimg = dimg;
    a.M = M; a.N = N; a.d = d; a.eps = eps; a.rms = rms;
    return herr(launch_vispos_bwd(a, io_dtype == VLPET_F32, (hipStream_t)stream));
}

extern "C" size_t vlpet_visproj_gemm_exchange_bytes(int d_out) {
    return (d_out > 0 && d_out % 256 == 0 && d_out / 256 <= 4) ? visproj_gemm_exchange_bytes(d_out) : 0;
}
static int visproj_gemm_call(const void* feats, const void* w_io, const float* bias, const float* gamma, const float* beta,
                             const void* r, void* out, void* xhat, float* rstd, float* mean, void* workspace, size_t workspace_bytes,
                             int64_t M, int feat_dim, int d_out, float eps, int rms, int io_dtype, int form, int bm, vlpet_stream_t stream) {
    if (!feats || !w_io || !gamma || !out || !workspace) return VLPET_E_NULL;
    if (!xhat && d_out > 256) return VLPET_E_NULL;       // (a workgroup that gives up on its partners parks its pre-norm tile there)
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (!visproj_gemm_applies(M, feat_dim, d_out, io_dtype == VLPET_F32)) return VLPET_E_SHAPE;
    if (workspace_bytes < visproj_gemm_workspace_bytes(M, feat_dim, d_out)) return VLPET_E_WORKSPACE;
    if (!aligned16(feats) || !aligned16(w_io) || !aligned16(out) || (r && !aligned16(r)) || (xhat && !aligned16(xhat)) || !aligned16(workspace))
        return VLPET_E_ALIGN;
    VisGemmArgs a{};
    a.feats = feats; a.w = w_io; a.bias = bias; a.gamma = gamma; a.beta = beta; a.R = r; a.out = out; a.xhat = xhat; a.rstd = rstd;
    a.mean = mean; a.M = M; a.F = feat_dim; a.d_out = d_out; a.eps = eps; a.rms = rms;
    return herr(launch_visproj_gemm(a, workspace, form, bm, (hipStream_t)stream));
}
extern "C" int vlpet_visproj_fwd_gemm(const void* feats, const void* w_io, const float* bias, const float* gamma, const float* beta,
                                      const void* r, void* out, void* xhat, float* rstd, float* mean, void* workspace,
                                      size_t workspace_bytes, int64_t M, int feat_dim, int d_out, float eps, int rms, int io_dtype,
                                      vlpet_stream_t stream) {
    return visproj_gemm_call(feats, w_io, bias, gamma, beta, r, out, xhat, rstd, mean, workspace, workspace_bytes, M, feat_dim, d_out,
                             eps, rms, io_dtype, 0, 0, stream);
}
// the same with the ring form (1: BK 64 / 2 slots, 2: BK 32 / 4 slots, 3: BK 32 / 3 slots; 0: default) and the rows per workgroup
// (128 / 256; 0: by shape) forced -- tools/k4bench.py and the parity tests of the non-default forms
extern "C" int vlpet_visproj_fwd_gemm_cfg(const void* feats, const void* w_io, const float* bias, const float* gamma, const float* beta,
                                          const void* r, void* out, void* xhat, float* rstd, float* mean, void* workspace,
                                          size_t workspace_bytes, int64_t M, int feat_dim, int d_out, float eps, int rms, int io_dtype,
                                          int form, int rows_per_workgroup, vlpet_stream_t stream) {
    if (form < 0 || (form & 255) > 6 || (form >> 8) > 31 || (rows_per_workgroup != 0 && rows_per_workgroup != 128 && rows_per_workgroup != 192 && rows_per_workgroup != 256)) return VLPET_E_SHAPE;
    return visproj_gemm_call(feats, w_io, bias, gamma, beta, r, out, xhat, rstd, mean, workspace, workspace_bytes, M, feat_dim, d_out,
                             eps, rms, io_dtype, form, rows_per_workgroup, stream);
}

static void visproj_wgrad_plan(int64_t M, int feat_dim, int d_out, int* RT, int* pcols, int* rc, int64_t* rpc) {
    *RT = (d_out % 96 == 0) ? 3 : 1;
    *pcols = 32 * *RT;
    wgrad_plan(M, 4, feat_dim, rc, rpc);
}

// The tiled split-K form (bf16, visproj_wgrad.hip) keeps one fp32 [d_out, feat_dim] partial per row chunk: 16 chunks x 6.3 MB = 100 MB at
// feat_dim 2048 -> 768, written once and read once by the finalize launch (16.5 of the kernel's 87 us); the job-stream form of the
// fp32 path needs a few MB.  The size is asked for per IO dtype; the dtype-less entry point returns the larger of the two.
extern "C" size_t vlpet_visproj_wgrad_workspace_bytes_io(int64_t M, int feat_dim, int d_out, int io_dtype) {
    if (M <= 0 || feat_dim <= 0 || d_out <= 0 || !dtype_ok(io_dtype)) return 0;
    if (k4_wgrad2_applies(M, feat_dim, d_out, io_dtype == VLPET_F32))
        return align256(k4_wgrad2_workspace_bytes(M, feat_dim, d_out));
    int RT, pcols, rc; int64_t rpc;
    visproj_wgrad_plan(M, feat_dim, d_out, &RT, &pcols, &rc, &rpc);
    return align256(wgrad_workspace_bytes(4, RT, feat_dim, rc));
}
extern "C" size_t vlpet_visproj_wgrad_workspace_bytes(int64_t M, int feat_dim, int d_out) {
    const size_t a = vlpet_visproj_wgrad_workspace_bytes_io(M, feat_dim, d_out, VLPET_BF16);
    const size_t b = vlpet_visproj_wgrad_workspace_bytes_io(M, feat_dim, d_out, VLPET_F32);
    return a > b ? a : b;
}

extern "C" int vlpet_visproj_wgrad(const void* dpre, const void* feats, float* dw, float* db, void* workspace,
                                   size_t workspace_bytes, int64_t M, int feat_dim, int d_out, int io_dtype,
                                   vlpet_stream_t stream) {
    if (!dpre || !feats || !dw || !db || !workspace) return VLPET_E_NULL;
    if (M <= 0 || d_out % 32 != 0 || feat_dim <= 0 || feat_dim % 64 != 0) return VLPET_E_SHAPE;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (!aligned16(dpre) || !aligned16(feats) || !aligned16(workspace)) return VLPET_E_ALIGN;
    if (k4_wgrad2_applies(M, feat_dim, d_out, io_dtype == VLPET_F32)) {   // tiled split-K GEMM (round 3)
        if (workspace_bytes < k4_wgrad2_workspace_bytes(M, feat_dim, d_out)) return VLPET_E_WORKSPACE;
        return herr(launch_k4_wgrad2(dpre, feats, dw, db, workspace, M, feat_dim, d_out, (hipStream_t)stream));
    }
    int RT, pcols, rc; int64_t rpc;
    visproj_wgrad_plan(M, feat_dim, d_out, &RT, &pcols, &rc, &rpc);
    if (workspace_bytes < wgrad_workspace_bytes(4, RT, feat_dim, rc)) return VLPET_E_WORKSPACE;
    const size_t esz = io_dtype == VLPET_F32 ? 4 : 2;
    const int njobs_total = d_out / pcols;
    for (int j0 = 0; j0 < njobs_total; j0 += 4) {
        WgradArgs g{};
        g.M = M; g.RT = RT; g.row_chunks = rc; g.rows_per_chunk = rpc;
        g.partial = reinterpret_cast<float*>(workspace);
        g.njobs = njobs_total - j0 < 4 ? njobs_total - j0 : 4;
        for (int j = 0; j < g.njobs; ++j) {
            WgradJob& J = g.job[j];
            const int c0 = (j0 + j) * pcols;
            J.P = reinterpret_cast<const uint8_t*>(dpre) + (size_t)c0 * esz; J.ldp = d_out; J.pcols = pcols;
            J.X = feats; J.ldx = feat_dim; J.xcols = feat_dim;
            J.drop = NO_DROP; J.has_drop = 0; J.scale = 1.f;
            J.out = dw + (size_t)c0 * feat_dim; J.ldo = feat_dim; J.transposed = 0; J.out_rows = pcols;
            J.colsum_x = nullptr; J.colsum_p = db + c0;
        }
        hipError_t e = launch_wgrad(g, io_dtype == VLPET_F32, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

// ------------------------------------------------------------------ f4: low-rank visual projector
// LowRankVisualEmbedding (src/modeling_bart.py:195-334):  fe = up(gelu_new(cat_i down_i(feats))) [* (sigmoid(gup(gelu_new(gdown(feats)))) (+ 1))]
// One packed buffer per projection pair: [square pair pack at d_out: up, up_t, biases (down slots zero)] [down-only pack at feat_dim].
static inline bool lowrank_dims_ok(int feat_dim, int d_out) {
    return feat_dim > 0 && feat_dim % 64 == 0 && d_out > 0 && d_out % 64 == 0;
}
static inline size_t lowrank_sq_bytes(int tiles, int d_out, int NS) { return align256((size_t)pack_geom(tiles, d_out, NS).total_bytes); }
static inline size_t lowrank_dn_bytes(int tiles, int feat_dim, int NS) {
    return align256((size_t)(feat_dim / 16) * tiles * NS * 1024 + (size_t)(32 * tiles + feat_dim) * 4);
}
extern "C" size_t vlpet_lowrank_packed_bytes(int tiles, int feat_dim, int d_out, int io_dtype) {
    if (!(tiles == 1 || tiles == 3) || !lowrank_dims_ok(feat_dim, d_out)) return 0;
    const int NS = io_dtype == VLPET_F32 ? 2 : 1;
    return lowrank_sq_bytes(tiles, d_out, NS) + lowrank_dn_bytes(tiles, feat_dim, NS);
}

extern "C" int vlpet_lowrank_pack(const void* const* wd_heads, const void* const* bd_heads, int n_heads,
                                  const void* wu, const void* bu, int r, int feat_dim, int d_out, int tiles,
                                  int param_dtype, int io_dtype, void* packed, vlpet_stream_t stream) {
    if (!wd_heads || !wu || !packed) return VLPET_E_NULL;
    if (!lowrank_dims_ok(feat_dim, d_out) || r <= 0 || n_heads <= 0 || n_heads > VLPET_MAX_HEADS || r % n_heads != 0) return VLPET_E_SHAPE;
    if (!(tiles == 1 || tiles == 3) || r > 32 * tiles) return VLPET_E_RANK;
    if (!dtype_ok(param_dtype) || !dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (!aligned16(packed)) return VLPET_E_ALIGN;
    const int NS = io_dtype == VLPET_F32 ? 2 : 1;
    PackArgs a;
    for (int i = 0; i < VLPET_MAX_HEADS; ++i) {
        a.wd[i] = nullptr;
        a.bd[i] = (bd_heads && i < n_heads) ? bd_heads[i] : nullptr;
        if (i < n_heads && wd_heads[i] == nullptr) return VLPET_E_NULL;
    }
    a.n_heads = n_heads; a.rows_per_head = r / n_heads;
    a.r = r; a.RT = tiles; a.src_bf16 = param_dtype == VLPET_BF16;
    // (i) the up side at d_out: up / up_t fragments and both biases; no down weight (its slots come out zero)
    a.wu = wu; a.bu = bu; a.d = d_out; a.n_packs = 4;
    a.out = reinterpret_cast<uint8_t*>(packed);
    hipError_t e = launch_pack_pair(a, NS, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    // (ii) the down side at feat_dim: down fragments only
    for (int i = 0; i < n_heads; ++i) a.wd[i] = wd_heads[i];
    a.wu = nullptr; a.bu = nullptr; a.d = feat_dim; a.n_packs = 1;
    a.out = reinterpret_cast<uint8_t*>(packed) + lowrank_sq_bytes(tiles, d_out, NS);
    return herr(launch_pack_pair(a, NS, (hipStream_t)stream));
}

static int lowrank_common(int64_t M, int feat_dim, int d_out, int tiles, int io_dtype) {
    if (M <= 0 || !lowrank_dims_ok(feat_dim, d_out)) return VLPET_E_SHAPE;
    if (io_dtype == VLPET_F32 && (feat_dim % 32 != 0)) return VLPET_E_SHAPE;
    if (!(tiles == 1 || tiles == 3)) return VLPET_E_RANK;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    return 0;
}

// packed_g == NULL: ungated projector (the gate chain runs on packed_a with multiplier 0, offset 1).
// gate_residual: 1 = fe + fe*gate (use_visual_projector_residual_connection), 0 = fe*gate.
extern "C" int vlpet_lowrank_gate_fwd(const void* feats, const void* packed_a, const void* packed_g, void* fe,
                                      void* saved, int64_t M, int feat_dim, int d_out, int tiles, int gate_residual,
                                      int io_dtype, vlpet_stream_t stream) {
    int rc = lowrank_common(M, feat_dim, d_out, tiles, io_dtype);
    if (rc) return rc;
    if (!feats || !packed_a || !fe) return VLPET_E_NULL;
    if (!aligned16(feats) || !aligned16(packed_a) || !aligned16(fe) || (packed_g && !aligned16(packed_g)) ||
        (saved && !aligned16(saved))) return VLPET_E_ALIGN;
    const int NS = io_dtype == VLPET_F32 ? 2 : 1;
    const size_t sq = lowrank_sq_bytes(tiles, d_out, NS);
    const bool gated = packed_g != nullptr;
    const uint8_t* pa = reinterpret_cast<const uint8_t*>(packed_a);
    const uint8_t* pgt = gated ? reinterpret_cast<const uint8_t*>(packed_g) : pa;
    PetFwdArgs a;
    a.xa = feats; a.res = nullptr; a.xg = feats; a.out = fe;
    a.pk_a = pa; a.pk_g = pgt;
    a.pk_a_dn = pa + sq; a.pk_g_dn = pgt + sq;
    a.drop = NO_DROP;
    a.M = M; a.d = d_out; a.d_in = feat_dim; a.RT = tiles;
    a.s2 = 0.f; a.sd = 1.f; a.gs = 1.f; a.flags = PET_GATE;
    a.gm = gated ? 1.f : 0.f; a.go = gated ? (gate_residual ? 1.f : 0.f) : 1.f;
    a.save = saved; a.save_stride = (int64_t)saved_stride(M, tiles, io_dtype);
    a.dbg = 0; a.dbg_ts = nullptr;
    return herr(launch_pet_lowrank_fwd(a, io_dtype == VLPET_F32, (hipStream_t)stream));
}

struct LowrankWs { size_t dp_a, dp_g, dh, dq, partial, total; int row_chunks; int64_t rows_per_chunk; };
static LowrankWs lowrank_ws(int64_t M, int feat_dim, int d_out, int tiles, int io_dtype) {
    LowrankWs w{};
    const size_t esz = io_dtype == VLPET_F32 ? 4 : 2;
    const size_t side = align256((size_t)M * 32 * tiles * esz), wide = align256((size_t)M * d_out * esz);
    size_t o = 0;
    w.dp_a = o; o += side; w.dp_g = o; o += side; w.dh = o; o += wide; w.dq = o; o += wide;
    const int xmax = feat_dim > d_out ? feat_dim : d_out;
    wgrad_plan(M, 4, xmax, &w.row_chunks, &w.rows_per_chunk);
    w.partial = o; o += align256(wgrad_workspace_bytes(4, tiles, xmax, w.row_chunks));
    w.total = o;
    return w;
}
extern "C" size_t vlpet_lowrank_bwd_workspace_bytes(int64_t M, int feat_dim, int d_out, int tiles, int io_dtype) {
    if (lowrank_common(M, feat_dim, d_out, tiles, io_dtype)) return 0;
    return lowrank_ws(M, feat_dim, d_out, tiles, io_dtype).total;
}

// dfe = d loss / d fe ([M, d_out]); `saved` = the forward's block.  Weight gradients (fp32, overwritten): dwd [r, feat_dim],
// dbd [r], dwu [d_out, r], dbu [d_out] and the gate's four (ignored and may be NULL when packed_g == NULL).
extern "C" int vlpet_lowrank_gate_bwd(const void* dfe, const void* feats, const void* saved, const void* packed_a,
                                      const void* packed_g, float* dwd, float* dbd, float* dwu, float* dbu,
                                      float* dwgd, float* dbgd, float* dwgu, float* dbgu, int r, int rg,
                                      void* workspace, size_t workspace_bytes, int64_t M, int feat_dim, int d_out,
                                      int tiles, int gate_residual, int io_dtype, vlpet_stream_t stream) {
    int rc = lowrank_common(M, feat_dim, d_out, tiles, io_dtype);
    if (rc) return rc;
    const bool gated = packed_g != nullptr;
    if (!dfe || !feats || !saved || !packed_a || !dwd || !dbd || !dwu || !dbu || !workspace) return VLPET_E_NULL;
    if (gated && (!dwgd || !dbgd || !dwgu || !dbgu)) return VLPET_E_NULL;
    if (r <= 0 || r > 32 * tiles || (gated && (rg <= 0 || rg > 32 * tiles))) return VLPET_E_RANK;
    if (!aligned16(dfe) || !aligned16(feats) || !aligned16(saved) || !aligned16(packed_a) || !aligned16(workspace) ||
        (gated && !aligned16(packed_g))) return VLPET_E_ALIGN;
    const LowrankWs w = lowrank_ws(M, feat_dim, d_out, tiles, io_dtype);
    if (workspace_bytes < w.total) return VLPET_E_WORKSPACE;
    uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
    const uint8_t* sv = reinterpret_cast<const uint8_t*>(saved);
    PetBwdArgs b{};
    b.dy = dfe; b.xa = feats; b.res = nullptr; b.xg = feats;
    b.dxa = nullptr; b.dxg = nullptr; b.dxg_in = nullptr;
    b.saved = saved; b.saved_stride = (int64_t)saved_stride(M, tiles, io_dtype);
    b.z_a = const_cast<uint8_t*>(sv); b.z_g = const_cast<uint8_t*>(sv) + 2 * b.saved_stride;
    b.dp_a = ws + w.dp_a; b.dp_g = ws + w.dp_g; b.dh = ws + w.dh; b.dq = ws + w.dq;
    b.pk_a = reinterpret_cast<const uint8_t*>(packed_a);
    b.pk_g = gated ? reinterpret_cast<const uint8_t*>(packed_g) : b.pk_a;
    b.drop = NO_DROP;
    b.M = M; b.d = d_out; b.RT = tiles;
    b.s2 = 0.f; b.sd = 1.f; b.gs = 1.f; b.flags = PET_GATE;
    b.gm = gated ? 1.f : 0.f; b.go = gated ? (gate_residual ? 1.f : 0.f) : 1.f;
    hipError_t e = launch_pet_lowrank_bwd(b, io_dtype == VLPET_F32, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;

    WgradArgs g{};
    g.M = M; g.RT = tiles; g.row_chunks = w.row_chunks; g.rows_per_chunk = w.rows_per_chunk;
    g.partial = reinterpret_cast<float*>(ws + w.partial);
    const int ldp = 32 * tiles;
    auto job = [&](int i, const void* P, const void* X, int xw, float* out, int ldo, int transposed, int out_rows,
                   float* csx, float* csp) {
        WgradJob& J = g.job[i];
        J.P = P; J.ldp = ldp; J.pcols = ldp;
        J.X = X; J.ldx = xw; J.xcols = xw;
        J.drop = NO_DROP; J.has_drop = 0;
        J.scale = 1.f; J.out = out; J.ldo = ldo; J.transposed = transposed; J.out_rows = out_rows;
        J.colsum_x = csx; J.colsum_p = csp;
    };
    job(0, b.dp_a, feats, feat_dim, dwd, feat_dim, 0, r, nullptr, dbd);     // dWd[c,k] = sum_m dpre[m,c] feats[m,k]
    job(1, b.z_a, b.dh, d_out, dwu, r, 1, r, dbu, nullptr);                  // dWu[f,c] = sum_m dh[m,f] z[m,c]
    g.njobs = 2;
    if (gated) {
        job(2, b.dp_g, feats, feat_dim, dwgd, feat_dim, 0, rg, nullptr, dbgd);
        job(3, b.z_g, b.dq, d_out, dwgu, rg, 1, rg, dbgu, nullptr);
        g.njobs = 4;
    }
    return herr(launch_wgrad(g, io_dtype == VLPET_F32, (hipStream_t)stream));
}

// out = LayerNorm(y) * gamma + beta + r   (visual_projector_layer_norm, then the position / order-embedding term:
// src/modeling_bart.py:298-299, 324-325).  Backward: vlpet_sublayer_tail_bwd with h_save = y, p = 0 (its dx1 is d/dy;
// d/dr is dout itself).
extern "C" int vlpet_norm_residual_fwd(const void* y, const void* r, const float* gamma, const float* beta, void* out,
                                       float* mean, float* rstd, int64_t M, int d, float eps, int io_dtype,
                                       vlpet_stream_t stream);

// ---- K5 sublayer tail -------------------------------------------------------------------------------------
static int tail_common(int64_t M, int d, float p, int io_dtype) {
    if (M <= 0 || d <= 0 || d % 8 != 0) return VLPET_E_SHAPE;
    if (!(p >= 0.f && p < 1.f)) return VLPET_E_SHAPE;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    const int pieces = d / (io_dtype == VLPET_F32 ? 4 : 8);
    if (pieces > 8 * 64) return VLPET_E_SHAPE;
    return 0;
}
static uint32_t tail_thr(float p) {
    double t = (double)p * 65536.0 + 0.5;
    if (t > 65535.0) t = 65535.0;
    return (uint32_t)t;
}

extern "C" int vlpet_sublayer_tail_partials(int64_t M) { return M > 0 ? tail_blocks(M) : 0; }

// LayerNorm backward from the normalised rows (K4 saves xhat and rstd, not the pre-norm rows): the tail's backward kernel
// with `h` = xhat.  dx [M, d] = d/d(pre-norm); dgb_partials as in vlpet_sublayer_tail_bwd (or NULL).
extern "C" int vlpet_layernorm_bwd_xhat(const void* dout, const void* xhat, const float* rstd, const float* gamma, void* dx,
                                        float* dgb_partials, int64_t M, int d, int io_dtype, vlpet_stream_t stream) {
    int rc = tail_common(M, d, 0.f, io_dtype);
    if (rc) return rc;
    if (!dout || !xhat || !rstd || !gamma || !dx) return VLPET_E_NULL;
    if (!aligned16(dout) || !aligned16(xhat) || !aligned16(dx)) return VLPET_E_ALIGN;
    TailArgs a{};
    a.out = const_cast<void*>(dout); a.h = const_cast<void*>(xhat); a.mean = nullptr; a.rstd = const_cast<float*>(rstd);
    a.gamma = gamma; a.x1 = dx; a.y = nullptr; a.dgb = dgb_partials; a.M = M; a.d = d; a.thr = 0; a.keep_scale = 1.f;
    a.norm = 1; a.h_xhat = 1;
    return herr(launch_tail(a, io_dtype == VLPET_F32, true, (hipStream_t)stream));
}

// T5's RMS norm (my_transformers/modeling_t5.py:235-252: x * rsqrt(mean(x^2) + eps) * weight) as one pass each way on the tail
// kernels: forward out = rmsnorm(x) * gamma, rstd [M] saved; backward dx from (dout, x, rstd, gamma) + the dgamma partials.
extern "C" int vlpet_rmsnorm_fwd(const void* x, const float* gamma, void* out, float* rstd, int64_t M, int d, float eps,
                                 int io_dtype, vlpet_stream_t stream) {
    int rc = tail_common(M, d, 0.f, io_dtype);
    if (rc) return rc;
    if (!x || !gamma || !out || !rstd) return VLPET_E_NULL;
    if (!aligned16(x) || !aligned16(out)) return VLPET_E_ALIGN;
    TailArgs a{};
    a.y = nullptr; a.x1 = x; a.out = out; a.h = nullptr; a.gamma = gamma; a.beta = nullptr; a.mean = nullptr; a.rstd = rstd;
    a.keep_out = nullptr; a.dgb = nullptr; a.M = M; a.d = d; a.eps = eps; a.thr = 0; a.keep_scale = 1.f; a.norm = 1; a.rms = 1;
    return herr(launch_tail(a, io_dtype == VLPET_F32, false, (hipStream_t)stream));
}

extern "C" int vlpet_rmsnorm_bwd(const void* dout, const void* x, const float* rstd, const float* gamma, const void* dx_in,
                                 void* dx, float* dgb_partials, int64_t M, int d, int io_dtype, vlpet_stream_t stream) {
    int rc = tail_common(M, d, 0.f, io_dtype);
    if (rc) return rc;
    if (!dout || !x || !rstd || !gamma || !dx) return VLPET_E_NULL;
    if (!aligned16(dout) || !aligned16(x) || !aligned16(dx) || (dx_in && !aligned16(dx_in))) return VLPET_E_ALIGN;
    TailArgs a{};
    a.out = const_cast<void*>(dout); a.h = const_cast<void*>(x); a.mean = nullptr; a.rstd = const_cast<float*>(rstd);
    a.gamma = gamma; a.x1 = dx; a.y = nullptr; a.dgb = dgb_partials; a.M = M; a.d = d; a.thr = 0; a.keep_scale = 1.f;
    a.norm = 1; a.rms = 1; a.dres = dx_in;
    return herr(launch_tail(a, io_dtype == VLPET_F32, true, (hipStream_t)stream));
}

// T5's residual tail and the NEXT sublayer's T5LayerNorm in one pass (round 5):  sum = x1 + dropout(y);  normed = rmsnorm(sum) * gamma_next.
// Replaces my_transformers/modeling_t5.py:408 (824) followed by :366 (782) of the next sublayer.  Backward: vlpet_rmsnorm_tail_bwd.
extern "C" int vlpet_sublayer_tail_rms_fwd(const void* y, const void* x1, const float* gamma_next, void* sum, void* normed, float* rstd,
                                           int64_t M, int d, float eps, float p, uint64_t seed, int io_dtype, vlpet_stream_t stream) {
    int rc = tail_common(M, d, p, io_dtype);
    if (rc) return rc;
    if (!y || !x1 || !gamma_next || !sum || !normed || !rstd) return VLPET_E_NULL;
    if (!aligned16(y) || !aligned16(x1) || !aligned16(sum) || !aligned16(normed)) return VLPET_E_ALIGN;
    TailArgs a{};
    a.y = y; a.x1 = x1; a.out = sum; a.out2 = normed; a.gamma2 = gamma_next; a.rstd = rstd; a.M = M; a.d = d; a.eps = eps;
    a.thr = tail_thr(p); a.keep_scale = 1.0f / (1.0f - p); a.seed = seed; a.seed_ctr = g_seed_ctr.load(); a.norm = 0;
    return herr(launch_tail(a, io_dtype == VLPET_F32, false, (hipStream_t)stream));
}
// ... and its backward: d_sum = rmsnorm'(d_normed) (+ dsum_in, the gradient the sum's other readers parked);  dx1 = d_sum;
// dy = d_sum * keep / (1 - p) (written when p > 0; with p = 0 dy == dx1).  One pass instead of the norm's backward + the tail's.
extern "C" int vlpet_rmsnorm_tail_bwd(const void* d_normed, const void* sum, const float* rstd, const float* gamma_next, const void* dsum_in,
                                      void* dx1, void* dy, float* dgb_partials, int64_t M, int d, float p, uint64_t seed, int io_dtype,
                                      vlpet_stream_t stream) {
    int rc = tail_common(M, d, p, io_dtype);
    if (rc) return rc;
    if (!d_normed || !sum || !rstd || !gamma_next || !dx1) return VLPET_E_NULL;
    const uint32_t thr = tail_thr(p);
    if (thr && !dy) return VLPET_E_NULL;
    if (!aligned16(d_normed) || !aligned16(sum) || !aligned16(dx1) || (dy && !aligned16(dy)) || (dsum_in && !aligned16(dsum_in))) return VLPET_E_ALIGN;
    TailArgs a{};
    a.out = const_cast<void*>(d_normed); a.h = const_cast<void*>(sum); a.mean = nullptr; a.rstd = const_cast<float*>(rstd);
    a.gamma = gamma_next; a.x1 = dx1; a.y = dy; a.dgb = dgb_partials; a.M = M; a.d = d; a.thr = thr; a.keep_scale = 1.0f / (1.0f - p);
    a.seed = seed; a.seed_ctr = g_seed_ctr.load(); a.norm = 1; a.rms = 1; a.dres = dsum_in;
    return herr(launch_tail(a, io_dtype == VLPET_F32, true, (hipStream_t)stream));
}

// Column sums of x [M, n] in fp32 (OVERWRITTEN): the gradient of a trainable bias (dy.sum(0)).  workspace: at least
// vlpet_sublayer_tail_partials(M) * n floats.  n % 16 == 0.
extern "C" int vlpet_colsum(const void* x, int64_t M, int n, float* workspace, float* out, int io_dtype, vlpet_stream_t stream) {
    if (M <= 0 || n <= 0 || n % 16 != 0) return VLPET_E_SHAPE;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (n / (io_dtype == VLPET_F32 ? 4 : 8) > 8 * 64) return VLPET_E_SHAPE;
    if (!x || !workspace || !out) return VLPET_E_NULL;
    if (!aligned16(x)) return VLPET_E_ALIGN;
    return herr(launch_colsum(x, M, n, workspace, out, io_dtype == VLPET_F32, (hipStream_t)stream));
}

extern "C" int vlpet_colsum_partial(const void* x, int64_t M, int n, float* workspace, int io_dtype, vlpet_stream_t stream) {
    if (M <= 0 || n <= 0 || n % 16 != 0) return VLPET_E_SHAPE;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (n / (io_dtype == VLPET_F32 ? 4 : 8) > 8 * 64) return VLPET_E_SHAPE;
    if (!x || !workspace) return VLPET_E_NULL;
    if (!aligned16(x)) return VLPET_E_ALIGN;
    return herr(launch_colsum_partial(x, M, n, workspace, io_dtype == VLPET_F32, (hipStream_t)stream));
}

extern "C" int vlpet_reduce_batch(const float* const* partials, float* const* out0, float* const* out1, const int* n_partials,
                                  const int* d, int n_jobs, vlpet_stream_t stream) {
    if (n_jobs <= 0) return n_jobs == 0 ? 0 : VLPET_E_SHAPE;
    if (!partials || !out0 || !out1 || !n_partials || !d) return VLPET_E_NULL;
    for (int k0 = 0; k0 < n_jobs; k0 += VLPET_REDUCE_BATCH) {
        ReduceBatch b{};
        int max_d = 0;
        b.n = n_jobs - k0 < VLPET_REDUCE_BATCH ? n_jobs - k0 : VLPET_REDUCE_BATCH;
        for (int k = 0; k < b.n; ++k) {
            const int j = k0 + k;
            if (!partials[j] || (!out0[j] && !out1[j])) return VLPET_E_NULL;
            if (n_partials[j] <= 0 || d[j] <= 0) return VLPET_E_SHAPE;
            b.j[k] = ReduceJob{partials[j], out0[j], out1[j], n_partials[j], d[j]};
            if (d[j] > max_d) max_d = d[j];
        }
        if (int rc = herr(launch_tail_reduce_batch(b, max_d, (hipStream_t)stream))) return rc;
    }
    return 0;
}

extern "C" int vlpet_sublayer_tail_reduce(const float* dgb_partials, int n_partials, int d, float* dgamma, float* dbeta,
                                          vlpet_stream_t stream) {
    if (n_partials <= 0 || d <= 0) return VLPET_E_SHAPE;
    if (!dgb_partials || (!dgamma && !dbeta)) return VLPET_E_NULL;
    return herr(launch_tail_reduce(dgb_partials, n_partials, d, dgamma, dbeta, (hipStream_t)stream));
}

extern "C" int vlpet_sublayer_tail_fwd(const void* y, const void* x1, const float* gamma, const float* beta, void* out,
                                       void* h_save, float* mean, float* rstd, uint8_t* keep_out, int64_t M, int d,
                                       float eps, float p, uint64_t seed, int norm_mode, int io_dtype,
                                       vlpet_stream_t stream) {
    int rc = tail_common(M, d, p, io_dtype);
    if (rc) return rc;
    if (!y || !x1 || !out) return VLPET_E_NULL;
    if (norm_mode && (!gamma || !mean || !rstd)) return VLPET_E_NULL;
    if (norm_mode != 0 && norm_mode != 1) return VLPET_E_SHAPE;
    if (!aligned16(y) || !aligned16(x1) || !aligned16(out) || (h_save && !aligned16(h_save))) return VLPET_E_ALIGN;
    TailArgs a{};
    a.y = y; a.x1 = x1; a.out = out; a.h = h_save; a.gamma = gamma; a.beta = beta; a.mean = mean; a.rstd = rstd;
    a.keep_out = keep_out; a.dgb = nullptr; a.M = M; a.d = d; a.eps = eps; a.thr = tail_thr(p);
    a.keep_scale = 1.0f / (1.0f - p); a.seed = seed; a.seed_ctr = g_seed_ctr.load(); a.norm = norm_mode;
    return herr(launch_tail(a, io_dtype == VLPET_F32, false, (hipStream_t)stream));
}

extern "C" int vlpet_norm_residual_fwd(const void* y, const void* r, const float* gamma, const float* beta, void* out,
                                       float* mean, float* rstd, int64_t M, int d, float eps, int io_dtype,
                                       vlpet_stream_t stream) {
    int rc = tail_common(M, d, 0.f, io_dtype);
    if (rc) return rc;
    if (!y || !r || !out || !gamma || !mean || !rstd) return VLPET_E_NULL;
    if (!aligned16(y) || !aligned16(r) || !aligned16(out)) return VLPET_E_ALIGN;
    TailArgs a{};
    a.y = y; a.x1 = r; a.out = out; a.h = nullptr; a.gamma = gamma; a.beta = beta; a.mean = mean; a.rstd = rstd;
    a.keep_out = nullptr; a.dgb = nullptr; a.M = M; a.d = d; a.eps = eps; a.thr = 0; a.keep_scale = 1.f; a.seed = 0; a.seed_ctr = nullptr;
    a.norm = 1; a.post = 1;
    return herr(launch_tail(a, io_dtype == VLPET_F32, false, (hipStream_t)stream));
}

extern "C" int vlpet_sublayer_tail_bwd(const void* dout, const void* h_save, const float* mean, const float* rstd,
                                       const float* gamma, void* dx1, void* dy, float* dgb_partials, int64_t M, int d,
                                       float p, uint64_t seed, int norm_mode, int io_dtype, vlpet_stream_t stream) {
    int rc = tail_common(M, d, p, io_dtype);
    if (rc) return rc;
    if (norm_mode != 0 && norm_mode != 1) return VLPET_E_SHAPE;
    const uint32_t thr = tail_thr(p);
    // dx1 may be NULL for the plain residual tail under dropout (norm_mode 0, p > 0): there d/dx1 IS dout, and a caller that hands dout on
    // itself saves the copy (a third of the pass's traffic; T5 runs 60 such tails per step)
    if (!dout || (!dx1 && (norm_mode != 0 || thr == 0))) return VLPET_E_NULL;
    if (norm_mode && (!h_save || !mean || !rstd || !gamma)) return VLPET_E_NULL;
    if (thr && !dy) return VLPET_E_NULL;
    if (!aligned16(dout) || (dx1 && !aligned16(dx1)) || (dy && !aligned16(dy)) || (h_save && !aligned16(h_save))) return VLPET_E_ALIGN;
    TailArgs a{};
    a.out = const_cast<void*>(dout); a.h = const_cast<void*>(h_save); a.mean = const_cast<float*>(mean);
    a.rstd = const_cast<float*>(rstd); a.gamma = gamma; a.beta = nullptr; a.x1 = dx1; a.y = dy; a.keep_out = nullptr;
    a.dgb = dgb_partials; a.M = M; a.d = d; a.eps = 0.f; a.thr = thr; a.keep_scale = 1.0f / (1.0f - p); a.seed = seed; a.seed_ctr = g_seed_ctr.load();
    a.norm = norm_mode;
    return herr(launch_tail(a, io_dtype == VLPET_F32, true, (hipStream_t)stream));
}

// The same backward from the LayerNorm OUTPUT rows (`out_save` = what vlpet_sublayer_tail_fwd wrote to `out`) instead of the pre-norm
// sum: xhat = (out - beta) / gamma.  With it the forward is called with h_save = NULL and moves 3 row tensors instead of 4.
extern "C" int vlpet_sublayer_tail_bwd_out(const void* dout, const void* out_save, const float* rstd, const float* gamma,
                                           const float* beta, void* dx1, void* dy, float* dgb_partials, int64_t M, int d,
                                           float p, uint64_t seed, int io_dtype, vlpet_stream_t stream) {
    int rc = tail_common(M, d, p, io_dtype);
    if (rc) return rc;
    if (!dout || !dx1 || !out_save || !rstd || !gamma) return VLPET_E_NULL;
    const uint32_t thr = tail_thr(p);
    if (thr && !dy) return VLPET_E_NULL;
    if (!aligned16(dout) || !aligned16(dx1) || (dy && !aligned16(dy)) || !aligned16(out_save)) return VLPET_E_ALIGN;
    TailArgs a{};
    a.out = const_cast<void*>(dout); a.h = const_cast<void*>(out_save); a.mean = nullptr;
    a.rstd = const_cast<float*>(rstd); a.gamma = gamma; a.beta = beta; a.x1 = dx1; a.y = dy; a.keep_out = nullptr;
    a.dgb = dgb_partials; a.M = M; a.d = d; a.eps = 0.f; a.thr = thr; a.keep_scale = 1.0f / (1.0f - p); a.seed = seed; a.seed_ctr = g_seed_ctr.load();
    a.norm = 1; a.h_out = 1;
    return herr(launch_tail(a, io_dtype == VLPET_F32, true, (hipStream_t)stream));
}

static uint32_t attn_thr(float p) {
    double t = (double)p * 4294967296.0 + 0.5;
    if (t > 4294967295.0) t = 4294967295.0;
    return (uint32_t)t;
}

static int attn_ld_ok(int H, int ld_q, int ld_kv) {
    return ld_q >= H * 64 && ld_kv >= H * 64 && ld_q % 8 == 0 && ld_kv % 8 == 0;
}

// The argument checks of the attention entry points and the kernel arguments of a call that passes them.  max_len: VLPET_ATTN_MAX_LEN
// (attn.hip) or VLPET_ATTN_LONG_MAX_LEN (attn_long.hip, attn_long_bwd.hip); bwd: dout, dq, dk, dv are required, and with them the
// transposed copy of a bias (attn.hip) or the [B, H, Lq] of scratch `delta` (attn_long_bwd.hip, which does not read bias_t) -- a forward
// passes NULL for all of these.  Shape errors come first (the lengths, the grid -- a workgroup per pair and 128 queries, or 128 keys in the
// long backward's second launch: B * H at max_len = 128 --, the row strides, scale, p), then NULL, then alignment.
static int attn_args(AttnArgs& a, int max_len, bool bwd, const void* q, const void* k, const void* v, const uint8_t* key_mask,
                     const float* bias, const float* bias_t, const void* o, const float* lse, uint8_t* keep_out, const void* dout,
                     void* dq, void* dk, void* dv, const float* delta, int B, int H, int Lq, int Lk, int ld_q, int ld_k, int ld_v,
                     int causal, float scale, float p, uint64_t seed) {
    const bool lng = max_len > VLPET_ATTN_MAX_LEN;
    if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0 || Lq > max_len || Lk > max_len) return VLPET_E_SHAPE;
    if ((int64_t)B * H * ((Lq + 127) / 128) > 0x7fffffffLL || (int64_t)B * H * ((Lk + 127) / 128) > 0x7fffffffLL) return VLPET_E_SHAPE;
    if (!attn_ld_ok(H, ld_q, ld_k) || !attn_ld_ok(H, ld_q, ld_v) || !(scale != 0.f)) return VLPET_E_SHAPE;
    if (!(p >= 0.0f && p < 1.0f)) return VLPET_E_SHAPE;
    if (!q || !k || !v || !o || !lse) return VLPET_E_NULL;
    if (bwd && (!dout || !dq || !dk || !dv || (lng ? !delta : (bias != nullptr) != (bias_t != nullptr)))) return VLPET_E_NULL;
    if (lng) bias_t = nullptr;
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || (bias && !aligned16(bias))) return VLPET_E_ALIGN;
    if (bwd && (!aligned16(dout) || !aligned16(dq) || !aligned16(dk) || !aligned16(dv) || (bias_t && !aligned16(bias_t)))) return VLPET_E_ALIGN;
    a = AttnArgs{};
    a.ld_q = ld_q; a.ld_kv = ld_k; a.ld_v = ld_v; a.bias = bias; a.bias_t = bias_t;
    a.q = (const __bf16*)q; a.k = (const __bf16*)k; a.v = (const __bf16*)v; a.o = (__bf16*)const_cast<void*>(o);
    a.lse = const_cast<float*>(lse); a.dout = (const __bf16*)dout; a.dq = (__bf16*)dq; a.dk = (__bf16*)dk; a.dv = (__bf16*)dv;
    a.key_mask = key_mask; a.keep_out = keep_out; a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.causal = causal ? 1 : 0;
    a.scale = scale; a.thr = attn_thr(p); a.inv_keep = a.thr ? 1.0f / (1.0f - p) : 1.0f; a.seed = seed; a.seed_ctr = g_seed_ctr.load();
    return 0;
}

// ... with separate row strides for k / dk (ld_k) and v / dv (ld_v): k may be a column block of a wider buffer (the decoder layers' fused
// key projection of the encoder output) while v keeps its own width
extern "C" int vlpet_attn_fwd_kv(const void* q, const void* k, const void* v, const uint8_t* key_mask, const float* bias, void* o,
                                 float* lse, uint8_t* keep_out, int B, int H, int Lq, int Lk, int ld_q, int ld_k, int ld_v, int causal,
                                 float scale, float p, uint64_t seed, vlpet_stream_t stream) {
    AttnArgs a;
    int rc = attn_args(a, VLPET_ATTN_MAX_LEN, false, q, k, v, key_mask, bias, nullptr, o, lse, keep_out, nullptr, nullptr, nullptr, nullptr, nullptr,
                       B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, scale, p, seed);
    return rc ? rc : herr(launch_attn(a, false, (hipStream_t)stream));
}
// attention forward up to VLPET_ATTN_LONG_MAX_LEN keys / queries (attn_long.hip): no dropout, no backward; same checks as vlpet_attn_fwd_kv
extern "C" int vlpet_attn_long_fwd(const void* q, const void* k, const void* v, const uint8_t* key_mask, const float* bias, void* o,
                                   float* lse, int B, int H, int Lq, int Lk, int ld_q, int ld_k, int ld_v, int causal, float scale,
                                   vlpet_stream_t stream) {
    AttnArgs a;
    int rc = attn_args(a, VLPET_ATTN_LONG_MAX_LEN, false, q, k, v, key_mask, bias, nullptr, o, lse, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                       B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, scale, 0.f, 0);
    if (rc) return rc;
    a.seed_ctr = nullptr;      // (p = 0: thr = 0, inv_keep = 1, and no seed to step)
    return herr(launch_attn_long_fwd(a, (hipStream_t)stream));
}
// the training form of vlpet_attn_long_fwd: dropout on the probabilities (the short kernels' mask rule), optional export of the mask;
// p = 0 launches the kernel of vlpet_attn_long_fwd (the same bits)
extern "C" int vlpet_attn_long_fwd_train(const void* q, const void* k, const void* v, const uint8_t* key_mask, const float* bias, void* o,
                                         float* lse, uint8_t* keep_out, int B, int H, int Lq, int Lk, int ld_q, int ld_k, int ld_v,
                                         int causal, float scale, float p, uint64_t seed, vlpet_stream_t stream) {
    AttnArgs a;
    int rc = attn_args(a, VLPET_ATTN_LONG_MAX_LEN, false, q, k, v, key_mask, bias, nullptr, o, lse, keep_out, nullptr, nullptr, nullptr, nullptr, nullptr,
                       B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, scale, p, seed);
    return rc ? rc : herr(launch_attn_long_fwd(a, (hipStream_t)stream));
}
// ... and its backward (attn_long_bwd.hip): the arguments of vlpet_attn_bwd_kv (bias_t is accepted and not read) plus `delta`, [B, H, Lq]
// fp32 of scratch that the caller allocates
extern "C" int vlpet_attn_long_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                                   const uint8_t* key_mask, const float* bias, const float* bias_t, void* dq, void* dk, void* dv,
                                   int B, int H, int Lq, int Lk, int ld_q, int ld_k, int ld_v, int causal, float scale, float p,
                                   uint64_t seed, float* delta, vlpet_stream_t stream) {
    AttnArgs a;
    int rc = attn_args(a, VLPET_ATTN_LONG_MAX_LEN, true, q, k, v, key_mask, bias, bias_t, o, lse, nullptr, dout, dq, dk, dv, delta,
                       B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, scale, p, seed);
    return rc ? rc : herr(launch_attn_long_bwd(a, delta, (hipStream_t)stream));
}
extern "C" int vlpet_attn_fwd_bias(const void* q, const void* k, const void* v, const uint8_t* key_mask, const float* bias, void* o,
                                   float* lse, uint8_t* keep_out, int B, int H, int Lq, int Lk, int ld_q, int ld_kv, int causal,
                                   float scale, float p, uint64_t seed, vlpet_stream_t stream) {
    return vlpet_attn_fwd_kv(q, k, v, key_mask, bias, o, lse, keep_out, B, H, Lq, Lk, ld_q, ld_kv, ld_kv, causal, scale, p, seed, stream);
}

extern "C" int vlpet_attn_fwd_ld(const void* q, const void* k, const void* v, const uint8_t* key_mask, void* o, float* lse,
                                 uint8_t* keep_out, int B, int H, int Lq, int Lk, int ld_q, int ld_kv, int causal, float scale,
                                 float p, uint64_t seed, vlpet_stream_t stream) {
    return vlpet_attn_fwd_bias(q, k, v, key_mask, nullptr, o, lse, keep_out, B, H, Lq, Lk, ld_q, ld_kv, causal, scale, p, seed, stream);
}

extern "C" int vlpet_attn_fwd(const void* q, const void* k, const void* v, const uint8_t* key_mask, void* o, float* lse,
                              uint8_t* keep_out, int B, int H, int Lq, int Lk, int causal, float scale, float p, uint64_t seed,
                              vlpet_stream_t stream) {
    return vlpet_attn_fwd_ld(q, k, v, key_mask, o, lse, keep_out, B, H, Lq, Lk, H * 64, H * 64, causal, scale, p, seed, stream);
}

extern "C" int vlpet_attn_bwd_kv(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                                 const uint8_t* key_mask, const float* bias, const float* bias_t, void* dq, void* dk, void* dv,
                                 int B, int H, int Lq, int Lk, int ld_q, int ld_k, int ld_v, int causal, float scale, float p, uint64_t seed,
                                 vlpet_stream_t stream) {
    AttnArgs a;
    int rc = attn_args(a, VLPET_ATTN_MAX_LEN, true, q, k, v, key_mask, bias, bias_t, o, lse, nullptr, dout, dq, dk, dv, nullptr,
                       B, H, Lq, Lk, ld_q, ld_k, ld_v, causal, scale, p, seed);
    return rc ? rc : herr(launch_attn(a, true, (hipStream_t)stream));
}
extern "C" int vlpet_attn_bwd_bias(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                                   const uint8_t* key_mask, const float* bias, const float* bias_t, void* dq, void* dk, void* dv,
                                   int B, int H, int Lq, int Lk, int ld_q, int ld_kv, int causal, float scale, float p, uint64_t seed,
                                   vlpet_stream_t stream) {
    return vlpet_attn_bwd_kv(q, k, v, o, dout, lse, key_mask, bias, bias_t, dq, dk, dv, B, H, Lq, Lk, ld_q, ld_kv, ld_kv, causal, scale, p, seed,
                             stream);
}

extern "C" int vlpet_attn_bwd_ld(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                                 const uint8_t* key_mask, void* dq, void* dk, void* dv, int B, int H, int Lq, int Lk, int ld_q,
                                 int ld_kv, int causal, float scale, float p, uint64_t seed, vlpet_stream_t stream) {
    return vlpet_attn_bwd_bias(q, k, v, o, dout, lse, key_mask, nullptr, nullptr, dq, dk, dv, B, H, Lq, Lk, ld_q, ld_kv, causal, scale, p, seed,
                               stream);
}

extern "C" int vlpet_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                              const uint8_t* key_mask, void* dq, void* dk, void* dv, int B, int H, int Lq, int Lk, int causal,
                              float scale, float p, uint64_t seed, vlpet_stream_t stream) {
    return vlpet_attn_bwd_ld(q, k, v, o, dout, lse, key_mask, dq, dk, dv, B, H, Lq, Lk, H * 64, H * 64, causal, scale, p, seed, stream);
}

static int ce_common(int64_t N, int V, int ld, int io_dtype) {
    if (N <= 0 || V <= 0 || ld < V || (ld & 7) != 0) return VLPET_E_SHAPE;
    if (io_dtype != VLPET_F32 && io_dtype != VLPET_BF16) return VLPET_E_DTYPE;
    return 0;
}

extern "C" int vlpet_ce_loss_fwd_checked(const void* logits, const int64_t* labels, float* loss, float* lse, unsigned int* bad_count,
                                         int64_t N, int V, int ld, int io_dtype, vlpet_stream_t stream) {
    int rc = ce_common(N, V, ld, io_dtype);
    if (rc) return rc;
    if (!logits || !labels || !loss || !lse) return VLPET_E_NULL;
    if (!aligned16(logits)) return VLPET_E_ALIGN;
    CeArgs a{};
    a.logits = logits; a.labels = labels; a.loss = loss; a.lse = lse; a.dloss = nullptr; a.dlogits = nullptr;
    a.N = N; a.V = V; a.ld = ld; a.bad = bad_count;
    return herr(launch_ce(a, false, io_dtype == VLPET_F32, (hipStream_t)stream));
}
extern "C" int vlpet_ce_loss_fwd(const void* logits, const int64_t* labels, float* loss, float* lse, int64_t N, int V, int ld,
                                 int io_dtype, vlpet_stream_t stream) {
    return vlpet_ce_loss_fwd_checked(logits, labels, loss, lse, nullptr, N, V, ld, io_dtype, stream);
}

extern "C" int vlpet_ce_loss_bwd(const void* logits, const int64_t* labels, const float* lse, const float* dloss, void* dlogits,
                                 int64_t N, int V, int ld, int io_dtype, vlpet_stream_t stream) {
    int rc = ce_common(N, V, ld, io_dtype);
    if (rc) return rc;
    if (!logits || !labels || !lse || !dloss || !dlogits) return VLPET_E_NULL;
    if (!aligned16(logits) || !aligned16(dlogits)) return VLPET_E_ALIGN;
    CeArgs a{};
    a.logits = logits; a.labels = labels; a.loss = nullptr; a.lse = const_cast<float*>(lse); a.dloss = dloss; a.dlogits = dlogits;
    a.N = N; a.V = V; a.ld = ld;
    return herr(launch_ce(a, true, io_dtype == VLPET_F32, (hipStream_t)stream));
}

static int act_common(int64_t n, int act, float p, int io_dtype) {
    if (n <= 0 || (n & 7) != 0) return VLPET_E_SHAPE;
    if (act != VLPET_ACT_GELU && act != VLPET_ACT_GELU_NEW && act != VLPET_ACT_RELU) return VLPET_E_SHAPE;
    if (!(p >= 0.0f && p < 1.0f)) return VLPET_E_SHAPE;
    if (io_dtype != VLPET_F32 && io_dtype != VLPET_BF16) return VLPET_E_DTYPE;
    return 0;
}

extern "C" int vlpet_act_dropout_fwd(const void* x, void* out, uint8_t* keep_out, int64_t n, int act, float p, uint64_t seed,
                                     int io_dtype, vlpet_stream_t stream) {
    int rc = act_common(n, act, p, io_dtype);
    if (rc) return rc;
    if (!x || !out) return VLPET_E_NULL;
    if (!aligned16(x) || !aligned16(out)) return VLPET_E_ALIGN;
    ActDropArgs a{};
    a.x = x; a.dy = nullptr; a.out = out; a.keep_out = keep_out; a.n = n; a.act = act; a.thr = tail_thr(p);
    a.keep_scale = a.thr ? 1.0f / (1.0f - p) : 1.0f; a.seed = seed; a.seed_ctr = g_seed_ctr.load();
    return herr(launch_act_dropout(a, false, io_dtype == VLPET_F32, (hipStream_t)stream));
}

// x [B, La + Lv, d] = dropout(cat([a [B, La, d], v [B, Lv, d]], dim = 1), p): the joint encoder's input assembly (src/modeling_bart.py:804-820)
extern "C" int vlpet_concat_dropout_fwd(const void* a, const void* v, void* x, int64_t B, int La, int Lv, int d, float p, uint64_t seed,
                                        int io_dtype, vlpet_stream_t stream) {
    if (!a || !v || !x) return VLPET_E_NULL;
    if (B <= 0 || La <= 0 || Lv <= 0 || d <= 0 || d % 8 != 0 || !(p >= 0.f && p < 1.f)) return VLPET_E_SHAPE;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (!aligned16(a) || !aligned16(v) || !aligned16(x)) return VLPET_E_ALIGN;
    const uint32_t thr = tail_thr(p);
    return herr(launch_cat_dropout(a, v, x, B, La, Lv, d, thr, thr ? 1.0f / (1.0f - p) : 1.0f, seed, g_seed_ctr.load(), false,
                                   io_dtype == VLPET_F32, (hipStream_t)stream));
}
// ... backward: dx [B, La + Lv, d] -> da [B, La, d], dv [B, Lv, d] (either NULL: not wanted), the mask regenerated from (p, seed)
extern "C" int vlpet_concat_dropout_bwd(const void* dx, void* da, void* dv, int64_t B, int La, int Lv, int d, float p, uint64_t seed,
                                        int io_dtype, vlpet_stream_t stream) {
    if (!dx || (!da && !dv)) return VLPET_E_NULL;
    if (B <= 0 || La <= 0 || Lv <= 0 || d <= 0 || d % 8 != 0 || !(p >= 0.f && p < 1.f)) return VLPET_E_SHAPE;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (!aligned16(dx) || (da && !aligned16(da)) || (dv && !aligned16(dv))) return VLPET_E_ALIGN;
    const uint32_t thr = tail_thr(p);
    return herr(launch_cat_dropout(da, dv, const_cast<void*>(dx), B, La, Lv, d, thr, thr ? 1.0f / (1.0f - p) : 1.0f, seed, g_seed_ctr.load(), true,
                                   io_dtype == VLPET_F32, (hipStream_t)stream));
}

// ---- prompt tuning: x [B, P + La + Lv, d] = dropout(cat([pre [P, d] (every batch item), a [B, La, d], v [B, Lv, d]], dim = 1), p) -------
extern "C" int vlpet_prefix_concat_chunks(int64_t B) {
    if (B <= 0) return 0;
    int cs, nc;
    prefix_cat_split(B, &cs, &nc);
    return nc;
}
extern "C" size_t vlpet_prefix_concat_ws_bytes(int64_t B, int P, int d) {
    if (B <= 0 || P <= 0 || d <= 0) return 0;
    return (size_t)vlpet_prefix_concat_chunks(B) * (size_t)P * (size_t)d * sizeof(float);
}
static int prefix_cat_common(int64_t B, int P, int La, int Lv, int d, float p, int io_dtype) {
    if (B <= 0 || P <= 0 || La <= 0 || Lv <= 0 || d <= 0 || d % 8 != 0 || !(p >= 0.f && p < 1.f)) return VLPET_E_SHAPE;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    return 0;
}
static PrefixCatArgs prefix_cat_args(const void* pre, const void* a, const void* v, void* x, int64_t B, int P, int La, int Lv, int d, float p,
                                     uint64_t seed) {
    PrefixCatArgs c{};
    c.pre = pre; c.a = a; c.v = v; c.x = x; c.B = B; c.P = P; c.La = La; c.Lv = Lv; c.d = d;
    prefix_cat_split(B, &c.CS, &c.NC);
    c.thr = tail_thr(p); c.keep_scale = c.thr ? 1.0f / (1.0f - p) : 1.0f; c.seed = seed; c.seed_ctr = g_seed_ctr.load();
    return c;
}
extern "C" int vlpet_prefix_concat_dropout_fwd(const void* pre, const void* a, const void* v, void* x, int64_t B, int P, int La, int Lv, int d,
                                               float p, uint64_t seed, int io_dtype, vlpet_stream_t stream) {
    if (!pre || !a || !v || !x) return VLPET_E_NULL;
    if (int rc = prefix_cat_common(B, P, La, Lv, d, p, io_dtype)) return rc;
    if (!aligned16(pre) || !aligned16(a) || !aligned16(v) || !aligned16(x)) return VLPET_E_ALIGN;
    const PrefixCatArgs c = prefix_cat_args(pre, a, v, x, B, P, La, Lv, d, p, seed);
    return herr(launch_prefix_cat(c, false, io_dtype == VLPET_F32, (hipStream_t)stream));
}
// ... backward: dx -> dpre [P, d] (summed over the batch), da, dv; any of them NULL: not wanted.  ws: vlpet_prefix_concat_ws_bytes(B, P, d)
// bytes of fp32 partials, required exactly when dpre is wanted
extern "C" int vlpet_prefix_concat_dropout_bwd(const void* dx, void* dpre, void* da, void* dv, float* ws, int64_t B, int P, int La, int Lv,
                                               int d, float p, uint64_t seed, int io_dtype, vlpet_stream_t stream) {
    if (!dx || (!dpre && !da && !dv) || (dpre && !ws)) return VLPET_E_NULL;
    if (int rc = prefix_cat_common(B, P, La, Lv, d, p, io_dtype)) return rc;
    if (!dpre && ws) return VLPET_E_SHAPE;            // a workspace without the output it serves: a caller's mistake
    if (!aligned16(dx) || (dpre && !aligned16(dpre)) || (da && !aligned16(da)) || (dv && !aligned16(dv)) || (ws && !aligned16(ws)))
        return VLPET_E_ALIGN;
    PrefixCatArgs c = prefix_cat_args(nullptr, da, dv, const_cast<void*>(dx), B, P, La, Lv, d, p, seed);
    c.dpre = dpre; c.ws = ws;
    return herr(launch_prefix_cat(c, true, io_dtype == VLPET_F32, (hipStream_t)stream));
}

extern "C" int vlpet_act_dropout_bwd(const void* dy, const void* x, void* dx, int64_t n, int act, float p, uint64_t seed,
                                     int io_dtype, vlpet_stream_t stream) {
    int rc = act_common(n, act, p, io_dtype);
    if (rc) return rc;
    if (!dy || !x || !dx) return VLPET_E_NULL;
    if (!aligned16(dy) || !aligned16(x) || !aligned16(dx)) return VLPET_E_ALIGN;
    ActDropArgs a{};
    a.x = x; a.dy = dy; a.out = dx; a.keep_out = nullptr; a.n = n; a.act = act; a.thr = tail_thr(p);
    a.keep_scale = a.thr ? 1.0f / (1.0f - p) : 1.0f; a.seed = seed; a.seed_ctr = g_seed_ctr.load();
    return herr(launch_act_dropout(a, true, io_dtype == VLPET_F32, (hipStream_t)stream));
}

// ---- bias gradients where the data already is (biasgrad.hip) ---------------------------------------------------------------
extern "C" size_t vlpet_colsum_seg_workspace_bytes(int64_t M, int n) {
    if (M <= 0 || n <= 0) return 0;
    return colsum_seg_ws_floats(M, n) * sizeof(float);
}
extern "C" int vlpet_colsum_seg(const void* x, int64_t M, int n_segments, int w, int64_t ld, float* const* out, float* workspace,
                                size_t workspace_bytes, int io_dtype, vlpet_stream_t stream) {
    if (M <= 0 || n_segments <= 0 || n_segments > VLPET_COLSUM_SEGS || w <= 0 || w % 16 != 0 || w > 65536) return VLPET_E_SHAPE;
    const int n = n_segments * w;
    if (n > 65536 || ld < n) return VLPET_E_SHAPE;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (ld % (io_dtype == VLPET_F32 ? 4 : 8) != 0) return VLPET_E_ALIGN;      // every row starts on a 16-byte boundary
    if (!x || !out || !workspace) return VLPET_E_NULL;
    if (!aligned16(x) || !aligned16(workspace)) return VLPET_E_ALIGN;
    if (workspace_bytes < vlpet_colsum_seg_workspace_bytes(M, n)) return VLPET_E_WORKSPACE;
    SegOut so{};
    bool any = false;
    for (int s = 0; s < n_segments; ++s) {
        so.p[s] = out[s];
        any = any || out[s] != nullptr;
        if (reinterpret_cast<uintptr_t>(out[s]) & 3) return VLPET_E_ALIGN;
    }
    if (!any) return 0;                     // no segment wanted: nothing to launch
    return herr(launch_colsum_seg(x, M, n, ld, w, so, workspace, io_dtype == VLPET_F32, (hipStream_t)stream));
}

extern "C" int vlpet_act_dropout_bwd_cols(const void* dy, const void* x, void* dx, int64_t M, int n_cols, int act, float p, uint64_t seed,
                                          float* workspace, size_t workspace_bytes, float* out, int* n_partials, int io_dtype,
                                          vlpet_stream_t stream) {
    if (M <= 0 || n_cols <= 0 || n_cols % 8 != 0) return VLPET_E_SHAPE;
    if (int rc = act_common(M * (int64_t)n_cols, act, p, io_dtype)) return rc;
    if (!dy || !x || !dx || !workspace || (!out && !n_partials)) return VLPET_E_NULL;
    if (!aligned16(dy) || !aligned16(x) || !aligned16(dx) || !aligned16(workspace)) return VLPET_E_ALIGN;
    const int nb = act_cols_partials(M, n_cols);
    if (workspace_bytes < (size_t)nb * (size_t)n_cols * sizeof(float)) return VLPET_E_WORKSPACE;
    ActColsArgs a{};
    a.x = x; a.dy = dy; a.dx = dx; a.part = workspace; a.M = M; a.n_cols = n_cols; a.act = act; a.thr = tail_thr(p);
    a.keep_scale = a.thr ? 1.0f / (1.0f - p) : 1.0f; a.seed = seed; a.seed_ctr = g_seed_ctr.load();
    if (int rc = herr(launch_act_dropout_bwd_cols(a, io_dtype == VLPET_F32, (hipStream_t)stream))) return rc;
    if (n_partials) *n_partials = nb;
    if (!out) return 0;                     // the caller reduces (vlpet_sublayer_tail_reduce / vlpet_reduce_batch with d = n_cols / 2)
    return herr(launch_tail_reduce(workspace, nb, n_cols / 2, out, out + n_cols / 2, (hipStream_t)stream));
}

// ---- Downsample ---------------------------------------------------------------------------------------------
extern "C" int vlpet_downsample_fwd(const void* x, void* out, int64_t n_images, int s_in, int s_out, int dim,
                                    int in_dtype, int out_dtype, vlpet_stream_t stream) {
    if (!x || !out) return VLPET_E_NULL;
    if (n_images <= 0 || s_in <= 0 || s_out <= 0 || s_out > s_in || dim <= 0 || dim % 8 != 0) return VLPET_E_SHAPE;
    if (!dtype_ok(in_dtype) || !dtype_ok(out_dtype)) return VLPET_E_DTYPE;
    if (!aligned16(x) || !aligned16(out)) return VLPET_E_ALIGN;
    PoolArgs a;
    a.x = x; a.out = out; a.n_img = n_images; a.s_in = s_in; a.s_out = s_out; a.dim = dim;
    return herr(launch_downsample(a, in_dtype == VLPET_F32, out_dtype == VLPET_F32, (hipStream_t)stream));
}

// ---- small / middleX / middleY gates (row kernels) ------------------------------------------------------------
static int row_common(int64_t M, int d, int io_dtype) {
    if (M <= 0 || d <= 0 || d % 8 != 0) return VLPET_E_SHAPE;
    if (!dtype_ok(io_dtype)) return VLPET_E_DTYPE;
    if (d / (io_dtype == VLPET_F32 ? 4 : 8) > 4 * 64) return VLPET_E_SHAPE;
    return 0;
}
static int row_launch(RowArgs& a, int op, int64_t M, int d, int io_dtype, vlpet_stream_t stream) {
    a.M = M; a.d = d;
    return herr(launch_rowgate(a, op, io_dtype == VLPET_F32, (hipStream_t)stream));
}

extern "C" int vlpet_rowgate_partials(int64_t M) { return M > 0 ? rowgate_blocks(M) : 0; }

extern "C" int vlpet_row_dot(const void* a, const void* c, const float* wa, const float* wc, float* s_out, int64_t M,
                             int d, int io_dtype, vlpet_stream_t stream) {
    int rc = row_common(M, d, io_dtype);
    if (rc) return rc;
    if (!a || !s_out) return VLPET_E_NULL;
    if (!wa && !c) return VLPET_E_NULL;                 // pair mode needs both row operands
    if (wa && c && !wc) return VLPET_E_NULL;
    if (!aligned16(a) || (c && !aligned16(c))) return VLPET_E_ALIGN;
    RowArgs r{};
    r.a = a; r.c = c; r.va = wa; r.vc = wc; r.rs = s_out;
    return row_launch(r, ROW_DOT, M, d, io_dtype, stream);
}

extern "C" int vlpet_row_affine(const void* h, const float* alpha, const float* gamma, void* y, int64_t M, int d,
                                int io_dtype, vlpet_stream_t stream) {
    int rc = row_common(M, d, io_dtype);
    if (rc) return rc;
    if (!h || !alpha || !y) return VLPET_E_NULL;
    if (!aligned16(h) || !aligned16(y)) return VLPET_E_ALIGN;
    RowArgs r{};
    r.a = h; r.ra = alpha; r.rb = gamma; r.o1 = y;
    return row_launch(r, ROW_AFFINE, M, d, io_dtype, stream);
}

extern "C" int vlpet_rowgate_bwd(const void* dy, const void* x1, const void* h, const float* alpha, const float* beta,
                                 const float* wa, const float* wc, void* dh, void* dx1, float* partials, int64_t M,
                                 int d, int io_dtype, vlpet_stream_t stream) {
    int rc = row_common(M, d, io_dtype);
    if (rc) return rc;
    if (!dy || !x1 || !h || !alpha || !beta || !wa || !wc || !dh || !dx1 || !partials) return VLPET_E_NULL;
    if (!aligned16(dy) || !aligned16(x1) || !aligned16(h) || !aligned16(dh) || !aligned16(dx1)) return VLPET_E_ALIGN;
    RowArgs r{};
    r.a = dy; r.c = x1; r.e = h; r.ra = alpha; r.rb = beta; r.va = wa; r.vc = wc; r.o1 = dh; r.o2 = dx1; r.part = partials;
    return row_launch(r, ROW_BWD, M, d, io_dtype, stream);
}

extern "C" int vlpet_vecgate_fwd(const void* h, const float* v, const float* u, void* y, int64_t M, int d, int io_dtype,
                                 vlpet_stream_t stream) {
    int rc = row_common(M, d, io_dtype);
    if (rc) return rc;
    if (!h || !v || !y) return VLPET_E_NULL;
    if (!aligned16(h) || !aligned16(y)) return VLPET_E_ALIGN;
    RowArgs r{};
    r.a = h; r.va = v; r.vc = u; r.o1 = y;
    return row_launch(r, VEC_FWD, M, d, io_dtype, stream);
}

extern "C" int vlpet_vecgate_bwd(const void* dy, const void* h, const float* v, void* dh, float* partials, int64_t M,
                                 int d, int io_dtype, vlpet_stream_t stream) {
    int rc = row_common(M, d, io_dtype);
    if (rc) return rc;
    if (!dy || !h || !v || !dh || !partials) return VLPET_E_NULL;
    if (!aligned16(dy) || !aligned16(h) || !aligned16(dh)) return VLPET_E_ALIGN;
    RowArgs r{};
    r.a = dy; r.c = h; r.va = v; r.o1 = dh; r.part = partials;
    return row_launch(r, VEC_BWD, M, d, io_dtype, stream);
}

// ---- fused clip + AdamW over the flat trainable buffer ------------------------------------------------------
extern "C" int vlpet_optim_blocks(int64_t n) { return n > 0 ? optim_blocks(n) : 0; }

extern "C" int vlpet_grad_sumsq(const float* g, int64_t n, float* partials, vlpet_stream_t stream) {
    if (!g || !partials) return VLPET_E_NULL;
    if (n <= 0) return VLPET_E_SHAPE;
    if (!aligned16(g)) return VLPET_E_ALIGN;
    return herr(launch_sumsq(g, n, partials, (hipStream_t)stream));
}

extern "C" int vlpet_adamw_step(float* p, float* g, float* m, float* v, const uint8_t* decay_mask, int64_t n,
                                const float* partials, int n_partials, float max_norm, float grad_scale, float lr,
                                float beta1, float beta2, float eps, float weight_decay, int step, int variant,
                                int zero_grad, float* norm_out, vlpet_stream_t stream) {
    if (!p || !g || !m || !v || !partials) return VLPET_E_NULL;
    if (n <= 0 || n_partials <= 0 || step <= 0 || (variant != 0 && variant != 1)) return VLPET_E_SHAPE;
    if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v) || (decay_mask && ((uintptr_t)decay_mask & 3)))
        return VLPET_E_ALIGN;
    AdamwArgs a;
    a.p = p; a.g = g; a.m = m; a.v = v; a.decay = decay_mask; a.n = n; a.partials = partials; a.n_partials = n_partials;
    a.max_norm = max_norm; a.grad_scale = grad_scale; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    a.weight_decay = weight_decay;
    a.bias_c1 = (float)(1.0 - pow((double)beta1, (double)step));
    a.bias_c2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    a.decay_first = variant == 1; a.eps_scaled = variant == 1; a.zero_grad = zero_grad; a.norm_out = norm_out;
    a.slice_of = nullptr; a.slice_bc = nullptr;
    return herr(launch_adamw(a, (hipStream_t)stream));
}

extern "C" int vlpet_adamw_step_sliced(float* p, float* g, float* m, float* v, const uint8_t* decay_mask, int64_t n,
                                       const float* partials, int n_partials, float max_norm, float grad_scale, float lr,
                                       float beta1, float beta2, float eps, float weight_decay, const int32_t* slice_of,
                                       const float* slice_bc, int variant, int zero_grad, float* norm_out,
                                       vlpet_stream_t stream) {
    if (!p || !g || !m || !v || !partials || !slice_of || !slice_bc) return VLPET_E_NULL;
    if (n <= 0 || n_partials <= 0 || (variant != 0 && variant != 1)) return VLPET_E_SHAPE;
    if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v) || !aligned16(slice_of) ||
        (decay_mask && ((uintptr_t)decay_mask & 3)))
        return VLPET_E_ALIGN;
    AdamwArgs a;
    a.p = p; a.g = g; a.m = m; a.v = v; a.decay = decay_mask; a.n = n; a.partials = partials; a.n_partials = n_partials;
    a.max_norm = max_norm; a.grad_scale = grad_scale; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    a.weight_decay = weight_decay; a.bias_c1 = 1.f; a.bias_c2_sqrt = 1.f;
    a.decay_first = variant == 1; a.eps_scaled = variant == 1; a.zero_grad = zero_grad; a.norm_out = norm_out;
    a.slice_of = slice_of; a.slice_bc = slice_bc;
    return herr(launch_adamw(a, (hipStream_t)stream));
}

// ---- sequential adapter + residual + norm, inference form (adapter_tail.hip)
extern "C" int vlpet_adapter_tail_rows(void) { return adapter_tail_rows(); }

extern "C" int vlpet_adapter_tail_applies(int64_t M, int d, int r, int io_dtype) {
    return (M > 0 && (M + adapter_tail_rows() - 1) / adapter_tail_rows() <= 0x7fffffffLL && adapter_tail_geometry_ok(d, r) && dtype_ok(io_dtype)) ? 1 : 0;
}

static inline bool ranges_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

extern "C" int vlpet_adapter_tail_fwd(const void* h, const void* res, const void* down_w, const void* down_b, const void* up_w,
                                      const void* up_b, const float* gamma, const float* beta, void* out, int64_t M, int d, int r,
                                      float scale, float eps, int norm_mode, int param_dtype, int io_dtype, vlpet_stream_t stream) {
    if (!h || !res || !down_w || !down_b || !up_w || !up_b || !out) return VLPET_E_NULL;
    if (norm_mode != 0 && norm_mode != 1) return VLPET_E_SHAPE;
    if (norm_mode == 1 && !gamma) return VLPET_E_NULL;
    if (!dtype_ok(io_dtype) || !dtype_ok(param_dtype)) return VLPET_E_DTYPE;
    if (M <= 0 || d <= 0 || r <= 0) return VLPET_E_SHAPE;
    if (!adapter_tail_geometry_ok(d, r)) return VLPET_E_RANK;
    if (!vlpet_adapter_tail_applies(M, d, r, io_dtype)) return VLPET_E_SHAPE;
    if (!aligned16(h) || !aligned16(res) || !aligned16(down_w) || !aligned16(down_b) || !aligned16(up_w) || !aligned16(up_b) ||
        !aligned16(out) || (norm_mode == 1 && (!aligned16(gamma) || (beta && !aligned16(beta))))) return VLPET_E_ALIGN;
    const size_t bytes = (size_t)M * d * (io_dtype == VLPET_F32 ? 4 : 2);
    if (ranges_overlap(out, h, bytes) || ranges_overlap(out, res, bytes)) return VLPET_E_ALIAS;
    AdapterTailArgs a{};
    a.h = h; a.res = res; a.wd = down_w; a.bd = down_b; a.wu = up_w; a.bu = up_b; a.gamma = gamma; a.beta = beta; a.out = out;
    a.M = M; a.d = d; a.r = r; a.scale = scale; a.eps = eps; a.norm = norm_mode;
    return herr(launch_adapter_tail(a, io_dtype == VLPET_F32, param_dtype == VLPET_F32, (hipStream_t)stream));
}

// ---- Compacter: PHM weight expansion of one adapter's (down, up) pair and its backward (phm.hip)
static int phm_geometry(int d, int r, int n) {
    if (n < 1 || n > 8) return VLPET_E_RANK;
    if (d < n || r < n || d % n != 0 || r % n != 0) return VLPET_E_SHAPE;
    if (phm_layer_tiles(d, r, n) + phm_layer_tiles(r, d, n) > 0x7fffffffLL) return VLPET_E_SHAPE;
    return 0;
}
static inline size_t phm_ws_bytes(int d, int r, int n) {
    return align256((size_t)(phm_layer_tiles(d, r, n) + phm_layer_tiles(r, d, n)) * n * n * n * sizeof(float));
}
extern "C" size_t vlpet_phm_workspace_bytes(int d, int r, int n) { return phm_geometry(d, r, n) == 0 ? phm_ws_bytes(d, r, n) : 0; }

struct ByteRange { const void* p; size_t bytes; };
// every output against every input and every later output
static bool phm_outputs_alias(const ByteRange* in, int n_in, const ByteRange* out, int n_out) {
    for (int o = 0; o < n_out; ++o) {
        const uintptr_t x = reinterpret_cast<uintptr_t>(out[o].p);
        for (int i = 0; i < n_in + n_out; ++i) {
            if (i >= n_in && i - n_in <= o) continue;
            const ByteRange& q = i < n_in ? in[i] : out[i - n_in];
            const uintptr_t y = reinterpret_cast<uintptr_t>(q.p);
            if (x < y + q.bytes && y < x + out[o].bytes) return true;
        }
    }
    return false;
}

extern "C" int vlpet_phm_expand_pair_fwd(const void* rule_d, const void* W_d, const void* rule_u, const void* W_u, void* wt_d, void* wt_u,
                                         int d, int r, int n, int param_dtype, vlpet_stream_t stream) {
    if (!rule_d || !W_d || !rule_u || !W_u || !wt_d || !wt_u) return VLPET_E_NULL;
    if (!dtype_ok(param_dtype)) return VLPET_E_DTYPE;
    if (int rc = phm_geometry(d, r, n)) return rc;
    if (!aligned16(rule_d) || !aligned16(W_d) || !aligned16(rule_u) || !aligned16(W_u) || !aligned16(wt_d) || !aligned16(wt_u))
        return VLPET_E_ALIGN;
    const size_t es = param_dtype == VLPET_F32 ? 4 : 2, nr = (size_t)n * n * n * es, nw = (size_t)d * r / n * es, nh = (size_t)d * r * es;
    const ByteRange in[4] = {{rule_d, nr}, {W_d, nw}, {rule_u, nr}, {W_u, nw}}, out[2] = {{wt_d, nh}, {wt_u, nh}};
    if (phm_outputs_alias(in, 4, out, 2)) return VLPET_E_ALIAS;
    PhmArgs a{};
    a.l[0].rule = rule_d; a.l[0].W = W_d; a.l[0].wt = wt_d; a.l[0].in = d; a.l[0].out = r;
    a.l[1].rule = rule_u; a.l[1].W = W_u; a.l[1].wt = wt_u; a.l[1].in = r; a.l[1].out = d;
    a.n = n;
    return herr(launch_phm_expand_fwd(a, param_dtype == VLPET_F32, (hipStream_t)stream));
}

extern "C" int vlpet_phm_expand_pair_bwd(const float* dwt_d, const float* dwt_u, const void* rule_d, const void* W_d, const void* rule_u,
                                         const void* W_u, float* drule_d, float* dW_d, float* drule_u, float* dW_u, void* workspace,
                                         size_t workspace_bytes, int d, int r, int n, int param_dtype, vlpet_stream_t stream) {
    if (!dwt_d || !dwt_u || !rule_d || !W_d || !rule_u || !W_u || !drule_d || !dW_d || !drule_u || !dW_u || !workspace) return VLPET_E_NULL;
    if (!dtype_ok(param_dtype)) return VLPET_E_DTYPE;
    if (int rc = phm_geometry(d, r, n)) return rc;
    if (!aligned16(dwt_d) || !aligned16(dwt_u) || !aligned16(rule_d) || !aligned16(W_d) || !aligned16(rule_u) || !aligned16(W_u) ||
        !aligned16(drule_d) || !aligned16(dW_d) || !aligned16(drule_u) || !aligned16(dW_u) || !aligned16(workspace)) return VLPET_E_ALIGN;
    const size_t need = phm_ws_bytes(d, r, n);
    if (workspace_bytes < need) return VLPET_E_WORKSPACE;
    const size_t es = param_dtype == VLPET_F32 ? 4 : 2, n3 = (size_t)n * n * n, nw = (size_t)d * r / n, nh = (size_t)d * r;
    const ByteRange in[6] = {{dwt_d, nh * 4}, {dwt_u, nh * 4}, {rule_d, n3 * es}, {W_d, nw * es}, {rule_u, n3 * es}, {W_u, nw * es}};
    const ByteRange out[5] = {{drule_d, n3 * 4}, {dW_d, nw * 4}, {drule_u, n3 * 4}, {dW_u, nw * 4}, {workspace, need}};
    if (phm_outputs_alias(in, 6, out, 5)) return VLPET_E_ALIAS;
    PhmArgs a{};
    a.l[0].rule = rule_d; a.l[0].W = W_d; a.l[0].dwt = dwt_d; a.l[0].drule = drule_d; a.l[0].dW = dW_d; a.l[0].in = d; a.l[0].out = r;
    a.l[1].rule = rule_u; a.l[1].W = W_u; a.l[1].dwt = dwt_u; a.l[1].drule = drule_u; a.l[1].dW = dW_u; a.l[1].in = r; a.l[1].out = d;
    a.n = n; a.ws = reinterpret_cast<float*>(workspace);
    return herr(launch_phm_expand_bwd(a, param_dtype == VLPET_F32, (hipStream_t)stream));
}

// ---- Hyperformer: one stack's weight generator (S linear maps on the same E embedding rows) and its backward (hyper.hip)
// -> 0 and the workgroups of every map's row slabs (blk0[s]: the first of map s), or VLPET_E_SHAPE
static int hyper_geometry(int S, const int* n, int E, int P, int* blk0, int64_t* blocks) {
    if (S < 1 || S > HYP_MAX_S || E < 1 || E > HYP_MAX_E || P < 1 || P > HYP_MAX_P || S * E > HYP_MAX_ROWPTRS) return VLPET_E_SHAPE;
    int64_t b = 0;
    for (int s = 0; s < S; ++s) {
        if (n[s] < 1) return VLPET_E_SHAPE;
        if (blk0) blk0[s] = (int)b;
        b += ((int64_t)n[s] + HYP_ROWS - 1) / HYP_ROWS;
        if (b > 0x7fffffffLL / (HYP_MAX_E * HYP_MAX_P)) return VLPET_E_SHAPE;
    }
    *blocks = b;
    return 0;
}
extern "C" size_t vlpet_hyper_gen_workspace_bytes(int S, const int* n, int E, int P) {
    int64_t blocks = 0;
    if (!n || hyper_geometry(S, n, E, P, nullptr, &blocks) != 0) return 0;
    return align256((size_t)blocks * E * P * sizeof(float));
}

extern "C" int vlpet_hyper_gen_fwd(int S, const void* const* G, const void* const* g, const int* n, const float* e, int E, int P,
                                   void* const* out, int param_dtype, vlpet_stream_t stream) {
    if (!G || !g || !n || !e || !out) return VLPET_E_NULL;
    if (S >= 1 && S <= HYP_MAX_S)
        for (int s = 0; s < S; ++s)
            if (!G[s] || !g[s] || !out[s]) return VLPET_E_NULL;
    if (!dtype_ok(param_dtype)) return VLPET_E_DTYPE;
    HyperFwdArgs a{};
    int blk0[HYP_MAX_S];
    int64_t blocks = 0;
    if (int rc = hyper_geometry(S, n, E, P, blk0, &blocks)) return rc;
    if (!aligned16(e)) return VLPET_E_ALIGN;
    for (int s = 0; s < S; ++s)
        if (!aligned16(G[s]) || !aligned16(g[s]) || !aligned16(out[s])) return VLPET_E_ALIGN;
    const size_t es = param_dtype == VLPET_F32 ? 4 : 2;
    ByteRange in[2 * HYP_MAX_S + 1], o[HYP_MAX_S];
    for (int s = 0; s < S; ++s) {
        in[2 * s] = {G[s], (size_t)n[s] * P * es};
        in[2 * s + 1] = {g[s], (size_t)n[s] * es};
        o[s] = {out[s], (size_t)E * n[s] * es};
    }
    in[2 * S] = {e, (size_t)E * P * 4};
    if (phm_outputs_alias(in, 2 * S + 1, o, S)) return VLPET_E_ALIAS;
    for (int s = 0; s < S; ++s) a.m[s] = {G[s], g[s], out[s], n[s], blk0[s]};
    a.e = e; a.S = S; a.E = E; a.P = P;
    return herr(launch_hyper_gen_fwd(a, (int)blocks, param_dtype == VLPET_F32, (hipStream_t)stream));
}

extern "C" int vlpet_hyper_gen_bwd(int S, const float* const* dout, const void* const* G, const int* n, const float* e, int E, int P,
                                   float* const* dG, float* const* dg, float* de, void* workspace, size_t workspace_bytes,
                                   int param_dtype, vlpet_stream_t stream) {
    if (!dout || !G || !n || !e || !dG || !dg || !de || !workspace) return VLPET_E_NULL;
    if (S >= 1 && S <= HYP_MAX_S)
        for (int s = 0; s < S; ++s)
            if (!G[s] || !dG[s] || !dg[s]) return VLPET_E_NULL;
    if (!dtype_ok(param_dtype)) return VLPET_E_DTYPE;
    int blk0[HYP_MAX_S];
    int64_t blocks = 0;
    if (int rc = hyper_geometry(S, n, E, P, blk0, &blocks)) return rc;
    if (!aligned16(e) || !aligned16(de) || !aligned16(workspace)) return VLPET_E_ALIGN;
    for (int s = 0; s < S; ++s)
        if (!aligned16(G[s]) || !aligned16(dG[s]) || !aligned16(dg[s])) return VLPET_E_ALIGN;
    for (int k = 0; k < S * E; ++k)
        if (reinterpret_cast<uintptr_t>(dout[k]) & 3) return VLPET_E_ALIGN;
    const size_t need = align256((size_t)blocks * E * P * sizeof(float));
    if (workspace_bytes < need) return VLPET_E_WORKSPACE;
    const size_t es = param_dtype == VLPET_F32 ? 4 : 2;
    ByteRange in[HYP_MAX_ROWPTRS + HYP_MAX_S + 1], o[2 * HYP_MAX_S + 2];
    int n_in = 0, n_out = 0;
    for (int s = 0; s < S; ++s) {
        for (int l = 0; l < E; ++l)
            if (dout[s * E + l]) in[n_in++] = {dout[s * E + l], (size_t)n[s] * 4};
        in[n_in++] = {G[s], (size_t)n[s] * P * es};
        o[n_out++] = {dG[s], (size_t)n[s] * P * 4};
        o[n_out++] = {dg[s], (size_t)n[s] * 4};
    }
    in[n_in++] = {e, (size_t)E * P * 4};
    o[n_out++] = {de, (size_t)E * P * 4};
    o[n_out++] = {workspace, need};
    if (phm_outputs_alias(in, n_in, o, n_out)) return VLPET_E_ALIAS;
    HyperBwdArgs a{};
    for (int s = 0; s < S; ++s) a.m[s] = {G[s], dG[s], dg[s], n[s], blk0[s]};
    for (int k = 0; k < S * E; ++k) a.dout[k] = dout[k];
    a.e = e; a.de = de; a.ws = reinterpret_cast<float*>(workspace); a.S = S; a.E = E; a.P = P;
    return herr(launch_hyper_gen_bwd(a, (int)blocks, param_dtype == VLPET_F32, (hipStream_t)stream));
}
