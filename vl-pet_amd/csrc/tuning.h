// Experiment switches of the kernels: the four that the tests and tools still use (the retired ones: DESIGN.md, "switches retired").
// The product library reads NOTHING from the environment: every switch below is a constant.  Only a diagnosis build
// (make DEBUG=1: -DVLPET_DEBUG, what tools/ uses for same-box A/Bs and what the tests of the alternatives ask for via
// vlpet_debug_build()) fills the table from VLPET_* variables, once, when the library is loaded.
#pragma once
#include <cstdlib>

struct VlpetTuning {
    int rg = 0;             // VLPET_RG: force the row groups per workgroup of the row kernels (0: pick_row_groups)
    int fwd2p = -1;         // VLPET_FWD2P: gated forward of the training form: -1 by shape (k1_fwd2p_preferred), 0 one-kernel (pet_gate_fwd.hip), 1 two-pass
                            //   (pet_fwd2p.hip), 2 = pass A only, 3 = pass B only (timing)
    int dz6 = 1;            // VLPET_DZ6=0: pet_gate_dz_kernel instead of the four-wave feature-split pass 1 at six tiles; 2: that pass at every size
    int dbg = 0;            // VLPET_DBG: ablation / stamp bits
};

#ifdef VLPET_DEBUG
inline const VlpetTuning& vlpet_tuning() {
    static const VlpetTuning t = [] {
        VlpetTuning v;
        auto rd = [](const char* n, int& dst) { if (const char* e = getenv(n)) dst = atoi(e); };
        rd("VLPET_RG", v.rg); rd("VLPET_FWD2P", v.fwd2p); rd("VLPET_DZ6", v.dz6); rd("VLPET_DBG", v.dbg);
        return v;
    }();
    return t;
}
#define VLPET_IS_DEBUG_BUILD 1
#else
inline const VlpetTuning& vlpet_tuning() { static const VlpetTuning t{}; return t; }
#define VLPET_IS_DEBUG_BUILD 0
#endif
