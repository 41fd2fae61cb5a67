// The six compilations of the FK20 proofs map the engine runs (g1_linmap.hpp compiles, k_g1slp.hip executes): which strategy each
// one is built with, the order its outputs leave in, and which of them carries fused a + b / a - b pairs.  Free of HIP: the engine
// (engine.hip: build_slp_program) and the host dump of the programs (tests/c/dump_linmap.cpp) both take the programs from here, so
// what the tests model on the CPU is what the device is given.
#pragma once
#include "g1_linmap.hpp"

namespace kzg {
namespace linmap {

constexpr int SLP_PROGRAM_COUNT = 6;  // Engine::SlpProgramId: 0 tuned with fused pairs, 1 tuned, 2 Karatsuba, 3 (456), 4 (606), 5 (372)

inline Strategy slp_strategy(int id) {
    Strategy s;
    s.allow_toom8 = true;
    s.lambda = glv_lambda();  // phi = [lambda] with the lambda the constants are GLV-recoded with: the device's beta was picked to match it (init_srs)
    auto fixed = [&](int k4, int k8, int k16, int k32) {
        s.tuned = false;
        s.balanced_lincomb = true;
        s.phi = false;  // the real Toom-Cook points these depth-optimised programs were measured with
        s.hankel_split = {{2, 2}, {4, k4}, {8, k8}, {16, k16}, {32, k32}};
    };
    // (tools/linmap_explore.cpp lists every assignment of splits with its multiplication count and the latency of its cheap
    // levels; these are points of that Pareto front)
    switch (id) {
        case 2: fixed(2, 2, 2, 2); break;  // Karatsuba throughout: 712 multiplications, 13 levels of single additions
        case 3: fixed(4, 2, 4, 2); break;  // 456 multiplications, 18 levels, at most two doublings in front of an addition
        case 4: fixed(2, 2, 2, 4); break;  // 606 multiplications, 15 levels
        case 5: fixed(4, 2, 4, 8); break;  // 372 multiplications, 19 levels (8-way split of the 32-point products only)
        default: break;                    // tuned by operation count, Toom-Cook points on mu_6: 298 multiplications (16-way splits)
    }
    return s;
}

inline int bit_reverse7(int p) {
    int k = 0;
    for (int b = 0; b < 7; b++) k |= ((p >> b) & 1) << (6 - b);
    return k;
}

struct SlpCompiled {
    Plan plan;       // outputs already in the order the executor leaves them
    Schedule sched;
};
// Program `id` over w128[e] = omega_128^e (Montgomery form): the plan with its outputs permuted, and its slot program.
inline SlpCompiled compile_slp_program(const std::vector<Fr>& w128, int id, bool verbose = false) {
    SlpCompiled c;
    c.plan = build_fk20_proofs_plan(w128, slp_strategy(id), verbose);
    {   // the executor leaves output p in arena slot 128 + p, and the proofs are wanted in bit-reversed FFT order
        std::vector<Ref> perm(128);
        for (int p = 0; p < 128; p++) perm[p] = c.plan.outputs[bit_reverse7(p)];
        c.plan.outputs = perm;
    }
    // a + b / a - b pairs as ONE operation only in the large-batch schedule: for batches that leave the chip part empty a
    // step lasts as long as its longest operation, and the fused pair is 15 % longer than an addition (64 blobs: 2.65 against
    // 2.73 ms for the map; 2048 blobs: 16.15 against 16.0 ms -- fewer, fuller rounds win there)
    c.sched = make_schedule(c.plan, /*fuse_add_sub=*/id == 0);
    return c;
}

}  // namespace linmap
}  // namespace kzg
