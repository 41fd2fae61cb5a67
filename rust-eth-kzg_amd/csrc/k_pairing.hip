// k_pairing_check: MANY pairing checks e(P0, key0) e(P1, key1) == 1 in one launch, one check per lane, for the search of the
// many-verifications for their wrong entries (vm_search.hpp).  The pairs are the folds k_vm_fold_ranges has just left in HBM, both G2
// arguments are fixed per context, so every lane of every wave walks the SAME 2 x 68 prepared lines (scalar loads) in the same
// order: the bits of |x| are public and an identity point is a select (pairing_tower.hpp: miller_loop_lines), never a branch.  The
// arithmetic is pairing_tower.hpp's, the statement the host's checks compile too; with the points made affine first (one binary-GCD
// inversion each, under a tenth of the work) a lane's Miller value equals the host's bit for bit.
// One wave per block: a check is ~16 k Fp multiplications in one dependent chain per lane, a batch of the search is at most a few
// thousand checks, and 64-lane blocks spread them over the most CUs.  Lanes behind the last check repeat its work and store nothing
// (a wave with few live lanes runs no faster).
#include "pairing_tower.hpp"
#include "launch.hpp"
#include "hip_check.hpp"

namespace kzg {

using pairing::Fp12;
using pairing::FrobConsts;
using pairing::Line;

__global__ __launch_bounds__(64) void k_pairing_check(const JacQ* __restrict__ pairs /*[n][2]*/, const Line* __restrict__ key0,
                                                      const Line* __restrict__ key1, const FrobConsts* __restrict__ fc,
                                                      int8_t* __restrict__ verdict, int n, Fp12* __restrict__ miller /*[n], test hook; else null*/) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    const int j = live ? i : n - 1;
    const int v = pairing::check_lane(pairs + 2 * (size_t)j, key0, key1, *fc, live && miller ? miller + j : nullptr);
    if (live) verdict[i] = (int8_t)v;
}

namespace launch {
void pairing_check(const void* pairs, const void* key0, const void* key1, const void* frob, int8_t* verdict, int n, hipStream_t st, void* miller) {
    if (n <= 0) return;
    k_pairing_check<<<(n + 63) / 64, 64, 0, st>>>((const JacQ*)pairs, (const Line*)key0, (const Line*)key1, (const FrobConsts*)frob, verdict, n,
                                                  (Fp12*)miller);
    HIPCK(hipGetLastError());
}
}  // namespace launch

}  // namespace kzg
