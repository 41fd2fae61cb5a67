// What the passes of the many-verifications share on the host (verify_many.hip: cell proofs per problem; point_many.hip: point proofs
// per item): the size of the host thread pool, the pairing check of a pair read back, and the SEARCH for the wrong entries of a pass
// whose folded check failed.  Where a batch of the search's probes is large enough (GPU_PAIRING_MIN_DEFAULT / the knob), their pairings run
// on the GPU, one per lane (k_pairing.hip), on the folds where k_vm_fold_ranges left them: wrong entries everywhere would otherwise keep
// every host thread busy for n / T pairings of 0.85 ms.  A launch takes 43 ms whatever it holds (up to 65536 checks), 1024 checks on 16
// host threads 57 ms: that is where the default lies.
#pragma once
#include "engine_internal.hpp"
#include "curve29.hpp"
#include "host_pairing.hpp"

#include <functional>

namespace kzg {
namespace vm {

inline int host_threads(const Knobs& k) {
    int t = 16;
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw && (int)hw < t) t = (int)hw;
    if (k.host_threads) t = k.host_threads;
    return t;
}
// the pairing check of two sums read back against vk: 1 / 0, or -1 where the poison of the result slots is still there (a device failure)
inline bool poisoned(const JacQ& s) { return pairing::poisoned(s); }
inline int check_pair(const JacQ* two, const pairing::G2Prepared* const* vk) {
    G1Affine pts[2];
    for (int j = 0; j < 2; j++) {
        if (poisoned(two[j])) return -1;
        pts[j] = to_affine(jac_from_jacq(two[j]));
    }
    return pairing::product_is_one(pts, vk, 2) ? 1 : 0;
}

// The smallest batch of probes whose pairings go to the GPU when ETH_KZG_AMD_GPU_PAIRING_MIN is not set: the measured crossover against
// 16 host threads (profiles/pairing_search.json)
constexpr int GPU_PAIRING_MIN_DEFAULT = 1024;
// What k_pairing_check needs of a context (engine.hpp: d_pairing_), for the pass's pair of keys.  min_probes 0: every probe on the host
struct DevicePairing {
    const void *key0 = nullptr, *key1 = nullptr, *frob = nullptr;
    int min_probes = 0;
};

// A pass as the search sees it: n entries whose weighted pairs rho_b * pair_b are resident in HBM ([n][2] JacQ at db + off_pairs), range
// buffers for max_ranges probes on both sides (device: off_rng, off_rsum; pinned: poff_rng, poff_rsum).
struct SearchView {
    int n = 0, max_ranges = 0, T = 1;
    HostPool* pool = nullptr;
    uint8_t* hb = nullptr;
    size_t poff_rng = 0, poff_rsum = 0, off_rng = 0, off_pairs = 0, off_rsum = 0;
    DevicePairing gpu;                     // probes in batches of gpu.min_probes or more are checked by k_pairing_check ...
    size_t off_verd = 0, poff_verd = 0;    // ... which leaves max_ranges verdict bytes here (device) that come down to here (pinned)
    const pairing::G2Prepared* const* vk = nullptr;
    const char* live = nullptr;            // entries that take part
    int* verified = nullptr;               // the verdicts of the live entries
    std::atomic<int>* device_fault = nullptr;
    // the end of the search, when few entries are left or wrong ones are everywhere: every live suspect on its own.  Set: the pass has its
    // pairs on the host and checks each there; null: single-entry probes, like every other probe
    std::function<void(int)> check_single;
    // taps (null in the product): the probes in order (lo, hi, passed) and their pairs
    std::vector<int>* tap_probes = nullptr;
    std::vector<uint8_t>* tap_probe_sums = nullptr;
    int* tap_device_probes = nullptr;      // how many probes k_pairing_check judged
};
// The view of a pass of n entries laid out by L (PassLayout, PointPassLayout: the search's buffers go by the same names in both), its
// weighted pairs at off_pairs; check_single and the taps are the caller's to add
template <class Layout>
inline SearchView search_view(const Layout& L, int n, size_t off_pairs, int T, HostPool* pool, uint8_t* hb, const pairing::G2Prepared* const* vk,
                              const DevicePairing& gpu, const char* live, int* verified, std::atomic<int>* device_fault) {
    SearchView S;
    S.n = n; S.max_ranges = L.max_ranges; S.T = T; S.pool = pool; S.hb = hb;
    S.poff_rng = L.poff_rng; S.poff_rsum = L.poff_rsum; S.poff_verd = L.poff_verd;
    S.off_rng = L.off_rng; S.off_pairs = off_pairs; S.off_rsum = L.off_rsum; S.off_verd = L.off_verd;
    S.gpu = gpu; S.vk = vk; S.live = live; S.verified = verified; S.device_fault = device_fault;
    return S;
}

// Some entry of the pass is wrong.  SEARCH for the wrong ones by folding sub-ranges of the resident weighted pairs (k_vm_fold_ranges: one
// small launch per level) and checking each with one pairing on a host thread -- a range whose fold passes holds only valid entries
// (the 2^-127 argument of the fold: the weights were fixed after every input byte), a single entry whose weighted pair fails is wrong
// EXACTLY (rho_b != 0 and the pairing group has prime order).  Ranges are split K ways with K chosen so that a level's probes fill the
// host threads once: one wrong proof among 1024 costs ~36 pairings in 3 rounds instead of 1024 in 64 (round 3: 85 ms per call against
// 29.6 ms for an all-valid one).  When wrong proofs are many the search stops paying: from a quarter of the live entries suspect, the
// rest is checked one by one.
inline void search_wrong_proofs(const SearchView& V, int n_live, uint8_t* db, hipStream_t st) {
    const int T = V.T;
    uint8_t* const hb = V.hb;
    std::vector<std::pair<int, int>> suspects{{0, V.n}};
    int* h_rng = (int*)(hb + V.poff_rng);
    const JacQ* h_rsum = (const JacQ*)(hb + V.poff_rsum);
    // one level's probes -> fails.  A level may need more probes than the range buffers hold (e.g. > 4096 small problems with > 1024
    // scattered wrong proofs): it then runs in batches over the same buffers -- never an error, the valid entries of the pass keep
    // their verdicts
    // record: the probes go into the tap (all but the probes that stand in for check_single, which never did)
    auto run_probes = [&](const std::vector<std::pair<int, int>>& probes, std::vector<char>& fails, bool record = true) {
        fails.assign(probes.size(), 0);
        for (size_t q0 = 0; q0 < probes.size() && !V.device_fault->load(); q0 += (size_t)V.max_ranges) {
            const size_t cnt = std::min(probes.size() - q0, (size_t)V.max_ranges);
            const bool on_gpu = V.gpu.min_probes > 0 && cnt >= (size_t)V.gpu.min_probes;
            const bool sums_down = !on_gpu || (record && V.tap_probes);
            for (size_t q = 0; q < cnt; q++) { h_rng[2 * q] = probes[q0 + q].first; h_rng[2 * q + 1] = probes[q0 + q].second; }
            memset(hb + V.poff_rsum, 0xff, cnt * 2 * launch::SIZEOF_JACQ);
            HIPCK(hipMemcpyAsync(db + V.off_rng, h_rng, cnt * 8, hipMemcpyHostToDevice, st));
            if (on_gpu) HIPCK(hipMemsetAsync(db + V.off_rsum, 0xff, cnt * 2 * launch::SIZEOF_JACQ, st));  // (the host's copy is poisoned above)
            launch::vm_fold_ranges(db + V.off_pairs, (const int*)(db + V.off_rng), db + V.off_rsum, (int)cnt, st);
            int8_t* const h_verd = (int8_t*)(hb + V.poff_verd);
            if (on_gpu) {
                memset(h_verd, 0xff, cnt);  // -1: no verdict came down
                launch::pairing_check(db + V.off_rsum, V.gpu.key0, V.gpu.key1, V.gpu.frob, (int8_t*)(db + V.off_verd), (int)cnt, st);
                HIPCK(hipMemcpyAsync(h_verd, db + V.off_verd, cnt, hipMemcpyDeviceToHost, st));
            }
            if (sums_down) HIPCK(hipMemcpyAsync(hb + V.poff_rsum, db + V.off_rsum, cnt * 2 * launch::SIZEOF_JACQ, hipMemcpyDeviceToHost, st));
            SYNC_CHECKED(st);
            if (on_gpu) {
                for (size_t q = 0; q < cnt; q++) {
                    if (h_verd[q] != 0 && h_verd[q] != 1) V.device_fault->store(1);
                    else fails[q0 + q] = h_verd[q] ? 0 : 1;
                }
                if (V.tap_device_probes) *V.tap_device_probes += (int)cnt;
            } else {
                parallel_for((int)cnt, T, V.pool, [&](int q) {
                    const int v = check_pair(h_rsum + 2 * (size_t)q, V.vk);
                    if (v < 0) V.device_fault->store(1);
                    else fails[q0 + q] = v ? 0 : 1;
                });
            }
            if (record && V.tap_probes && !V.device_fault->load()) {
                for (size_t q = 0; q < cnt; q++) {
                    const int rec[3] = {probes[q0 + q].first, probes[q0 + q].second, fails[q0 + q] ? 0 : 1};
                    V.tap_probes->insert(V.tap_probes->end(), rec, rec + 3);
                }
                V.tap_probe_sums->insert(V.tap_probe_sums->end(), hb + V.poff_rsum, hb + V.poff_rsum + cnt * 2 * launch::SIZEOF_JACQ);
            }
        }
    };
    while (!suspects.empty()) {
        long suspect_entries = 0;
        for (auto& sr : suspects) suspect_entries += sr.second - sr.first;
        if ((long)suspects.size() * 4 >= n_live || suspect_entries <= 2 * T) {  // few entries left, or wrong proofs everywhere
            std::vector<int> todo;
            for (auto& sr : suspects)
                for (int i = sr.first; i < sr.second; i++)
                    if (V.live[i]) todo.push_back(i);
            // (enough of them for the GPU: single-entry probes over the resident weighted pairs also where the pass could check on the
            // host -- an entry's weighted pair passes exactly when its own pair does, rho_b != 0)
            if (V.check_single && !(V.gpu.min_probes > 0 && (int)todo.size() >= V.gpu.min_probes)) {
                parallel_for((int)todo.size(), T, V.pool, [&](int q) { V.check_single(todo[q]); });
            } else {
                std::vector<std::pair<int, int>> singles;
                for (int i : todo) singles.emplace_back(i, i + 1);
                std::vector<char> fails;
                run_probes(singles, fails, /*record=*/!V.check_single);
                if (V.device_fault->load()) break;
                for (size_t q = 0; q < todo.size(); q++) V.verified[todo[q]] = fails[q] ? 0 : 1;
            }
            break;
        }
        int K = T / (int)suspects.size();
        K = K < 2 ? 2 : K > 16 ? 16 : K;
        std::vector<std::pair<int, int>> probes;
        for (auto& sr : suspects) {
            const int len = sr.second - sr.first, parts = std::min(K, len);
            for (int q = 0; q < parts; q++) probes.emplace_back(sr.first + (int)((long)len * q / parts), sr.first + (int)((long)len * (q + 1) / parts));
        }
        std::vector<char> fails;
        run_probes(probes, fails);
        if (V.device_fault->load()) break;
        suspects.clear();
        for (size_t q = 0; q < probes.size(); q++) {
            const int lo = probes[q].first, hi = probes[q].second;
            if (!fails[q]) {
                for (int i = lo; i < hi; i++) if (V.live[i]) V.verified[i] = 1;
            } else if (hi - lo == 1) {
                V.verified[lo] = 0;  // exact: its own weighted pair fails the check
            } else {
                suspects.emplace_back(lo, hi);
            }
        }
    }
}

}  // namespace vm
}  // namespace kzg
