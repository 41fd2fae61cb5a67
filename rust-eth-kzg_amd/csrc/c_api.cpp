// C ABI of the MI355X KZG engine: the reference's `eth_kzg_*` symbols (bindings/c/src/lib.rs) over
// kzg::Engine, plus the batched / device-resident `eth_kzg_amd_*` additions.  See include/c_eth_kzg.h.
//
// A context may span a DEVICE LIST (c_ctx.hpp): every entry point below first decides WHERE a call runs --
//   single-problem calls (the reference's sixteen symbols)   the least-loaded device (DevicePicker)
//   host-pointer batches (_batch, _many)                     contiguous slices, one per device (fan_out_slices)
//   device-resident forms (_device)                          the device that owns the caller's buffers
// -- and a one-device context takes none of these paths.
#include "../../include/c_eth_kzg.h"
#include "c_ctx.hpp"
#include "verify_host.hpp"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace {

constexpr int CELLS = 128;
// Batched entry points bound their count: the engine indexes blobs with `int`, and a count in the billions is a corrupted argument,
// not a workload (2^24 blobs are 2 TB of input).  Malformed input is `Err`, never a crash (bindings/c/src/lib.rs:272-280).
constexpr uint64_t MAX_BATCH = 1u << 24;

CResult ok() { return CResult{Ok, nullptr}; }
CResult err(const std::string& m) {  // CResult::with_error, bindings/c/src/lib.rs:146-153
    char* s = (char*)malloc(m.size() + 1);
    if (!s) return CResult{Err, nullptr};
    memcpy(s, m.c_str(), m.size() + 1);
    return CResult{Err, s};
}
const char* status_text(int st) {
    switch (st) {
        case kzg::ERR_SCALAR: return "Serialization(CouldNotDeserializeScalar)";
        case kzg::ERR_G1: return "Serialization(CouldNotDeserializeG1Point)";
        case kzg::ERR_INPUT: return "InvalidInput";
        case kzg::ERR_RECOVERY: return "Recovery(PolynomialHasInvalidLength)";
        default: return "DeviceError";
    }
}
const DASContext* live(const DASContext* ctx) {
    // `assert!(!ctx.is_null())` in the reference (e.g. compute_cells_and_kzg_proofs.rs:14): abort, like a Rust panic across FFI
    if (!ctx || !ctx->engine) {
        fprintf(stderr, "c_eth_kzg: context pointer is null\n");
        abort();
    }
    return ctx;
}
kzg::Engine* eng(const DASContext* ctx) { return live(ctx)->engine; }
std::string device_text(kzg::Engine* e) { return "DeviceError(" + e->last_error() + ")"; }
CResult device_err(kzg::Engine* e) { return err(device_text(e)); }

// where a single-problem call runs: the context's one engine, or the least-loaded device of its list.  `weight` = the call's size
// in units that compare across entry points (cells: a blob is 128 of them).
struct Picked {
    kzg::Engine* e;
    kzg::DevicePicker::Ticket ticket;
};
Picked pick(const DASContext* ctx, uint64_t weight) {
    live(ctx);
    auto t = ctx->picker->pick(weight ? weight : 1);
    return Picked{ctx->engines[(size_t)t.device()], std::move(t)};
}
// the engine whose GPU holds a device pointer of the caller (device-resident forms); NULL: none of the context's devices does
kzg::Engine* engine_of_pointer(const DASContext* ctx, const void* p) {
    live(ctx);
    if (ctx->engines.size() == 1 || !p) return ctx->engine;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    for (kzg::Engine* e : ctx->engines)
        if (e->device() == a.device) return e;
    return nullptr;
}
// the engine on whose GPU all of the pointers lie as device memory; NULL: they do not, or not on a device of this context
kzg::Engine* engine_of_device_pointers(const DASContext* ctx, const void* const* ptrs, int n_ptrs) {
    int dev = -1;
    for (int i = 0; i < n_ptrs; i++) {
        hipPointerAttribute_t a;
        if (!ptrs[i] || hipPointerGetAttributes(&a, ptrs[i]) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged) return nullptr;
        if (i && a.device != dev) return nullptr;
        dev = a.device;
    }
    for (kzg::Engine* e : ctx->engines)
        if (e->device() == dev) return e;
    return nullptr;
}
CResult slices_result(const DASContext* ctx, const std::pair<int, std::string>& r) {
    if (r.first < 0) return ok();
    if (ctx->engines.size() == 1) return err(r.second);
    return err("device " + std::to_string(ctx->engines[(size_t)r.first]->device()) + ": " + r.second);
}
// how a call that returns a Status ends; a verification also hands out its verdict when the status is OK
CResult finish(kzg::Engine* e, int st) {
    if (st == kzg::ERR_DEVICE) return device_err(e);
    return st ? err(status_text(st)) : ok();
}
CResult finish_verdict(kzg::Engine* e, int st, int ver, bool* verified) {
    if (!st) *verified = ver != 0;
    return finish(e, st);
}
// the verdicts and statuses of a many-verification into the caller's arrays
CResult verdicts_out(uint64_t n, const int* ver, const int* st, bool* verified, int32_t* status) {
    for (uint64_t i = 0; i < n; i++) {
        verified[i] = st[i] == 0 && ver[i] != 0;
        if (status) status[i] = st[i];
    }
    return ok();
}
std::string many_failure(kzg::Engine* e, int rc) { return rc == kzg::ERR_DEVICE ? device_text(e) : std::string(); }
std::string batch_failure(kzg::Engine* e, int rc) { return rc ? device_text(e) : std::string(); }
// A host-pointer batch of n items over the device list.  The count is checked before the context is looked at, args_ok() (null
// pointers) behind the empty call.  run(engine, lo, hi, st, ver) runs items [lo, hi) on a device's engine, fills their entries of
// the status (and verdict) words and returns "" or the slice's error text.  `verified` set: a many-verification, whose verdicts go out
// with the statuses; else a prover batch, whose statuses go out alone.
template <class ArgsOk, class Run>
CResult sliced_call(const DASContext* ctx, uint64_t n, uint64_t max_n, bool* verified, int32_t* status, ArgsOk args_ok, Run run) {
    if (n > max_n) return err("InvalidInput");
    live(ctx);
    if (n == 0) return ok();
    if (!args_ok()) return err("InvalidInput");
    try {
        std::vector<int> st(n), ver(verified ? n : 0);
        const auto r = kzg::fan_out_slices((int)ctx->engines.size(), n, [&](int d, uint64_t lo, uint64_t hi) -> std::string {
            return run(ctx->engines[(size_t)d], lo, hi, st.data(), ver.data());
        });
        if (r.first >= 0) return slices_result(ctx, r);
        if (verified) return verdicts_out(n, ver.data(), st.data(), verified, status);
        if (status) for (uint64_t i = 0; i < n; i++) status[i] = st[i];
        return ok();
    } catch (const std::exception& ex) {
        return err(std::string("DeviceError(") + ex.what() + ")");
    }
}
// verify_cell_kzg_proof_batch_many on a host source: by PROBLEM over the device list (each has its own transcript); no lane needed
CResult host_many(const DASContext* ctx, uint64_t n, uint64_t max_n, const kzg::VerifyManyInput& in, bool* verified, int32_t* status) {
    return sliced_call(ctx, n, max_n, verified, status, [] { return true; }, [&](kzg::Engine* e, uint64_t lo, uint64_t hi, int* st, int* ver) {
        return many_failure(e, e->verify_cell_kzg_proof_batch_many(hi - lo, in.from(lo), ver + lo, st + lo));
    });
}
// the same on a device source: on the one engine that owns the caller's buffers
CResult device_many(kzg::Engine* e, uint64_t n, const kzg::VerifyManyInput& in, bool* verified, int32_t* status) {
    try {
        std::vector<int> ver(n), st(n);
        if (e->verify_cell_kzg_proof_batch_many(n, in, ver.data(), st.data()) == kzg::ERR_DEVICE) return device_err(e);
        return verdicts_out(n, ver.data(), st.data(), verified, status);
    } catch (const std::exception& ex) {
        return err(std::string("DeviceError(") + ex.what() + ")");
    }
}

void free_ctx(DASContext* c) {
    if (!c) return;
    for (kzg::Engine* e : c->engines) delete e;
    delete c;
}
// the one constructor: NULL + message when the context cannot be built (no usable GPU, not even the 3.7 GB start tables fit).
// The engines of a device list are built side by side (a constructor is 0.1 - 2 s of set-up kernels and allocations per GPU).
DASContext* try_make_ctx(bool use_precomp, const std::vector<int>& devices, double table_budget_gb, std::string* why,
                         const std::shared_ptr<const kzg::TrustedSetup>& setup = nullptr) {
    DASContext* c = nullptr;
    try {
        if (devices.empty() || devices.size() > 64) throw std::runtime_error("empty or oversized device list");
        c = new DASContext;
        const size_t D = devices.size();
        c->engines.assign(D, nullptr);
        std::vector<std::string> errs(D);
        // Engines on DIFFERENT GPUs are built side by side (they share nothing but the mutex-guarded registries); entries that repeat
        // an ordinal -- the form the one-GPU tests use -- are built one after the other: the later one finds the tables the earlier
        // one has published.  (Same-GPU constructors side by side work as well -- the table registry is made for concurrent
        // constructors, tools/probe_concurrent_ctors.py -- but a list 0,0 built that way kept 1.4 GB of HBM after injected constructor
        // faults on two of the test boxes, which is not understood; the sequential order is the one the soaks have run on.)
        std::vector<size_t> first, again;  // entries that name a GPU for the first time / once more
        for (size_t d = 0; d < D; d++) {
            bool repeat = false;
            for (size_t k = 0; k < d; k++) repeat |= devices[k] == devices[d];
            (repeat ? again : first).push_back(d);
        }
        auto make = [&](const std::vector<size_t>& ds) {  // side by side
            const auto thrown = kzg::run_side_by_side((int)ds.size(), [&](int i) {
                c->engines[ds[(size_t)i]] = new kzg::Engine(use_precomp, devices[ds[(size_t)i]], nullptr, table_budget_gb, setup);
            });
            for (size_t i = 0; i < ds.size(); i++)
                if (thrown[i]) errs[ds[i]] = kzg::what_was_thrown(thrown[i], "", "unknown failure");
        };
        make(first);
        for (size_t d : again) make({d});
        for (size_t d = 0; d < D; d++)
            if (!c->engines[d]) throw std::runtime_error(D == 1 ? errs[d] : "device " + std::to_string(devices[d]) + ": " + errs[d]);
        c->engine = c->engines[0];
        c->picker.reset(new kzg::DevicePicker((int)D));
        return c;
    } catch (const std::exception& e) {
        free_ctx(c);
        if (why) *why = e.what();
        return nullptr;
    }
}
DASContext* make_ctx(bool use_precomp, const std::vector<int>& devices) {
    std::string why;
    DASContext* c = try_make_ctx(use_precomp, devices, 0, &why);
    if (!c) {
        // The reference panics when the context cannot be built (bad SRS); here: no usable GPU.  No CPU fallback.  A host that must
        // not die calls eth_kzg_amd_das_context_try_new instead.
        fprintf(stderr, "c_eth_kzg: cannot create the MI355X context: %s\n", why.c_str());
        abort();
    }
    return c;
}
std::vector<int> env_device_list() {  // ETH_KZG_AMD_DEVICES (a list, or "all"), else ETH_KZG_AMD_DEVICE, else GPU 0 -- read once per context
    const kzg::Knobs k = kzg::Knobs::from_env();
    if (k.devices.size() == 1 && k.devices[0] < 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
        std::vector<int> all;
        for (int d = 0; d < n; d++) all.push_back(d);
        if (all.empty()) all.push_back(0);  // (the constructor reports the missing GPU)
        return all;
    }
    if (!k.devices.empty()) return k.devices;
    return {k.device};
}

}  // namespace

extern "C" {

DASContext* eth_kzg_das_context_new(bool use_precomp) { return make_ctx(use_precomp, env_device_list()); }
DASContext* eth_kzg_amd_das_context_new_on_device(bool use_precomp, int device_ordinal) {
    return make_ctx(use_precomp, {device_ordinal});
}
DASContext* eth_kzg_amd_das_context_try_new(bool use_precomp, int device_ordinal, double table_budget_gb, CResult* result) {
    std::string why;
    DASContext* c = try_make_ctx(use_precomp, {device_ordinal}, table_budget_gb, &why);
    if (result) *result = c ? ok() : err("ContextCreation(" + why + ")");
    return c;
}
DASContext* eth_kzg_amd_das_context_new_on_devices(bool use_precomp, const int32_t* device_ordinals, uint64_t n_devices,
                                                   double table_budget_gb, CResult* result) {
    std::string why;
    DASContext* c = nullptr;
    if (!device_ordinals || n_devices == 0 || n_devices > 64) why = "InvalidInput: the device list holds 1 to 64 ordinals";
    else c = try_make_ctx(use_precomp, std::vector<int>(device_ordinals, device_ordinals + n_devices), table_budget_gb, &why);
    if (result) *result = c ? ok() : err("ContextCreation(" + why + ")");
    return c;
}
// A caller-supplied trusted setup.  Order of the checks: the arguments (no GPU needed, so a wrong count is reported as such on any
// machine), the G2 points on the host (trusted_setup.cpp), then per device the G1 points on the GPU (engine.hip: init_srs), the
// derived bases (engine_tables.hip: init_fk20) and, if asked for, the power structure (eip4844.hip: check_setup_powers).  Every
// failure is NULL + a message; a constructor that fails late tears down what it had built (Engine::teardown).
DASContext* eth_kzg_amd_das_context_new_with_setup(const uint8_t* g1_monomial, uint64_t n_g1, const uint8_t* g2_monomial, uint64_t n_g2,
                                                   uint32_t flags, bool use_precomp, const int32_t* device_ordinals, uint64_t n_devices,
                                                   double table_budget_gb, CResult* result) {
    std::string why;
    DASContext* c = nullptr;
    constexpr uint32_t KNOWN = ETH_KZG_AMD_SETUP_NO_SUBGROUP_CHECK | ETH_KZG_AMD_SETUP_CHECK_POWERS;
    if (n_g1 != kzg::TrustedSetup::N_G1 || n_g2 != kzg::TrustedSetup::N_G2)
        why = "InvalidInput: a trusted setup holds 4096 G1 and 65 G2 monomial points, got " + std::to_string(n_g1) + " and " + std::to_string(n_g2);
    else if (!g1_monomial || !g2_monomial) why = "InvalidInput: NULL point array (4096 G1 points of 48 bytes and 65 G2 points of 96 bytes are expected)";
    else if (flags & ~KNOWN) why = "InvalidInput: unknown setup flags";
    else if ((device_ordinals == nullptr) != (n_devices == 0) || n_devices > 64) why = "InvalidInput: the device list holds 1 to 64 ordinals (or NULL and 0)";
    else {
        try {
            const auto setup = kzg::TrustedSetup::from_points(g1_monomial, g2_monomial, !(flags & ETH_KZG_AMD_SETUP_NO_SUBGROUP_CHECK),
                                                              (flags & ETH_KZG_AMD_SETUP_CHECK_POWERS) != 0);
            const std::vector<int> devices = n_devices ? std::vector<int>(device_ordinals, device_ordinals + n_devices) : env_device_list();
            c = try_make_ctx(use_precomp, devices, table_budget_gb, &why, setup);
        } catch (const std::exception& e) {  // (the point copies and the device list are allocations too)
            why = std::string("InvalidSetup: ") + e.what();
        } catch (...) {
            why = "unknown failure";
        }
    }
    if (result) *result = c ? ok() : err("ContextCreation(" + why + ")");
    return c;
}
DASContext* eth_kzg_amd_das_context_new_with_setup_file(const uint8_t* file, uint64_t file_length, uint32_t flags, bool use_precomp,
                                                        const int32_t* device_ordinals, uint64_t n_devices, double table_budget_gb,
                                                        CResult* result) {
    // "KZGSRS01" | n_g1 (u32 LE) | n_g2 (u32 LE) | g1 monomial (48 B each) | g2 monomial (96 B each)
    uint32_t n1 = 0, n2 = 0;
    const char* bad = nullptr;
    if (!file) bad = "NULL file";
    else if (file_length < 16 || memcmp(file, "KZGSRS01", 8)) bad = "no KZGSRS01 header";
    else {
        memcpy(&n1, file + 8, 4);
        memcpy(&n2, file + 12, 4);
        if (file_length != 16 + (uint64_t)n1 * 48 + (uint64_t)n2 * 96) bad = "the length does not match the counts in the header";
    }
    if (bad) {
        if (result) *result = err(std::string("ContextCreation(InvalidInput: setup file: ") + bad + ")");
        return nullptr;
    }
    return eth_kzg_amd_das_context_new_with_setup(file + 16, n1, file + 16 + (size_t)n1 * 48, n2, flags, use_precomp, device_ordinals, n_devices,
                                                  table_budget_gb, result);
}
void eth_kzg_amd_setup_digest(const DASContext* ctx, uint8_t* out) { memcpy(out, eng(ctx)->setup().digest.data(), 32); }
uint64_t eth_kzg_amd_context_devices(const DASContext* ctx, int32_t* out_ordinals, uint64_t capacity) {
    live(ctx);
    for (size_t d = 0; d < ctx->engines.size() && d < capacity && out_ordinals; d++) out_ordinals[d] = ctx->engines[d]->device();
    return ctx->engines.size();
}
void eth_kzg_das_context_free(DASContext* ctx) {
    if (!ctx) return;
    eth_kzg_amd_comm_destroy(ctx);
    free_ctx(ctx);
}
void eth_kzg_free_error_message(char* c_message) {
    if (c_message) free(c_message);
}

CResult eth_kzg_blob_to_kzg_commitment(const DASContext* ctx, const uint8_t* blob, uint8_t* out) {
    Picked p = pick(ctx, CELLS);
    auto lane = p.e->lease_serial();
    kzg::Engine* e = lane.e;
    int st = 0;
    const uint8_t* blobs[1] = {blob};
    uint8_t* outs[1] = {out};
    if (e->blob_to_kzg_commitment_host(1, blobs, outs, &st)) return device_err(e);
    return st ? err(status_text(st)) : ok();
}

CResult eth_kzg_compute_cells_and_kzg_proofs(const DASContext* ctx, const uint8_t* blob, uint8_t** out_cells,
                                             uint8_t** out_proofs) {
    Picked p = pick(ctx, CELLS);
    kzg::Engine* e = p.e;
    int st = 0;
    const uint8_t* blobs[1] = {blob};
    uint8_t* const* cells[1] = {out_cells};
    uint8_t* const* proofs[1] = {out_proofs};
    if (e->compute_cells_and_kzg_proofs_host(1, blobs, cells, proofs, &st)) return device_err(e);
    return st ? err(status_text(st)) : ok();
}

CResult eth_kzg_compute_cells(const DASContext* ctx, const uint8_t* blob, uint8_t** out_cells) {
    Picked p = pick(ctx, CELLS / 16);
    kzg::Engine* e = p.e;
    int st = 0;
    const uint8_t* blobs[1] = {blob};
    uint8_t* const* cells[1] = {out_cells};
    if (e->compute_cells_and_kzg_proofs_host(1, blobs, cells, nullptr, &st)) return device_err(e);
    return st ? err(status_text(st)) : ok();
}

CResult eth_kzg_verify_cell_kzg_proof_batch(const DASContext* ctx, uint64_t commitments_length,
                                            const uint8_t* const* commitments, uint64_t cell_indices_length,
                                            const uint64_t* cell_indices, uint64_t cells_length,
                                            const uint8_t* const* cells, uint64_t proofs_length,
                                            const uint8_t* const* proofs, bool* verified) {
    // up to one caller per engine lane runs the latency path; callers beyond that are combined into many-verification passes
    Picked p = pick(ctx, cells_length / 8 + 1);
    kzg::Engine* e = p.e;
    int ver = 0;
    int st = e->verify_cell_kzg_proof_batch_combined(commitments_length, commitments, cell_indices_length, cell_indices,
                                                     cells_length, cells, proofs_length, proofs, &ver);
    return finish_verdict(e, st, ver, verified);
}

CResult eth_kzg_amd_verify_cell_kzg_proof_batch_many(const DASContext* ctx, uint64_t n_batches, const uint64_t* commitments_lengths,
                                                     const uint8_t* const* const* commitments, const uint64_t* cell_indices_lengths,
                                                     const uint64_t* const* cell_indices, const uint64_t* cells_lengths,
                                                     const uint8_t* const* const* cells, const uint64_t* proofs_lengths,
                                                     const uint8_t* const* const* proofs, bool* verified, int32_t* status) {
    return host_many(ctx, n_batches, MAX_BATCH, kzg::VerifyManyInput::lists(commitments_lengths, commitments, cell_indices_lengths, cell_indices, cells_lengths,
                     cells, proofs_lengths, proofs, /*leaf=*/false), verified, status);  // (the count is checked before the context is looked at: sliced_call)
}

CResult eth_kzg_amd_verify_cell_kzg_proof_batch_device(const DASContext* ctx, uint64_t n, const uint8_t* d_commitments,
                                                       const uint64_t* d_cell_indices, const uint8_t* d_cells,
                                                       const uint8_t* d_proofs, bool* verified, void* hip_stream) {
    kzg::Engine* owner = engine_of_pointer(ctx, d_cells);
    if (!owner) return err("InvalidInput: the buffers are on no device of this context");
    auto lane = owner->lease_serial();
    kzg::Engine* e = lane.e;
    int ver = 0;
    int st = e->verify_cell_kzg_proof_batch_device(n, d_commitments, d_cell_indices, d_cells, d_proofs, &ver, (hipStream_t)hip_stream);
    return finish_verdict(e, st, ver, verified);
}

// The two calls above with a flags word (c_eth_kzg.h: the leaf-hashed challenge).  The flagged host form is a single-problem call on a
// serial lane: it never joins the combiner, whose passes keep the reference's transcript.
CResult eth_kzg_amd_verify_cell_kzg_proof_batch_ex(const DASContext* ctx, uint64_t commitments_length, const uint8_t* const* commitments,
                                                   uint64_t cell_indices_length, const uint64_t* cell_indices, uint64_t cells_length,
                                                   const uint8_t* const* cells, uint64_t proofs_length, const uint8_t* const* proofs,
                                                   uint32_t flags, bool* verified) {
    if (flags & ~ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT) return err("InvalidInput: unknown verification flags");  // (before the context is looked at)
    if (cells_length > kzg::MAX_CELLS_PER_VERIFICATION) return err("InvalidInput");
    if (!flags)
        return eth_kzg_verify_cell_kzg_proof_batch(ctx, commitments_length, commitments, cell_indices_length, cell_indices, cells_length, cells,
                                                   proofs_length, proofs, verified);
    Picked p = pick(ctx, cells_length / 8 + 1);
    auto lane = p.e->lease_serial();
    kzg::Engine* e = lane.e;
    kzg::CellChallengeMode mode;
    mode.leaf = true;
    int ver = 0;
    int st = e->verify_cell_kzg_proof_batch_host(commitments_length, commitments, cell_indices_length, cell_indices, cells_length, cells,
                                                 proofs_length, proofs, &ver, &mode);
    return finish_verdict(e, st, ver, verified);
}
CResult eth_kzg_amd_verify_cell_kzg_proof_batch_device_ex(const DASContext* ctx, uint64_t n, const uint8_t* d_commitments,
                                                          const uint64_t* d_cell_indices, const uint8_t* d_cells, const uint8_t* d_proofs,
                                                          uint32_t flags, bool* verified, void* hip_stream) {
    if (flags & ~ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT) return err("InvalidInput: unknown verification flags");
    if (n > kzg::MAX_CELLS_PER_VERIFICATION) return err("InvalidInput");
    if (!flags) return eth_kzg_amd_verify_cell_kzg_proof_batch_device(ctx, n, d_commitments, d_cell_indices, d_cells, d_proofs, verified, hip_stream);
    kzg::Engine* owner = engine_of_pointer(ctx, d_cells);
    if (!owner) return err("InvalidInput: the buffers are on no device of this context");
    auto lane = owner->lease_serial();
    kzg::Engine* e = lane.e;
    kzg::CellChallengeMode mode;
    mode.leaf = true;
    int ver = 0;
    int st = e->verify_cell_kzg_proof_batch_device(n, d_commitments, d_cell_indices, d_cells, d_proofs, &ver, (hipStream_t)hip_stream, &mode);
    return finish_verdict(e, st, ver, verified);
}

// The many-verification with a flags word, on pointer lists and on flat arrays in HBM (c_eth_kzg.h).  Flags, counts and cell_starts are
// checked before the context is looked at.  The host form is cut by problem over the device list, as _many; the device form runs on the
// device that owns the buffers, and for it ALL FOUR pointers are resolved: a pointer that is not device memory of one listed device is
// InvalidInput, never a fault (none of them is dereferenced on the host).
CResult eth_kzg_amd_verify_cell_kzg_proof_batch_many_ex(const DASContext* ctx, uint64_t n_batches, const uint64_t* commitments_lengths,
                                                        const uint8_t* const* const* commitments, const uint64_t* cell_indices_lengths,
                                                        const uint64_t* const* cell_indices, const uint64_t* cells_lengths,
                                                        const uint8_t* const* const* cells, const uint64_t* proofs_lengths,
                                                        const uint8_t* const* const* proofs, uint32_t flags, bool* verified, int32_t* status) {
    if (flags & ~ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT) return err("InvalidInput: unknown verification flags");
    return host_many(ctx, n_batches, MAX_BATCH, kzg::VerifyManyInput::lists(commitments_lengths, commitments, cell_indices_lengths, cell_indices, cells_lengths,
                     cells, proofs_lengths, proofs, /*leaf=*/flags != 0), verified, status);
}
CResult eth_kzg_amd_verify_cell_kzg_proof_batch_many_device_ex(const DASContext* ctx, uint64_t n_batches, const uint64_t* cell_starts,
                                                               const uint8_t* d_commitments, const uint64_t* d_cell_indices, const uint8_t* d_cells,
                                                               const uint8_t* d_proofs, uint32_t flags, bool* verified, int32_t* status,
                                                               void* hip_stream) {
    if (flags & ~ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT) return err("InvalidInput: unknown verification flags");
    if (n_batches > MAX_BATCH) return err("InvalidInput");
    if (kzg::validate_cell_starts(n_batches, cell_starts) != kzg::INPUT_VALID)
        return err("InvalidInput: cell_starts holds n_batches + 1 non-decreasing entries, the first of them 0");
    live(ctx);
    if (n_batches == 0) return ok();
    kzg::Engine* e = ctx->engine;
    if (cell_starts[n_batches]) {  // (a call of empty problems only reads none of the arrays)
        const void* const ptrs[4] = {d_commitments, d_cell_indices, d_cells, d_proofs};
        e = engine_of_device_pointers(ctx, ptrs, 4);
        if (!e) return err("InvalidInput: the four buffers are not device memory of one device of this context");
    }
    return device_many(e, n_batches, kzg::VerifyManyInput::flat_device(cell_starts, d_commitments, d_cell_indices, d_cells, d_proofs, (hipStream_t)hip_stream,
                                                                       flags != 0), verified, status);
}

// The columns of one block over ONE commitment list (c_eth_kzg.h): the many-verification's column source (verify_many.hip).  Flags,
// counts and null arrays are refused before the context is looked at (verify_host.hpp: validate_data_columns_call).  The host form is
// cut by COLUMN over the device list, the commitments de-duplicated once, here, for all of its slices; the device form runs on the
// device that owns the three buffers.
CResult eth_kzg_amd_verify_data_columns(const DASContext* ctx, uint64_t n_blobs, const uint8_t* const* commitments, uint64_t n_columns,
                                        const uint64_t* column_indices, const uint8_t* const* const* cells, const uint8_t* const* const* proofs,
                                        uint32_t flags, bool* verified, int32_t* status) {
    if (kzg::validate_data_columns_call(flags, ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT, n_blobs, n_columns, !commitments, !column_indices, !cells, !proofs,
                                        !verified) != kzg::INPUT_VALID)
        return err("InvalidInput: unknown verification flags, more than 2^24 columns, or a null array");
    kzg::ColumnCommitments cc;
    auto in = kzg::VerifyManyInput::host_columns(n_blobs, commitments, column_indices, cells, proofs, flags != 0);
    if (n_columns && n_blobs && n_blobs <= kzg::MAX_CELLS_PER_VERIFICATION) {
        cc.from_list(n_blobs, commitments);
        in.col = &cc;
    }
    return host_many(ctx, n_columns, kzg::DATA_COLUMNS_MAX, in, verified, status);
}
CResult eth_kzg_amd_verify_data_columns_device(const DASContext* ctx, uint64_t n_blobs, const uint8_t* d_commitments, uint64_t n_columns,
                                               const uint64_t* column_indices, const uint8_t* d_cells, const uint8_t* d_proofs, uint32_t flags,
                                               bool* verified, int32_t* status, void* hip_stream) {
    if (kzg::validate_data_columns_call(flags, ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT, n_blobs, n_columns, !d_commitments, !column_indices, !d_cells, !d_proofs,
                                        !verified) != kzg::INPUT_VALID)
        return err("InvalidInput: unknown verification flags, more than 2^24 columns, or a null array");
    live(ctx);
    if (n_columns == 0) return ok();
    kzg::Engine* e = ctx->engine;
    if (n_blobs && n_blobs <= kzg::MAX_CELLS_PER_VERIFICATION) {  // (otherwise none of the arrays is read)
        const void* const ptrs[3] = {d_commitments, d_cells, d_proofs};
        e = engine_of_device_pointers(ctx, ptrs, 3);
        if (!e) return err("InvalidInput: the three buffers are not device memory of one device of this context");
    }
    return device_many(e, n_columns, kzg::VerifyManyInput::device_columns(n_blobs, d_commitments, column_indices, d_cells, d_proofs, (hipStream_t)hip_stream,
                                                                          flags != 0), verified, status);
}

// Partial data columns (c_eth_kzg.h): the column source's fifth spelling.  The call-level refusals come before the context is looked at
// (verify_host.hpp: validate_partial_columns_call); the bitmaps are validated and counted ONCE, here (PartialColumns), and the host
// form's commitments de-duplicated once for all slices of a device list.
CResult eth_kzg_amd_verify_partial_data_columns(const DASContext* ctx, uint64_t n_blobs, const uint8_t* const* commitments, uint64_t n_columns,
                                                const uint64_t* column_indices, const uint64_t* const* present, const uint8_t* const* const* cells,
                                                const uint8_t* const* const* proofs, uint32_t flags, bool* verified, int32_t* status) {
    if (kzg::validate_partial_columns_call(flags, ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT, n_blobs, n_columns, !commitments, !column_indices, !present, !cells,
                                           !proofs, !verified) != kzg::INPUT_VALID)
        return err("InvalidInput: unknown verification flags, more than 2^24 columns, or a null array");
    try {  // (the column plan and the de-duplication allocate: nothing may be thrown across the C ABI)
        kzg::PartialColumns pc;
        kzg::ColumnCommitments cc;
        pc.from_list(n_blobs, n_columns, column_indices, present);
        auto in = kzg::VerifyManyInput::host_partial_columns(pc, commitments, column_indices, cells, proofs, flags != 0);
        if (pc.total_cells()) {
            cc.from_list(n_blobs, commitments);
            in.col = &cc;
        }
        return host_many(ctx, n_columns, kzg::DATA_COLUMNS_MAX, in, verified, status);
    } catch (const std::exception& ex) {
        return err(std::string("DeviceError(") + ex.what() + ")");
    }
}
CResult eth_kzg_amd_verify_partial_data_columns_device(const DASContext* ctx, uint64_t n_blobs, const uint8_t* d_commitments, uint64_t n_columns,
                                                       const uint64_t* column_indices, const uint64_t* present, const uint8_t* d_cells,
                                                       const uint8_t* d_proofs, uint32_t flags, bool* verified, int32_t* status, void* hip_stream) {
    if (kzg::validate_partial_columns_call(flags, ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT, n_blobs, n_columns, !d_commitments, !column_indices, !present, !d_cells,
                                           !d_proofs, !verified) != kzg::INPUT_VALID)
        return err("InvalidInput: unknown verification flags, more than 2^24 columns, or a null array");
    live(ctx);
    if (n_columns == 0) return ok();
    try {  // (the column plan allocates: nothing may be thrown across the C ABI)
        kzg::PartialColumns pc;
        pc.from_flat(n_blobs, n_columns, column_indices, present);
        kzg::Engine* e = ctx->engine;
        if (n_blobs && n_blobs <= kzg::MAX_CELLS_PER_VERIFICATION) {  // (otherwise none of the arrays is read)
            const void* const ptrs[3] = {d_commitments, d_cells, d_proofs};
            e = engine_of_device_pointers(ctx, ptrs, 3);
            if (!e) return err("InvalidInput: the three buffers are not device memory of one device of this context");
        }
        return device_many(e, n_columns, kzg::VerifyManyInput::device_partial_columns(pc, d_commitments, column_indices, d_cells, d_proofs,
                                                                                      (hipStream_t)hip_stream, flags != 0), verified, status);
    } catch (const std::exception& ex) {
        return err(std::string("DeviceError(") + ex.what() + ")");
    }
}

CResult eth_kzg_amd_recover_cells_and_proofs_device(const DASContext* ctx, uint64_t n, const uint8_t* d_cells,
                                                    const uint64_t* present_masks, uint8_t* d_out_cells, uint8_t* d_out_proofs,
                                                    int32_t* status, void* hip_stream) {
    if (n > MAX_BATCH) return err("InvalidInput");
    kzg::Engine* owner = engine_of_pointer(ctx, d_cells);
    if (!owner) return err("InvalidInput: the buffers are on no device of this context");
    auto lane = owner->lease_serial();
    kzg::Engine* e = lane.e;
    static_assert(sizeof(int32_t) == sizeof(int), "status array");
    int st = e->recover_cells_and_kzg_proofs_device((int)n, d_cells, present_masks, d_out_cells, d_out_proofs, (int*)status,
                                                    (hipStream_t)hip_stream);
    if (st == kzg::ERR_DEVICE) return device_err(e);
    return st ? err(status_text(st)) : ok();
}

// Sharded verification: per-rank partial, then one combine over the gathered records.
CResult eth_kzg_amd_verify_cell_kzg_proof_batch_partial(const DASContext* ctx, uint64_t commitments_length,
                                                        const uint8_t* const* commitments, uint64_t cell_indices_length,
                                                        const uint64_t* cell_indices, uint64_t cells_length,
                                                        const uint8_t* const* cells, uint64_t proofs_length,
                                                        const uint8_t* const* proofs, uint64_t shard_begin,
                                                        uint64_t shard_end, uint8_t* out_partial) {
    Picked p = pick(ctx, (shard_end > shard_begin ? shard_end - shard_begin : 0) / 8 + 1);
    auto lane = p.e->lease_serial();
    kzg::Engine* e = lane.e;
    int st = e->verify_cell_kzg_proof_batch_partial_host(commitments_length, commitments, cell_indices_length, cell_indices,
                                                         cells_length, cells, proofs_length, proofs, shard_begin, shard_end,
                                                         out_partial);
    if (st == kzg::ERR_DEVICE) return device_err(e);
    return st ? err(status_text(st)) : ok();
}

CResult eth_kzg_amd_verify_cell_kzg_proof_batch_combine(const DASContext* ctx, uint64_t n_partials, const uint8_t* partials,
                                                        bool* verified) {
    if (n_partials > MAX_BATCH) return err("InvalidInput");
    Picked p = pick(ctx, 1);
    auto lane = p.e->lease_serial();
    kzg::Engine* e = lane.e;
    int ver = 0;
    int st = e->verify_cell_kzg_proof_batch_combine_host(n_partials, partials, &ver);
    if (st) return err(status_text(st));
    *verified = ver != 0;
    return ok();
}

CResult eth_kzg_recover_cells_and_proofs(const DASContext* ctx, uint64_t cells_length, const uint8_t* const* cells,
                                         uint64_t cell_indices_length, const uint64_t* cell_indices,
                                         uint8_t** out_cells, uint8_t** out_proofs) {
    Picked p = pick(ctx, 2 * CELLS);
    auto lane = p.e->lease_serial();
    kzg::Engine* e = lane.e;
    int st = e->recover_cells_and_kzg_proofs_host(cells_length, cells, cell_indices_length, cell_indices, out_cells, out_proofs);
    if (st == kzg::ERR_DEVICE) return device_err(e);
    return st ? err(status_text(st)) : ok();
}

uint64_t eth_kzg_constant_bytes_per_cell(void) { return 2048; }
uint64_t eth_kzg_constant_bytes_per_proof(void) { return 48; }
uint64_t eth_kzg_constant_cells_per_ext_blob(void) { return CELLS; }

// EIP-4844 single-point operations (bindings/c/src/lib.rs:423-566)
CResult eth_kzg_compute_kzg_proof(const DASContext* ctx, const uint8_t* blob, const uint8_t* z, uint8_t* out_proof, uint8_t* out_y) {
    Picked p = pick(ctx, CELLS);
    auto lane = p.e->lease_serial();
    kzg::Engine* e = lane.e;
    return finish(e, e->compute_kzg_proof_host(blob, z, out_proof, out_y));
}
CResult eth_kzg_compute_blob_kzg_proof(const DASContext* ctx, const uint8_t* blob, const uint8_t* commitment, uint8_t* out) {
    Picked p = pick(ctx, CELLS);
    auto lane = p.e->lease_serial();
    kzg::Engine* e = lane.e;
    return finish(e, e->compute_blob_kzg_proof_host(blob, commitment, out));
}
CResult eth_kzg_verify_kzg_proof(const DASContext* ctx, const uint8_t* commitment, const uint8_t* z, const uint8_t* y,
                                 const uint8_t* proof, bool* verified) {
    Picked p = pick(ctx, 1);
    auto lane = p.e->lease_serial();
    kzg::Engine* e = lane.e;
    int ver = 0;
    int st = e->verify_kzg_proof_host(commitment, z, y, proof, &ver);
    return finish_verdict(e, st, ver, verified);
}
CResult eth_kzg_verify_blob_kzg_proof(const DASContext* ctx, const uint8_t* blob, const uint8_t* commitment, const uint8_t* proof,
                                      bool* verified) {
    Picked p = pick(ctx, CELLS);
    auto lane = p.e->lease_serial();
    kzg::Engine* e = lane.e;
    int ver = 0;
    int st = e->verify_blob_kzg_proof_host(blob, commitment, proof, &ver);
    return finish_verdict(e, st, ver, verified);
}
CResult eth_kzg_verify_blob_kzg_proof_batch(const DASContext* ctx, uint64_t blobs_length, const uint8_t* const* blobs,
                                            uint64_t commitments_length, const uint8_t* const* commitments, uint64_t proofs_length,
                                            const uint8_t* const* proofs, bool* verified) {
    // ONE random linear combination over the whole batch (crates/eip4844/src/verifier.rs): not cut over devices
    Picked p = pick(ctx, blobs_length < MAX_BATCH ? blobs_length * CELLS + 1 : 1);
    auto lane = p.e->lease_serial();
    kzg::Engine* e = lane.e;
    int ver = 0;
    int st = e->verify_blob_kzg_proof_batch_host(blobs_length, blobs, commitments_length, commitments, proofs_length, proofs, &ver);
    return finish_verdict(e, st, ver, verified);
}

// ---------------------------------------------------------------------------------------------
// Host-pointer batches: contiguous slices over the context's device list (the caller's buffers are the gather target; no
// collective), the whole batch on the one engine of a one-device context.
CResult eth_kzg_amd_compute_cells_and_kzg_proofs_batch(const DASContext* ctx, uint64_t n, const uint8_t* const* blobs,
                                                       uint8_t* const* const* out_cells, uint8_t* const* const* out_proofs,
                                                       int32_t* status) {
    return sliced_call(ctx, n, MAX_BATCH, nullptr, status, [&] { return blobs != nullptr; }, [&](kzg::Engine* e, uint64_t lo, uint64_t hi, int* st, int*) {
        return batch_failure(e, e->compute_cells_and_kzg_proofs_host((int)(hi - lo), blobs + lo, out_cells ? out_cells + lo : nullptr,
                                                                     out_proofs ? out_proofs + lo : nullptr, st + lo));
    });
}
CResult eth_kzg_amd_blob_to_kzg_commitment_batch(const DASContext* ctx, uint64_t n, const uint8_t* const* blobs,
                                                 uint8_t* const* out, int32_t* status) {
    return sliced_call(ctx, n, MAX_BATCH, nullptr, status, [&] { return blobs && out; }, [&](kzg::Engine* dev, uint64_t lo, uint64_t hi, int* st, int*) {
        auto lane = dev->lease_serial();
        kzg::Engine* e = lane.e;
        return batch_failure(e, e->blob_to_kzg_commitment_host((int)(hi - lo), blobs + lo, out + lo, st + lo));
    });
}
CResult eth_kzg_amd_recover_cells_and_proofs_batch(const DASContext* ctx, uint64_t n, const uint64_t* cells_lengths,
                                                   const uint8_t* const* const* cells, const uint64_t* cell_indices_lengths,
                                                   const uint64_t* const* cell_indices, uint8_t* const* const* out_cells,
                                                   uint8_t* const* const* out_proofs, int32_t* status) {
    return sliced_call(ctx, n, MAX_BATCH, nullptr, status, [&] { return cells_lengths && cells && cell_indices_lengths && cell_indices; },
                       [&](kzg::Engine* dev, uint64_t lo, uint64_t hi, int* st, int*) {
        auto lane = dev->lease_serial();
        kzg::Engine* e = lane.e;
        return batch_failure(e, e->recover_cells_and_kzg_proofs_batch_host((int)(hi - lo), cells_lengths + lo, cells + lo, cell_indices_lengths + lo,
                                                                           cell_indices + lo, out_cells ? out_cells + lo : nullptr,
                                                                           out_proofs ? out_proofs + lo : nullptr, st + lo));
    });
}
CResult eth_kzg_amd_compute_cells_and_kzg_proofs_device(const DASContext* ctx, uint64_t n, const uint8_t* d_blobs,
                                                        uint8_t* d_out_cells, uint8_t* d_out_proofs, int32_t* status,
                                                        void* hip_stream) {
    if (n > MAX_BATCH) return err("InvalidInput");
    kzg::Engine* e = engine_of_pointer(ctx, d_blobs);
    if (!e) return err("InvalidInput: the buffers are on no device of this context");
    bool sync = hip_stream == nullptr;
    if (e->compute_cells_and_kzg_proofs_device((int)n, d_blobs, d_out_cells, d_out_proofs, status, (hipStream_t)hip_stream, sync))
        return device_err(e);
    if (status) for (uint64_t i = 0; i < n; i++) status[i] = status[i] ? kzg::ERR_SCALAR : 0;
    return ok();
}
CResult eth_kzg_amd_blob_to_kzg_commitment_device(const DASContext* ctx, uint64_t n, const uint8_t* d_blobs, uint8_t* d_out,
                                                  int32_t* status, void* hip_stream) {
    if (n > MAX_BATCH) return err("InvalidInput");
    kzg::Engine* owner = engine_of_pointer(ctx, d_blobs);
    if (!owner) return err("InvalidInput: the buffers are on no device of this context");
    auto lane = owner->lease_serial();
    kzg::Engine* e = lane.e;
    bool sync = hip_stream == nullptr;
    if (e->blob_to_kzg_commitment_device((int)n, d_blobs, d_out, status, (hipStream_t)hip_stream, sync)) return device_err(e);
    if (status) for (uint64_t i = 0; i < n; i++) status[i] = status[i] ? kzg::ERR_SCALAR : 0;
    return ok();
}
// ---------------------------------------------------------------------------------------------
// A block's data columns in column layout (data_columns.hip; c_eth_kzg.h).  The count and the NULL arrays are refused before the context
// is looked at.  Host forms: contiguous slices by BLOB over the device list, every slice writing its blobs' entries of the shared
// column arrays; device forms: the device that owns every buffer given.
CResult eth_kzg_amd_compute_data_columns(const DASContext* ctx, uint64_t n_blobs, const uint8_t* const* blobs, uint8_t* const* out_commitments,
                                         uint8_t* const* const* out_cells, uint8_t* const* const* out_proofs, int32_t* status) {
    if (n_blobs > MAX_BATCH || (n_blobs && !blobs)) return err("InvalidInput");
    if (n_blobs == 0) return ok();  // (an empty call looks at nothing, the context included)
    return sliced_call(ctx, n_blobs, MAX_BATCH, nullptr, status, [] { return true; }, [&](kzg::Engine* e, uint64_t lo, uint64_t hi, int* st, int*) {
        return batch_failure(e, e->compute_data_columns_host((int)lo, (int)(hi - lo), blobs, out_commitments, out_cells, out_proofs, st));
    });
}
CResult eth_kzg_amd_compute_data_columns_device(const DASContext* ctx, uint64_t n_blobs, const uint8_t* d_blobs, uint8_t* d_out_commitments,
                                                uint8_t* d_out_cells, uint8_t* d_out_proofs, int32_t* status, void* hip_stream) {
    if (n_blobs > MAX_BATCH) return err("InvalidInput");
    if (n_blobs && !d_blobs) return err("InvalidInput");
    if (n_blobs == 0) return ok();
    live(ctx);
    const void* ptrs[4] = {d_blobs};
    int n_ptrs = 1;
    for (const void* p : {(const void*)d_out_commitments, (const void*)d_out_cells, (const void*)d_out_proofs})
        if (p) ptrs[n_ptrs++] = p;
    kzg::Engine* e = engine_of_device_pointers(ctx, ptrs, n_ptrs);
    if (!e) return err("InvalidInput: the buffers are not device memory of one device of this context");
    static_assert(sizeof(int32_t) == sizeof(int), "status array");
    const bool sync = hip_stream == nullptr;
    if (e->compute_data_columns_device((int)n_blobs, d_blobs, d_out_commitments, d_out_cells, d_out_proofs, (int*)status, (hipStream_t)hip_stream, sync))
        return device_err(e);
    if (status) for (uint64_t i = 0; i < n_blobs; i++) status[i] = status[i] ? kzg::ERR_SCALAR : 0;
    return ok();
}
CResult eth_kzg_amd_recover_data_columns(const DASContext* ctx, uint64_t n_blobs, uint64_t n_columns, const uint64_t* column_indices,
                                         const uint8_t* const* const* cells, uint8_t* const* const* out_cells, uint8_t* const* const* out_proofs,
                                         int32_t* status) {
    if (n_blobs > MAX_BATCH || (n_blobs && (!cells || !status || (n_columns && !column_indices)))) return err("InvalidInput");
    if (n_blobs == 0) return ok();
    return sliced_call(ctx, n_blobs, MAX_BATCH, nullptr, status, [] { return true; }, [&](kzg::Engine* dev, uint64_t lo, uint64_t hi, int* st, int*) {
        auto lane = dev->lease_serial();
        kzg::Engine* e = lane.e;
        return batch_failure(e, e->recover_data_columns_host((int)lo, (int)(hi - lo), n_columns, column_indices, cells, out_cells, out_proofs, st));
    });
}
CResult eth_kzg_amd_recover_data_columns_device(const DASContext* ctx, uint64_t n_blobs, uint64_t n_columns, const uint64_t* column_indices,
                                                const uint8_t* d_cells, uint8_t* d_out_cells, uint8_t* d_out_proofs, int32_t* status,
                                                void* hip_stream) {
    if (n_blobs > MAX_BATCH) return err("InvalidInput");
    if (n_blobs && (!d_cells || !status || (n_columns && !column_indices))) return err("InvalidInput");
    if (n_blobs == 0) return ok();
    live(ctx);
    const void* ptrs[3] = {d_cells};
    int n_ptrs = 1;
    for (const void* p : {(const void*)d_out_cells, (const void*)d_out_proofs})
        if (p) ptrs[n_ptrs++] = p;
    kzg::Engine* owner = engine_of_device_pointers(ctx, ptrs, n_ptrs);
    if (!owner) return err("InvalidInput: the buffers are not device memory of one device of this context");
    auto lane = owner->lease_serial();
    kzg::Engine* e = lane.e;
    static_assert(sizeof(int32_t) == sizeof(int), "status array");
    if (e->recover_data_columns_device((int)n_blobs, n_columns, column_indices, d_cells, d_out_cells, d_out_proofs, (int*)status, (hipStream_t)hip_stream))
        return device_err(e);
    return ok();
}
// The same recovery checked against the block's commitments.  The refusals of the call are those of the two above; the host form's
// slices index commitments, out_blobs and out_commitments with their offset like every other array of the call.  The device form
// settles a bad index list BEFORE it resolves a pointer: every blob is 3 and nothing -- d_commitments included -- is looked at.
CResult eth_kzg_amd_recover_data_columns_checked(const DASContext* ctx, uint64_t n_blobs, const uint8_t* const* commitments, uint64_t n_columns,
                                                 const uint64_t* column_indices, const uint8_t* const* const* cells, uint8_t* const* out_blobs,
                                                 uint8_t* const* out_commitments, uint8_t* const* const* out_cells, uint8_t* const* const* out_proofs,
                                                 int32_t* status) {
    if (n_blobs > MAX_BATCH || (n_blobs && (!cells || !status || (n_columns && !column_indices)))) return err("InvalidInput");
    if (n_blobs == 0) return ok();
    kzg::Engine::RecoverCheck chk;
    chk.commitments = commitments;
    chk.out_blobs = out_blobs;
    chk.out_commitments = out_commitments;
    return sliced_call(ctx, n_blobs, MAX_BATCH, nullptr, status, [] { return true; }, [&](kzg::Engine* dev, uint64_t lo, uint64_t hi, int* st, int*) {
        auto lane = dev->lease_serial();
        kzg::Engine* e = lane.e;
        return batch_failure(e, e->recover_data_columns_checked_host((int)lo, (int)(hi - lo), n_columns, column_indices, cells, chk, out_cells, out_proofs, st));
    });
}
CResult eth_kzg_amd_recover_data_columns_checked_device(const DASContext* ctx, uint64_t n_blobs, const uint8_t* d_commitments, uint64_t n_columns,
                                                        const uint64_t* column_indices, const uint8_t* d_cells, uint8_t* d_out_blobs,
                                                        uint8_t* d_out_commitments, uint8_t* d_out_cells, uint8_t* d_out_proofs, int32_t* status,
                                                        void* hip_stream) {
    if (n_blobs > MAX_BATCH) return err("InvalidInput");
    if (n_blobs && (!d_cells || !status || (n_columns && !column_indices))) return err("InvalidInput");
    if (n_blobs == 0) return ok();
    live(ctx);
    if (kzg::column_list_status(n_columns, column_indices) != kzg::INPUT_VALID) {
        for (uint64_t i = 0; i < n_blobs; i++) status[i] = kzg::ERR_INPUT;
        return ok();
    }
    const void* ptrs[6] = {d_cells};
    int n_ptrs = 1;
    for (const void* p : {(const void*)d_commitments, (const void*)d_out_blobs, (const void*)d_out_commitments, (const void*)d_out_cells, (const void*)d_out_proofs})
        if (p) ptrs[n_ptrs++] = p;
    kzg::Engine* owner = engine_of_device_pointers(ctx, ptrs, n_ptrs);
    if (!owner) return err("InvalidInput: the buffers are not device memory of one device of this context");
    auto lane = owner->lease_serial();
    kzg::Engine* e = lane.e;
    kzg::Engine::RecoverCheck chk;
    chk.d_commitments = d_commitments;
    chk.d_out_blobs = d_out_blobs;
    chk.d_out_commitments = d_out_commitments;
    if (e->recover_data_columns_checked_device((int)n_blobs, n_columns, column_indices, d_cells, chk, d_out_cells, d_out_proofs, (int*)status,
                                               (hipStream_t)hip_stream))
        return device_err(e);
    return ok();
}
// ---------------------------------------------------------------------------------------------
// EIP-4844 proofs for many blobs (eip4844.hip).  Host-pointer forms: contiguous slices over the device list; device-resident forms:
// the engine that owns d_blobs; the device verifier is ONE random combination over the whole batch and is never cut.
CResult eth_kzg_amd_compute_blob_kzg_proof_batch(const DASContext* ctx, uint64_t n, const uint8_t* const* blobs, const uint8_t* const* commitments,
                                                 uint8_t* const* out_proofs, int32_t* status) {
    return sliced_call(ctx, n, MAX_BATCH, nullptr, status, [&] { return blobs && commitments && out_proofs; }, [&](kzg::Engine* dev, uint64_t lo, uint64_t hi, int* st, int*) {
        auto lane = dev->lease_serial();
        kzg::Engine* e = lane.e;
        return batch_failure(e, e->compute_blob_kzg_proof_batch_host((int)(hi - lo), blobs + lo, commitments + lo, out_proofs + lo, st + lo));
    });
}
CResult eth_kzg_amd_compute_kzg_proof_batch(const DASContext* ctx, uint64_t n, const uint8_t* const* blobs, const uint8_t* const* zs,
                                            uint8_t* const* out_proofs, uint8_t* const* out_ys, int32_t* status) {
    return sliced_call(ctx, n, MAX_BATCH, nullptr, status, [&] { return blobs && zs && out_proofs && out_ys; }, [&](kzg::Engine* dev, uint64_t lo, uint64_t hi, int* st, int*) {
        auto lane = dev->lease_serial();
        kzg::Engine* e = lane.e;
        return batch_failure(e, e->compute_kzg_proof_batch_host((int)(hi - lo), blobs + lo, zs + lo, out_proofs + lo, out_ys + lo, st + lo));
    });
}
CResult eth_kzg_amd_compute_blob_kzg_proof_device(const DASContext* ctx, uint64_t n, const uint8_t* d_blobs, const uint8_t* d_commitments,
                                                  uint8_t* d_out_proofs, int32_t* status, void* hip_stream) {
    if (n > MAX_BATCH) return err("InvalidInput");
    kzg::Engine* owner = engine_of_pointer(ctx, d_blobs);
    if (!owner) return err("InvalidInput: the buffers are on no device of this context");
    if (n == 0) return ok();
    if (!d_blobs || !d_commitments || !d_out_proofs) return err("InvalidInput");
    auto lane = owner->lease_serial();
    kzg::Engine* e = lane.e;
    static_assert(sizeof(int32_t) == sizeof(int), "status array");
    const bool sync = hip_stream == nullptr;
    if (e->compute_blob_kzg_proof_device((int)n, d_blobs, d_commitments, d_out_proofs, (int*)status, (hipStream_t)hip_stream, sync)) return device_err(e);
    return ok();
}
CResult eth_kzg_amd_compute_kzg_proof_device(const DASContext* ctx, uint64_t n, const uint8_t* d_blobs, const uint8_t* d_zs, uint8_t* d_out_proofs,
                                             uint8_t* d_out_ys, int32_t* status, void* hip_stream) {
    if (n > MAX_BATCH) return err("InvalidInput");
    kzg::Engine* owner = engine_of_pointer(ctx, d_blobs);
    if (!owner) return err("InvalidInput: the buffers are on no device of this context");
    if (n == 0) return ok();
    if (!d_blobs || !d_zs || !d_out_proofs || !d_out_ys) return err("InvalidInput");
    auto lane = owner->lease_serial();
    kzg::Engine* e = lane.e;
    const bool sync = hip_stream == nullptr;
    if (e->compute_kzg_proof_device((int)n, d_blobs, d_zs, d_out_proofs, d_out_ys, (int*)status, (hipStream_t)hip_stream, sync)) return device_err(e);
    return ok();
}
CResult eth_kzg_amd_verify_blob_kzg_proof_batch_device(const DASContext* ctx, uint64_t n, const uint8_t* d_blobs, const uint8_t* d_commitments,
                                                       const uint8_t* d_proofs, bool* verified, void* hip_stream) {
    if (n > MAX_BATCH) return err("InvalidInput");
    kzg::Engine* owner = engine_of_pointer(ctx, d_blobs);
    if (!owner) return err("InvalidInput: the buffers are on no device of this context");
    if (n == 0) { *verified = true; return ok(); }
    if (!d_blobs || !d_commitments || !d_proofs) return err("InvalidInput");
    auto lane = owner->lease_serial();
    kzg::Engine* e = lane.e;
    int ver = 0;
    const int st = e->verify_blob_kzg_proof_batch_device(n, d_blobs, d_commitments, d_proofs, &ver, (hipStream_t)hip_stream);
    return finish_verdict(e, st, ver, verified);
}
// Many verify_kzg_proof items, a verdict each (point_many.hip).  The count and the arrays are checked before the context is looked at.
// Host form: contiguous slices by item over the device list; device form: the device that owns ALL FOUR buffers.
CResult eth_kzg_amd_verify_kzg_proof_many(const DASContext* ctx, uint64_t n, const uint8_t* const* commitments, const uint8_t* const* zs,
                                          const uint8_t* const* ys, const uint8_t* const* proofs, bool* verified, int32_t* status) {
    if (n && (!commitments || !zs || !ys || !proofs || !verified)) return err("InvalidInput");  // (with the count, before the context is looked at)
    kzg::PointManyInput in;
    in.commitments = commitments; in.zs = zs; in.ys = ys; in.proofs = proofs;
    auto items_ok = [&] {
        for (uint64_t i = 0; i < n; i++)
            if (!commitments[i] || !zs[i] || !ys[i] || !proofs[i]) return false;
        return true;
    };
    return sliced_call(ctx, n, kzg::POINT_MANY_MAX_ITEMS, verified, status, items_ok, [&](kzg::Engine* e, uint64_t lo, uint64_t hi, int* st, int* ver) {
        return many_failure(e, e->verify_kzg_proof_many(hi - lo, in.from(lo), ver + lo, st + lo));
    });
}
CResult eth_kzg_amd_verify_kzg_proof_many_device(const DASContext* ctx, uint64_t n, const uint8_t* d_commitments, const uint8_t* d_zs,
                                                 const uint8_t* d_ys, const uint8_t* d_proofs, bool* verified, int32_t* status, void* hip_stream) {
    if (n > kzg::POINT_MANY_MAX_ITEMS) return err("InvalidInput");
    if (n && (!d_commitments || !d_zs || !d_ys || !d_proofs || !verified)) return err("InvalidInput");
    live(ctx);
    if (n == 0) return ok();
    const void* const ptrs[4] = {d_commitments, d_zs, d_ys, d_proofs};
    kzg::Engine* e = engine_of_device_pointers(ctx, ptrs, 4);
    if (!e) return err("InvalidInput: the four buffers are not device memory of one device of this context");
    try {
        std::vector<int> ver(n), st(n);
        kzg::PointManyInput in;
        in.on_device = true;
        in.d_commitments = d_commitments; in.d_zs = d_zs; in.d_ys = d_ys; in.d_proofs = d_proofs;
        in.user_stream = (hipStream_t)hip_stream;
        if (e->verify_kzg_proof_many(n, in, ver.data(), st.data()) == kzg::ERR_DEVICE) return device_err(e);
        return verdicts_out(n, ver.data(), st.data(), verified, status);
    } catch (const std::exception& ex) {
        return err(std::string("DeviceError(") + ex.what() + ")");
    }
}
// Many verify_blob_kzg_proof items, a verdict each: the blob source of the same pass.  Count and arrays first, then the device list
// (host form: contiguous slices by item) or the owner of ALL THREE buffers (device form).
CResult eth_kzg_amd_verify_blob_kzg_proof_many(const DASContext* ctx, uint64_t n, const uint8_t* const* blobs, const uint8_t* const* commitments,
                                               const uint8_t* const* proofs, bool* verified, int32_t* status) {
    if (n && (!blobs || !commitments || !proofs || !verified)) return err("InvalidInput");  // (with the count, before the context is looked at)
    kzg::PointManyInput in;
    in.from_blobs = true;
    in.blobs = blobs; in.commitments = commitments; in.proofs = proofs;
    auto items_ok = [&] {
        for (uint64_t i = 0; i < n; i++) {
            verified[i] = false;
            if (!blobs[i] || !commitments[i] || !proofs[i]) return false;
        }
        return true;
    };
    return sliced_call(ctx, n, kzg::BLOB_MANY_MAX_ITEMS, verified, status, items_ok, [&](kzg::Engine* e, uint64_t lo, uint64_t hi, int* st, int* ver) {
        return many_failure(e, e->verify_kzg_proof_many(hi - lo, in.from(lo), ver + lo, st + lo));
    });
}
CResult eth_kzg_amd_verify_blob_kzg_proof_many_device(const DASContext* ctx, uint64_t n, const uint8_t* d_blobs, const uint8_t* d_commitments,
                                                      const uint8_t* d_proofs, bool* verified, int32_t* status, void* hip_stream) {
    if (n > kzg::BLOB_MANY_MAX_ITEMS) return err("InvalidInput");
    if (n && (!d_blobs || !d_commitments || !d_proofs || !verified)) return err("InvalidInput");
    live(ctx);
    if (n == 0) return ok();
    for (uint64_t i = 0; i < n; i++) verified[i] = false;
    const void* const ptrs[3] = {d_blobs, d_commitments, d_proofs};
    kzg::Engine* e = engine_of_device_pointers(ctx, ptrs, 3);
    if (!e) return err("InvalidInput: the three buffers are not device memory of one device of this context");
    try {
        std::vector<int> ver(n), st(n);
        kzg::PointManyInput in;
        in.on_device = true;
        in.from_blobs = true;
        in.d_blobs = d_blobs; in.d_commitments = d_commitments; in.d_proofs = d_proofs;
        in.user_stream = (hipStream_t)hip_stream;
        if (e->verify_kzg_proof_many(n, in, ver.data(), st.data()) == kzg::ERR_DEVICE) return device_err(e);
        return verdicts_out(n, ver.data(), st.data(), verified, status);
    } catch (const std::exception& ex) {
        return err(std::string("DeviceError(") + ex.what() + ")");
    }
}
// Many blobs against their 128 cell proofs, a verdict each: the blob source of the cell many-verification (verify_many.hip).  Count and
// arrays first (verify_host.hpp: validate_blob_cells_call), then the device list (host form: contiguous slices by item) or the owner of
// ALL THREE buffers (device form).  Nothing here takes a lane or the context's big lock: the passes run on pass slots.
CResult eth_kzg_amd_verify_blob_cell_proofs_many(const DASContext* ctx, uint64_t n, const uint8_t* const* blobs, const uint8_t* const* commitments,
                                                 const uint8_t* const* const* proofs, bool* verified, int32_t* status) {
    if (kzg::validate_blob_cells_call(n, !blobs, !commitments, !proofs, !verified) != kzg::INPUT_VALID)
        return err("InvalidInput: more than 2^24 items, or a null array");  // (before the context is looked at)
    const auto in = kzg::VerifyManyInput::host_blobs(blobs, commitments, proofs);
    auto items_ok = [&] {
        for (uint64_t i = 0; i < n; i++) verified[i] = false;
        for (uint64_t i = 0; i < n; i++) {
            if (!blobs[i] || !commitments[i] || !proofs[i]) return false;
            for (int k = 0; k < kzg::N_CELLS; k++)
                if (!proofs[i][k]) return false;
        }
        return true;
    };
    return sliced_call(ctx, n, kzg::BLOB_CELLS_MAX_ITEMS, verified, status, items_ok, [&](kzg::Engine* e, uint64_t lo, uint64_t hi, int* st, int* ver) {
        return many_failure(e, e->verify_cell_kzg_proof_batch_many(hi - lo, in.from(lo), ver + lo, st + lo));
    });
}
CResult eth_kzg_amd_verify_blob_cell_proofs_many_device(const DASContext* ctx, uint64_t n, const uint8_t* d_blobs, const uint8_t* d_commitments,
                                                        const uint8_t* d_proofs, bool* verified, int32_t* status, void* hip_stream) {
    if (kzg::validate_blob_cells_call(n, !d_blobs, !d_commitments, !d_proofs, !verified) != kzg::INPUT_VALID)
        return err("InvalidInput: more than 2^24 items, or a null array");
    live(ctx);
    if (n == 0) return ok();
    for (uint64_t i = 0; i < n; i++) verified[i] = false;
    const void* const ptrs[3] = {d_blobs, d_commitments, d_proofs};
    kzg::Engine* e = engine_of_device_pointers(ctx, ptrs, 3);
    if (!e) return err("InvalidInput: the three buffers are not device memory of one device of this context");
    return device_many(e, n, kzg::VerifyManyInput::device_blobs(d_blobs, d_commitments, d_proofs, (hipStream_t)hip_stream), verified, status);
}
// A block's data columns from blobs whose cell proofs the caller holds (data_columns.hip; under the flag verify_many.hip: the columns are
// an output of the blob source of the many-verification).  Flags, count and NULL arrays first, before the context is looked at; then the
// device list (host form: contiguous slices by blob, every slice writing its blobs' entries of the shared column arrays) or the owner of
// EVERY device buffer given (device form).  Nothing here takes a lane or the context's big lock.
static bool blobs_to_columns_args_ok(uint64_t n_blobs, bool blobs_null, bool commitments_null, bool proofs_null, uint32_t flags, bool out_proofs_given,
                                     bool verified_null) {
    if ((flags & ~(uint32_t)ETH_KZG_AMD_COLUMNS_VERIFY_PROOFS) || n_blobs > MAX_BATCH) return false;
    if (n_blobs == 0) return true;
    const bool verify = (flags & ETH_KZG_AMD_COLUMNS_VERIFY_PROOFS) != 0;
    if (blobs_null || (proofs_null && (verify || out_proofs_given))) return false;
    return !(verify && (commitments_null || verified_null));
}
CResult eth_kzg_amd_blobs_to_data_columns(const DASContext* ctx, uint64_t n_blobs, const uint8_t* const* blobs, const uint8_t* const* commitments,
                                          const uint8_t* const* const* proofs, uint32_t flags, uint8_t* const* const* out_cells,
                                          uint8_t* const* const* out_proofs, bool* verified, int32_t* status) {
    if (!blobs_to_columns_args_ok(n_blobs, !blobs, !commitments, !proofs, flags, out_proofs != nullptr, !verified))
        return err("InvalidInput: an unknown flag, more than 2^24 blobs, or a null array");
    if (n_blobs == 0) return ok();  // (an empty call looks at nothing, the context included)
    const bool verify = (flags & ETH_KZG_AMD_COLUMNS_VERIFY_PROOFS) != 0;
    auto items_ok = [&] {
        for (uint64_t i = 0; i < n_blobs; i++) {
            if (verify) verified[i] = false;
            if (!blobs[i] || (verify && !commitments[i]) || (proofs && !proofs[i])) return false;
            for (int k = 0; k < kzg::N_CELLS && proofs; k++)
                if (!proofs[i][k]) return false;
        }
        return true;
    };
    if (!verify)
        return sliced_call(ctx, n_blobs, MAX_BATCH, nullptr, status, items_ok, [&](kzg::Engine* e, uint64_t lo, uint64_t hi, int* st, int*) {
            return batch_failure(e, e->blobs_to_data_columns_host((int)lo, (int)(hi - lo), blobs, proofs, out_cells, out_proofs, st));
        });
    auto in = kzg::VerifyManyInput::host_blobs(blobs, commitments, proofs);
    in.out.cells = out_cells; in.out.proofs = out_proofs; in.out.n_total = n_blobs;
    return sliced_call(ctx, n_blobs, MAX_BATCH, verified, status, items_ok, [&](kzg::Engine* e, uint64_t lo, uint64_t hi, int* st, int* ver) {
        return many_failure(e, e->verify_cell_kzg_proof_batch_many(hi - lo, in.from(lo), ver + lo, st + lo));
    });
}
CResult eth_kzg_amd_blobs_to_data_columns_device(const DASContext* ctx, uint64_t n_blobs, const uint8_t* d_blobs, const uint8_t* d_commitments,
                                                 const uint8_t* d_proofs, uint32_t flags, uint8_t* d_out_cells, uint8_t* d_out_proofs, bool* verified,
                                                 int32_t* status, void* hip_stream) {
    if (!blobs_to_columns_args_ok(n_blobs, !d_blobs, !d_commitments, !d_proofs, flags, d_out_proofs != nullptr, !verified))
        return err("InvalidInput: an unknown flag, more than 2^24 blobs, or a null array");
    if (n_blobs == 0) return ok();
    live(ctx);
    const bool verify = (flags & ETH_KZG_AMD_COLUMNS_VERIFY_PROOFS) != 0;
    for (uint64_t i = 0; i < n_blobs && verify; i++) verified[i] = false;
    const void* ptrs[5] = {d_blobs};
    int n_ptrs = 1;
    for (const void* p : {(const void*)(verify ? d_commitments : nullptr), (const void*)d_proofs, (const void*)d_out_cells, (const void*)d_out_proofs})
        if (p) ptrs[n_ptrs++] = p;  // (without the flag the commitments are not read: not resolved either)
    kzg::Engine* e = engine_of_device_pointers(ctx, ptrs, n_ptrs);
    if (!e) return err("InvalidInput: the buffers are not device memory of one device of this context");
    if (verify) {
        auto in = kzg::VerifyManyInput::device_blobs(d_blobs, d_commitments, d_proofs, (hipStream_t)hip_stream);
        in.out.d_cells = d_out_cells; in.out.d_proofs = d_out_proofs; in.out.n_total = n_blobs;
        return device_many(e, n_blobs, in, verified, status);
    }
    static_assert(sizeof(int32_t) == sizeof(int), "status array");
    const bool sync = hip_stream == nullptr;
    if (e->blobs_to_data_columns_device((int)n_blobs, d_blobs, d_proofs, d_out_cells, d_out_proofs, (int*)status, (hipStream_t)hip_stream, sync))
        return device_err(e);
    if (status) for (uint64_t i = 0; i < n_blobs; i++) status[i] = status[i] ? kzg::ERR_SCALAR : 0;
    return ok();
}
void eth_kzg_amd_set_profiling(const DASContext* ctx, int on) { eng(ctx)->set_profiling(on != 0); }
int eth_kzg_amd_get_stage_times(const DASContext* ctx, double* ms, uint64_t* launches, int n) {
    double m[kzg::Engine::ST_COUNT];
    uint64_t l[kzg::Engine::ST_COUNT];
    eng(ctx)->get_stage_times(m, l);
    for (int i = 0; i < n && i < kzg::Engine::ST_COUNT; i++) { ms[i] = m[i]; launches[i] = l[i]; }
    return kzg::Engine::ST_COUNT;
}
// table queries: per device they describe the context's FIRST device; the byte count is the whole list's
uint64_t eth_kzg_amd_table_bytes(const DASContext* ctx) {
    live(ctx);
    uint64_t b = 0;
    std::vector<int> seen;
    for (kzg::Engine* e : ctx->engines) {  // two engines on one GPU share its tables: counted once
        bool dup = false;
        for (int d : seen) dup |= d == e->device();
        if (!dup) { b += e->table_bytes(); seen.push_back(e->device()); }
    }
    return b;
}
int eth_kzg_amd_window_bits(const DASContext* ctx) { return eng(ctx)->window_bits(); }
int eth_kzg_amd_window_count(const DASContext* ctx) { return eng(ctx)->window_count(); }
int eth_kzg_amd_glv_table(const DASContext* ctx) { (void)live(ctx); return 1; }  // deprecated: every table has been a GLV table since round 5
int eth_kzg_amd_abi_version(void) { return 6; }
int eth_kzg_amd_tables_ready(const DASContext* ctx, int wait_ms) {
    live(ctx);
    // the slowest device decides: 1 only when every device is on its final tables, 2 when a build failed somewhere, else 0
    int all = 1;
    for (kzg::Engine* e : ctx->engines) {
        const int s = e->tables_ready(wait_ms);
        if (s == 2) all = 2;
        else if (s == 0 && all != 2) all = 0;
    }
    return all;
}
void eth_kzg_amd_table_build_info(const DASContext* ctx, double* out4) { eng(ctx)->table_build_info(out4); }
int eth_kzg_amd_table_groups_ready(const DASContext* ctx) { return eng(ctx)->table_groups_ready(kzg::Engine::TAB_FK); }
void eth_kzg_amd_linmap_info(const DASContext* ctx, int32_t* out4) {
    for (int i = 0; i < 4; i++) out4[i] = eng(ctx)->linmap_info()[i];
}

}  // extern "C"
