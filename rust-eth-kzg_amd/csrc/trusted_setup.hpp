// The trusted setup a context is built on: the compressed monomial points, the SHA-256 of those bytes (the identity of the setup:
// window tables are shared between the contexts of a GPU that hold the SAME setup, engine_tables.hip) and how the points are to be
// validated.  The mainnet ceremony file linked into the library (srs_blob.S) is the default instance; a caller's points come in
// through eth_kzg_amd_das_context_new_with_setup (reference: TrustedSetup::from_json / from_json_unchecked,
// crates/trusted_setup/src/lib.rs:88-124, DASContext::new(&TrustedSetup, ..), crates/eip7594/src/lib.rs:81).  HIP-free.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace kzg {

struct TrustedSetup {
    static constexpr size_t N_G1 = 4096, N_G2 = 65, G1_BYTES = 48, G2_BYTES = 96;
    using Digest = std::array<uint8_t, 32>;
    std::vector<uint8_t> g1;  // N_G1 * 48: [tau^i]_1, ZCash compressed
    std::vector<uint8_t> g2;  // N_G2 * 96: [tau^i]_2
    Digest digest{};          // SHA-256(g1 | g2)
    bool embedded = false;        // the ceremony file of the library: decompressed without a subgroup test (trusted_setup/src/lib.rs:80-86)
    bool subgroup_check = true;   // G1 on the GPU (endomorphism test, engine.hip: init_srs), G2 on the host (from_points)
    bool check_powers = false;    // the points are consecutive powers of one tau over the standard generators (engine.hip: check_powers)

    // The file linked into the library, parsed once per process.  Throws std::runtime_error if it is malformed.
    static std::shared_ptr<const TrustedSetup> mainnet();
    // A caller's points.  Host-side validation happens here, before any GPU is touched: every G2 point decodes to a curve point
    // and (subgroup_check) lies in the order-r subgroup; with check_powers, g1[0] and g2[0] are the standard generators.
    // Throws std::runtime_error whose text names the first offending index.
    static std::shared_ptr<const TrustedSetup> from_points(const uint8_t* g1, const uint8_t* g2, bool subgroup_check, bool check_powers);
    // 128-bit weights rho_0 .. rho_{n-1} of the power check: SHA-256(digest | "powers" | domain | counter), so that nobody who
    // writes a setup file can pick points with the weights in hand
    void weights128(uint8_t domain, uint32_t (*out)[4], int n) const;
};

}  // namespace kzg
