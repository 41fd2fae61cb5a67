// See trusted_setup.hpp.
#include "trusted_setup.hpp"
#include "host_pairing.hpp"
#include "sha256.hpp"

#include <cstring>
#include <mutex>
#include <stdexcept>

extern "C" const unsigned char kzg_srs_begin[];
extern "C" const unsigned char kzg_srs_end[];

namespace kzg {

static TrustedSetup::Digest digest_of(const std::vector<uint8_t>& g1, const std::vector<uint8_t>& g2) {
    TrustedSetup::Digest d;
    Sha256 h;
    h.update(g1.data(), g1.size());
    h.update(g2.data(), g2.size());
    h.finish(d.data());
    return d;
}

std::shared_ptr<const TrustedSetup> TrustedSetup::mainnet() {
    static std::mutex mu;
    static std::shared_ptr<const TrustedSetup>* inst = nullptr;  // never destroyed: helper threads may read it while the process exits
    std::lock_guard<std::mutex> lk(mu);
    if (inst) return *inst;
    // "KZGSRS01" | n_g1 | n_g2 | g1 monomial (48 B each) | g2 monomial (96 B each)
    const unsigned char* p = kzg_srs_begin;
    const size_t len = (size_t)(kzg_srs_end - kzg_srs_begin);
    uint32_t n1, n2;
    if (len < 16 || memcmp(p, "KZGSRS01", 8)) throw std::runtime_error("bad embedded SRS");
    memcpy(&n1, p + 8, 4);
    memcpy(&n2, p + 12, 4);
    if (n1 != N_G1 || n2 != N_G2 || len != 16 + N_G1 * G1_BYTES + N_G2 * G2_BYTES) throw std::runtime_error("bad embedded SRS size");
    auto s = std::make_shared<TrustedSetup>();
    s->g1.assign(p + 16, p + 16 + N_G1 * G1_BYTES);
    s->g2.assign(p + 16 + N_G1 * G1_BYTES, p + len);
    s->digest = digest_of(s->g1, s->g2);
    s->embedded = true;
    s->subgroup_check = false;
    inst = new std::shared_ptr<const TrustedSetup>(s);
    return *inst;
}

std::shared_ptr<const TrustedSetup> TrustedSetup::from_points(const uint8_t* g1, const uint8_t* g2, bool subgroup_check, bool check_powers) {
    auto s = std::make_shared<TrustedSetup>();
    s->g1.assign(g1, g1 + N_G1 * G1_BYTES);
    s->g2.assign(g2, g2 + N_G2 * G2_BYTES);
    s->digest = digest_of(s->g1, s->g2);
    s->subgroup_check = subgroup_check;
    s->check_powers = check_powers;
    const auto main = mainnet();  // (the ceremony file through this door is validated like any other; same digest, so same tables)
    pairing::init();
    for (size_t i = 0; i < N_G2; i++) {
        pairing::G2Affine q;
        if (!pairing::g2_decompress(q, s->g2.data() + i * G2_BYTES))
            throw std::runtime_error("g2_monomial[" + std::to_string(i) + "] is not the encoding of a curve point");
        if (subgroup_check && !pairing::g2_in_subgroup(q))
            throw std::runtime_error("g2_monomial[" + std::to_string(i) + "] is not in the prime-order subgroup");
    }
    if (check_powers) {  // compressed encodings are canonical: byte equality with the ceremony file's generators
        if (memcmp(s->g1.data(), main->g1.data(), G1_BYTES)) throw std::runtime_error("g1_monomial[0] is not the standard G1 generator");
        if (memcmp(s->g2.data(), main->g2.data(), G2_BYTES)) throw std::runtime_error("g2_monomial[0] is not the standard G2 generator");
    }
    return s;
}

void TrustedSetup::weights128(uint8_t domain, uint32_t (*out)[4], int n) const {
    for (int i = 0; i < n; i += 2) {  // one hash gives two weights
        uint8_t msg[32 + 6 + 1 + 4], h[32];
        memcpy(msg, digest.data(), 32);
        memcpy(msg + 32, "powers", 6);
        msg[38] = domain;
        const uint32_t ctr = (uint32_t)(i / 2);
        memcpy(msg + 39, &ctr, 4);
        Sha256 sh;
        sh.update(msg, sizeof msg);
        sh.finish(h);
        memcpy(out[i], h, 16);
        if (i + 1 < n) memcpy(out[i + 1], h + 16, 16);
    }
}

}  // namespace kzg
