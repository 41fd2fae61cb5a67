// The C symbols of the stage-level test hooks (include/c_eth_kzg_test_hooks.h).  Linked into libc_eth_kzg_hooks.so only -- the
// library tests/ loads; the product library libc_eth_kzg.so neither defines nor exports them (csrc/Makefile).
#include "../../include/c_eth_kzg_test_hooks.h"
#include "c_ctx.hpp"
#include "launch.hpp"
#include "verify_host.hpp"

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
kzg::Engine* eng(const DASContext* ctx) {
    if (!ctx || !ctx->engine) {
        fprintf(stderr, "c_eth_kzg: context pointer is null\n");
        abort();
    }
    return ctx->engine;
}
}  // namespace

extern "C" {

int eth_kzg_amd_test_fr_ntt4096(const DASContext* ctx, const uint8_t* in, uint8_t* out, int inverse_dit) {
    return eng(ctx)->test_fr_ntt4096(in, out, inverse_dit);
}
int eth_kzg_amd_test_g1_fft128(const DASContext* ctx, const uint8_t* in, uint8_t* out, int n_lanes, int inverse) {
    return eng(ctx)->test_g1_fft128(in, out, n_lanes, inverse);
}
int eth_kzg_amd_test_fixed_msm(const DASContext* ctx, const uint8_t* scalars, int n_msm, uint8_t* out) {
    return eng(ctx)->test_fixed_msm(scalars, n_msm, out);
}
int eth_kzg_amd_test_fixed_msm_ex(const DASContext* ctx, int table_kind, int mode, int scalar_form, const uint8_t* scalars, int n_slices,
                                  uint8_t* out, int32_t* modes) {
    if (!scalars || !out || !modes) return kzg::ERR_INPUT;
    return eng(ctx)->test_fixed_msm_ex(table_kind, mode, scalar_form, scalars, n_slices, out, modes);
}
int eth_kzg_amd_test_prover_scalars(const DASContext* ctx, int n, const uint8_t* blobs, uint32_t* scalars, uint64_t max_words, uint64_t* n_words,
                                    uint8_t* cells, uint8_t* proofs, int32_t* status, int32_t* fused_launches) {
    if (!blobs || !scalars || !n_words || !cells || !proofs || !status || !fused_launches) return kzg::ERR_INPUT;
    return eng(ctx)->test_prover_scalars(n, blobs, scalars, max_words, n_words, cells, proofs, status, fused_launches);
}
int eth_kzg_amd_test_proofs_from_sums(const DASContext* ctx, int program, int n, const int32_t* sums_words, uint8_t* out_proofs) {
    if (!sums_words || !out_proofs) return kzg::ERR_INPUT;
    return eng(ctx)->test_proofs_from_sums(program, n, sums_words, out_proofs);
}
int eth_kzg_amd_test_linmap_program(const DASContext* ctx, int program, uint32_t* words, uint64_t max_words, uint64_t* n_words, int32_t* launches,
                                    uint64_t max_launches, uint64_t* n_launches, int32_t* n_slots, uint8_t* consts, uint64_t max_consts,
                                    uint64_t* n_consts) {
    if (!words || !n_words || !launches || !n_launches || !n_slots || !consts || !n_consts) return kzg::ERR_INPUT;
    return eng(ctx)->test_linmap_program(program, words, max_words, n_words, launches, max_launches, n_launches, n_slots, consts, max_consts, n_consts);
}
int eth_kzg_amd_test_g1_decompress(const DASContext* ctx, const uint8_t* in, int n, int subgroup_check, int32_t* status,
                                   uint8_t* out) {
    return eng(ctx)->test_g1_decompress(in, n, subgroup_check, status, out);
}
int eth_kzg_amd_test_g1_decode(const DASContext* ctx, int form, const uint8_t* in, int n0, int n1, int32_t* status, uint8_t* out_xy) {
    if (!in || !status || !out_xy) return kzg::ERR_INPUT;
    return eng(ctx)->test_g1_decode(form, in, n0, n1, status, out_xy);
}
int eth_kzg_amd_test_field_mul(const DASContext* ctx, const uint8_t* a, const uint8_t* b, uint8_t* out, int n, int is_fp) {
    return eng(ctx)->test_field_mul(a, b, out, n, is_fp);
}
int eth_kzg_amd_test_sha256_many(const DASContext* ctx, uint64_t n, const uint8_t* prefix, uint64_t prefix_len, const uint8_t* d_body,
                                 uint64_t body_stride, uint64_t body_len, const uint8_t* d_tail, uint64_t tail_stride, uint64_t tail_len,
                                 uint8_t* d_out) {
    if (n > (1u << 24) || (prefix_len | body_len | tail_len) >> 31) return kzg::ERR_INPUT;
    return eng(ctx)->test_sha256_many((int)n, prefix, (uint32_t)prefix_len, d_body, body_stride, (uint32_t)body_len, d_tail, tail_stride,
                                      (uint32_t)tail_len, d_out);
}
int eth_kzg_amd_test_verify_msm(const DASContext* ctx, int form, const uint8_t* points, int n_pts, const uint8_t* sc0, int n0,
                                const uint8_t* sc1, int n1, uint8_t* out96, int32_t* sub_status) {
    if (!points || !sc0 || !sc1 || !out96) return kzg::ERR_INPUT;
    return eng(ctx)->test_verify_msm(form, points, n_pts, sc0, n0, sc1, n1, out96, sub_status);
}
int eth_kzg_amd_test_verify_cells_partial_device(const DASContext* ctx, uint64_t n, const uint8_t* d_commitments, const uint64_t* d_cell_indices,
                                                 const uint8_t* d_cells, const uint8_t* d_proofs, uint64_t lo, uint64_t hi, uint8_t* out96) {
    if (!d_commitments || !d_cell_indices || !d_cells || !d_proofs || !out96) return kzg::ERR_INPUT;
    return eng(ctx)->test_verify_cells_partial_device(n, d_commitments, d_cell_indices, d_cells, d_proofs, lo, hi, out96);
}
int eth_kzg_amd_test_verify_blob_batch_inputs(const DASContext* ctx, uint64_t n, int on_device, const void* blobs, const void* commitments,
                                              const void* proofs, uint8_t* out96, int32_t* verified) {
    if (!blobs || !commitments || !proofs || !out96 || !verified) return kzg::ERR_INPUT;
    int v = 0;
    const int rc = eng(ctx)->test_verify_blob_batch_inputs(n, on_device, blobs, commitments, proofs, out96, &v);
    *verified = v;
    return rc;
}
int eth_kzg_amd_test_cell_leaf_digests(const DASContext* ctx, uint64_t n, const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells,
                                       const uint8_t* proofs, uint8_t* out_digests) {
    if (!commitments || !cell_indices || !cells || !proofs || !out_digests) return kzg::ERR_INPUT;
    return eng(ctx)->test_cell_leaf_digests(n, commitments, cell_indices, cells, proofs, out_digests);
}
int eth_kzg_amd_test_verify_cells_inputs_ex(const DASContext* ctx, uint64_t n, int on_device, const void* commitments, const void* cell_indices,
                                            const void* cells, const void* proofs, uint32_t flags, uint8_t* root32, uint8_t* out96) {
    if (!commitments || !cell_indices || !cells || !proofs || !root32 || !out96 || (flags & ~ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT)) return kzg::ERR_INPUT;
    return eng(ctx)->test_verify_cells_inputs_ex(n, on_device, commitments, cell_indices, cells, proofs, flags, root32, out96);
}
int eth_kzg_amd_test_verify_many_sums(const DASContext* ctx, uint64_t n_batches, const uint64_t* commitments_lengths,
                                      const uint8_t* const* const* commitments, const uint64_t* cell_indices_lengths,
                                      const uint64_t* const* cell_indices, const uint64_t* cells_lengths, const uint8_t* const* const* cells,
                                      const uint64_t* proofs_lengths, const uint8_t* const* const* proofs, int32_t* verified, int32_t* status,
                                      int32_t* form4, uint8_t* sums96, uint32_t* rho, uint8_t* fold96, int32_t* probe_ranges, uint8_t* probe_sums96,
                                      uint64_t max_probes, uint64_t* n_probes) {
    if (!commitments_lengths || !commitments || !cell_indices_lengths || !cell_indices || !cells_lengths || !cells || !proofs_lengths || !proofs ||
        !verified || !status || !form4 || !sums96 || !rho || !fold96 || !n_probes || (max_probes && (!probe_ranges || !probe_sums96)))
        return kzg::ERR_INPUT;
    const auto in = kzg::VerifyManyInput::lists(commitments_lengths, commitments, cell_indices_lengths, cell_indices, cells_lengths, cells, proofs_lengths,
                                                proofs, /*leaf=*/false);
    return eng(ctx)->test_verify_many_sums_in(n_batches, in, verified, status, form4, sums96, rho, fold96, probe_ranges, probe_sums96, max_probes, n_probes,
                                              nullptr, nullptr);
}
// the same pass over either source and with either challenge
int eth_kzg_amd_test_verify_many_sums_ex(const DASContext* ctx, uint64_t n_batches, const uint64_t* commitments_lengths,
                                         const uint8_t* const* const* commitments, const uint64_t* cell_indices_lengths,
                                         const uint64_t* const* cell_indices, const uint64_t* cells_lengths, const uint8_t* const* const* cells,
                                         const uint64_t* proofs_lengths, const uint8_t* const* const* proofs, uint32_t flags, int32_t* verified,
                                         int32_t* status, int32_t* form4, uint8_t* sums96, uint32_t* rho, uint8_t* fold96, int32_t* probe_ranges,
                                         uint8_t* probe_sums96, uint64_t max_probes, uint64_t* n_probes, uint8_t* digests32, uint8_t* leaves32) {
    if (!commitments_lengths || !commitments || !cell_indices_lengths || !cell_indices || !cells_lengths || !cells || !proofs_lengths || !proofs ||
        !verified || !status || !form4 || !sums96 || !rho || !fold96 || !n_probes || !digests32 || (max_probes && (!probe_ranges || !probe_sums96)) ||
        (flags & ~ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT))
        return kzg::ERR_INPUT;
    const auto in = kzg::VerifyManyInput::lists(commitments_lengths, commitments, cell_indices_lengths, cell_indices, cells_lengths, cells, proofs_lengths,
                                                proofs, flags != 0);
    return eng(ctx)->test_verify_many_sums_in(n_batches, in, verified, status, form4, sums96, rho, fold96, probe_ranges, probe_sums96, max_probes, n_probes,
                                              digests32, leaves32);
}
int eth_kzg_amd_test_verify_many_sums_device(const DASContext* ctx, uint64_t n_batches, const uint64_t* cell_starts, const uint8_t* d_commitments,
                                             const uint64_t* d_cell_indices, const uint8_t* d_cells, const uint8_t* d_proofs, uint32_t flags,
                                             int32_t* verified, int32_t* status, int32_t* form4, uint8_t* sums96, uint32_t* rho, uint8_t* fold96,
                                             int32_t* probe_ranges, uint8_t* probe_sums96, uint64_t max_probes, uint64_t* n_probes, uint8_t* digests32,
                                             uint8_t* leaves32) {
    if (!verified || !status || !form4 || !sums96 || !rho || !fold96 || !n_probes || !digests32 || (max_probes && (!probe_ranges || !probe_sums96)) ||
        (flags & ~ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT) || n_batches < 1 || n_batches > (1u << 20) ||
        kzg::validate_cell_starts(n_batches, cell_starts) != kzg::INPUT_VALID)
        return kzg::ERR_INPUT;
    if (cell_starts[n_batches] && (!d_commitments || !d_cell_indices || !d_cells || !d_proofs)) return kzg::ERR_INPUT;
    const auto in = kzg::VerifyManyInput::flat_device(cell_starts, d_commitments, d_cell_indices, d_cells, d_proofs, nullptr, flags != 0);
    return eng(ctx)->test_verify_many_sums_in(n_batches, in, verified, status, form4, sums96, rho, fold96, probe_ranges, probe_sums96, max_probes, n_probes,
                                              digests32, leaves32);
}
// the tap on a pass of the column source (eth_kzg_amd_verify_data_columns / _device)
int eth_kzg_amd_test_verify_data_columns_sums(const DASContext* ctx, uint64_t n_blobs, int on_device, const void* commitments, uint64_t n_columns,
                                              const uint64_t* column_indices, const void* cells, const void* proofs, uint32_t flags, int32_t* verified,
                                              int32_t* status, int32_t* form4, uint8_t* sums96, uint32_t* rho, uint8_t* fold96, int32_t* probe_ranges,
                                              uint8_t* probe_sums96, uint64_t max_probes, uint64_t* n_probes, uint8_t* digests32, uint8_t* leaves32,
                                              uint64_t* counts2) {
    if (!verified || !status || !form4 || !sums96 || !rho || !fold96 || !n_probes || !digests32 || !counts2 || (max_probes && (!probe_ranges || !probe_sums96)) ||
        (on_device != 0 && on_device != 1) || n_columns < 1 || n_columns > (1u << 20) ||
        kzg::validate_data_columns_call(flags, ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT, n_blobs, n_columns, !commitments, !column_indices, !cells, !proofs, false) !=
            kzg::INPUT_VALID)
        return kzg::ERR_INPUT;
    const auto in = on_device ? kzg::VerifyManyInput::device_columns(n_blobs, (const uint8_t*)commitments, column_indices, (const uint8_t*)cells,
                                                                     (const uint8_t*)proofs, nullptr, flags != 0)
                              : kzg::VerifyManyInput::host_columns(n_blobs, (const uint8_t* const*)commitments, column_indices,
                                                                   (const uint8_t* const* const*)cells, (const uint8_t* const* const*)proofs, flags != 0);
    return eng(ctx)->test_verify_many_sums_in(n_columns, in, verified, status, form4, sums96, rho, fold96, probe_ranges, probe_sums96, max_probes, n_probes,
                                              digests32, leaves32, counts2);
}
// the tap on a pass of the partial spelling (eth_kzg_amd_verify_partial_data_columns / _device)
int eth_kzg_amd_test_verify_partial_data_columns_sums(const DASContext* ctx, uint64_t n_blobs, int on_device, const void* commitments, uint64_t n_columns,
                                                      const uint64_t* column_indices, const void* present, const void* cells, const void* proofs,
                                                      uint32_t flags, int32_t* verified, int32_t* status, int32_t* form4, uint8_t* sums96, uint32_t* rho,
                                                      uint8_t* fold96, int32_t* probe_ranges, uint8_t* probe_sums96, uint64_t max_probes, uint64_t* n_probes,
                                                      uint8_t* digests32, uint8_t* leaves32, uint64_t* counts2) {
    if (!verified || !status || !form4 || !sums96 || !rho || !fold96 || !n_probes || !digests32 || !counts2 || (max_probes && (!probe_ranges || !probe_sums96)) ||
        (on_device != 0 && on_device != 1) || n_columns < 1 || n_columns > (1u << 20) ||
        kzg::validate_partial_columns_call(flags, ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT, n_blobs, n_columns, !commitments, !column_indices, !present, !cells,
                                           !proofs, false) != kzg::INPUT_VALID)
        return kzg::ERR_INPUT;
    try {
    kzg::PartialColumns pc;
    if (on_device) pc.from_flat(n_blobs, n_columns, column_indices, (const uint64_t*)present);
    else pc.from_list(n_blobs, n_columns, column_indices, (const uint64_t* const*)present);
    const auto in = on_device ? kzg::VerifyManyInput::device_partial_columns(pc, (const uint8_t*)commitments, column_indices, (const uint8_t*)cells,
                                                                             (const uint8_t*)proofs, nullptr, flags != 0)
                              : kzg::VerifyManyInput::host_partial_columns(pc, (const uint8_t* const*)commitments, column_indices,
                                                                           (const uint8_t* const* const*)cells, (const uint8_t* const* const*)proofs,
                                                                           flags != 0);
    return eng(ctx)->test_verify_many_sums_in(n_columns, in, verified, status, form4, sums96, rho, fold96, probe_ranges, probe_sums96, max_probes, n_probes,
                                              digests32, leaves32, counts2);
    } catch (const std::exception&) {  // (the column plan allocates)
        return kzg::ERR_DEVICE;
    }
}
int eth_kzg_amd_test_verify_kzg_proof_many_sums(const DASContext* ctx, uint64_t n, int on_device, const void* commitments, const void* zs, const void* ys,
                                                const void* proofs, uint64_t forced_pass, int32_t* verified, int32_t* status, uint64_t* pass_starts,
                                                uint64_t max_passes, uint64_t* n_passes, uint8_t* leaves32, uint8_t* seeds32, uint32_t* rho, uint8_t* fold96,
                                                int32_t* fold_verdicts, int32_t* probes4, uint8_t* probe_sums96, uint64_t max_probes, uint64_t* n_probes) {
    if (!commitments || !zs || !ys || !proofs || !verified || !status || !pass_starts || !n_passes || !leaves32 || !seeds32 || !rho || !fold96 ||
        !fold_verdicts || !n_probes || (max_probes && (!probes4 || !probe_sums96)) || (on_device != 0 && on_device != 1))
        return kzg::ERR_INPUT;
    kzg::PointManyInput in;
    in.on_device = on_device != 0;
    if (on_device) {
        in.d_commitments = (const uint8_t*)commitments; in.d_zs = (const uint8_t*)zs; in.d_ys = (const uint8_t*)ys; in.d_proofs = (const uint8_t*)proofs;
    } else {
        in.commitments = (const uint8_t* const*)commitments; in.zs = (const uint8_t* const*)zs; in.ys = (const uint8_t* const*)ys;
        in.proofs = (const uint8_t* const*)proofs;
    }
    return eng(ctx)->test_verify_kzg_proof_many_sums(n, in, forced_pass, verified, status, pass_starts, max_passes, n_passes, leaves32, seeds32, rho, fold96,
                                                     fold_verdicts, probes4, probe_sums96, max_probes, n_probes);
}
int eth_kzg_amd_test_blob_eval_at(const DASContext* ctx, uint64_t n, const uint8_t* const* blobs, const uint8_t* zs_be32, uint8_t* out_ys_be32,
                                  int32_t* out_bad) {
    if (n < 1 || n > 4096 || !blobs || !zs_be32 || !out_ys_be32 || !out_bad) return kzg::ERR_INPUT;
    for (uint64_t b = 0; b < n; b++)
        if (!blobs[b]) return kzg::ERR_INPUT;
    return eng(ctx)->test_blob_eval_at((int)n, blobs, zs_be32, out_ys_be32, out_bad);
}
int eth_kzg_amd_test_verify_blob_kzg_proof_many_sums(const DASContext* ctx, uint64_t n, int on_device, const void* blobs, const void* commitments,
                                                     const void* proofs, uint64_t forced_pass, int32_t* verified, int32_t* status, uint64_t* pass_starts,
                                                     uint64_t max_passes, uint64_t* n_passes, uint8_t* leaves32, uint8_t* seeds32, uint32_t* rho,
                                                     uint8_t* fold96, int32_t* fold_verdicts, int32_t* probes4, uint8_t* probe_sums96, uint64_t max_probes,
                                                     uint64_t* n_probes, uint8_t* zs32, uint8_t* ys32) {
    if (!blobs || !commitments || !proofs || !verified || !status || !pass_starts || !n_passes || !leaves32 || !seeds32 || !rho || !fold96 ||
        !fold_verdicts || !n_probes || !zs32 || !ys32 || (max_probes && (!probes4 || !probe_sums96)) || (on_device != 0 && on_device != 1))
        return kzg::ERR_INPUT;
    kzg::PointManyInput in;
    in.from_blobs = true;
    in.on_device = on_device != 0;
    if (on_device) {
        in.d_blobs = (const uint8_t*)blobs; in.d_commitments = (const uint8_t*)commitments; in.d_proofs = (const uint8_t*)proofs;
    } else {
        in.blobs = (const uint8_t* const*)blobs; in.commitments = (const uint8_t* const*)commitments; in.proofs = (const uint8_t* const*)proofs;
    }
    return eng(ctx)->test_verify_kzg_proof_many_sums(n, in, forced_pass, verified, status, pass_starts, max_passes, n_passes, leaves32, seeds32, rho, fold96,
                                                     fold_verdicts, probes4, probe_sums96, max_probes, n_probes, zs32, ys32);
}
int eth_kzg_amd_test_blob_extension(const DASContext* ctx, uint64_t n, const uint8_t* const* blobs, uint8_t* out_cells, int32_t* out_bad) {
    if (n < 1 || n > 1024 || !blobs || !out_cells || !out_bad) return kzg::ERR_INPUT;
    for (uint64_t b = 0; b < n; b++)
        if (!blobs[b]) return kzg::ERR_INPUT;
    return eng(ctx)->test_blob_extension((int)n, blobs, out_cells, out_bad);
}
int eth_kzg_amd_test_blob_to_columns(const DASContext* ctx, uint64_t n, const uint8_t* const* blobs, uint64_t n_total, uint64_t b0, int blob_half,
                                     uint8_t* matrix, int32_t* out_bad) {
    if (n < 1 || n > 1024 || n_total > 4096 || b0 > n_total || n > n_total - b0 || !blobs || !matrix || !out_bad) return kzg::ERR_INPUT;
    for (uint64_t b = 0; b < n; b++)
        if (!blobs[b]) return kzg::ERR_INPUT;
    return eng(ctx)->test_blob_to_columns((int)n, blobs, n_total, b0, blob_half, matrix, out_bad);
}
// the tap on a pass of the blob source of the cell many-verification (eth_kzg_amd_verify_blob_cell_proofs_many / _many_device)
int eth_kzg_amd_test_verify_blob_cell_proofs_sums(const DASContext* ctx, uint64_t n, int on_device, const void* blobs, const void* commitments,
                                                  const void* proofs, int32_t* verified, int32_t* status, int32_t* form4, uint8_t* sums96, uint32_t* rho,
                                                  uint8_t* fold96, int32_t* probe_ranges, uint8_t* probe_sums96, uint64_t max_probes, uint64_t* n_probes,
                                                  uint8_t* digests32, uint8_t* leaves32) {
    if (!blobs || !commitments || !proofs || !verified || !status || !form4 || !sums96 || !rho || !fold96 || !n_probes || !digests32 ||
        (max_probes && (!probe_ranges || !probe_sums96)) || (on_device != 0 && on_device != 1) || n < 1 || n > (1u << 20))
        return kzg::ERR_INPUT;
    const auto in = on_device ? kzg::VerifyManyInput::device_blobs((const uint8_t*)blobs, (const uint8_t*)commitments, (const uint8_t*)proofs, nullptr)
                              : kzg::VerifyManyInput::host_blobs((const uint8_t* const*)blobs, (const uint8_t* const*)commitments,
                                                                 (const uint8_t* const* const*)proofs);
    return eng(ctx)->test_verify_many_sums_in(n, in, verified, status, form4, sums96, rho, fold96, probe_ranges, probe_sums96, max_probes, n_probes,
                                              digests32, leaves32);
}
int eth_kzg_amd_test_pairing_check_many(const DASContext* ctx, int key, uint64_t n, const uint8_t* pairs, int rescale, int8_t* out_gpu, int8_t* out_host,
                                        uint8_t* out_miller_gpu, uint8_t* out_miller_host) {
    if ((key != 0 && key != 1) || n < 1 || n > (1u << 16) || !pairs || !out_gpu || !out_host || rescale < 0) return kzg::ERR_INPUT;
    return eng(ctx)->test_pairing_check_many(key, n, pairs, rescale, out_gpu, out_host, out_miller_gpu, out_miller_host);
}
int eth_kzg_amd_test_search_stats(const DASContext* ctx, uint64_t* out4) {
    if (!out4) return kzg::ERR_INPUT;
    eng(ctx)->test_search_stats(out4);
    return 0;
}
int eth_kzg_amd_test_rs_decode(const DASContext* ctx, int R, const uint64_t* n_cells, const uint64_t* const* cell_indices,
                               const uint8_t* const* const* cells, int flat_source, int32_t* status, int32_t* deg, uint8_t* zp, uint8_t* zeval,
                               uint8_t* zcinv, uint8_t* coeffs) {
    // every count and index before anything is launched: k_rec_vanishing_poly is defined for at most 64 roots, the scatter for slots < 128
    if (R < 1 || R > 4096 || !n_cells || !cell_indices || !cells || (flat_source != 0 && flat_source != 1)) return kzg::ERR_INPUT;
    for (int r = 0; r < R; r++) {
        if (n_cells[r] < 64 || n_cells[r] > 128 || !cell_indices[r] || !cells[r]) return kzg::ERR_INPUT;
        for (uint64_t k = 0; k < n_cells[r]; k++) {
            if (cell_indices[r][k] >= 128 || (k && cell_indices[r][k - 1] >= cell_indices[r][k])) return kzg::ERR_INPUT;
            if (!cells[r][flat_source ? 0 : k]) return kzg::ERR_INPUT;
        }
    }
    return eng(ctx)->test_rs_decode(R, n_cells, cell_indices, cells, flat_source, status, deg, zp, zeval, zcinv, coeffs);
}
int eth_kzg_amd_test_op_info(int op, int32_t* in_words, int32_t* out_words, int32_t* device_only, const char** name) {
    int i, o, d;
    const char* nm;
    if (kzg::launch::test_op_info(op, &i, &o, &d, &nm) != 0) return -1;
    *in_words = i;
    *out_words = o;
    *device_only = d;
    *name = nm;
    return 0;
}
int eth_kzg_amd_test_op(const DASContext* ctx, int op, int n, const int32_t* in, int32_t* out, int on_device) {
    if (on_device) return eng(ctx)->test_op(op, n, in, out);
    int i, o, d;
    const char* nm;
    if (kzg::launch::test_op_info(op, &i, &o, &d, &nm) != 0 || d || n <= 0) return kzg::ERR_INPUT;  // device-only forms have no host pass
    return kzg::launch::test_op_host(op, n, in, out) == 0 ? 0 : kzg::ERR_INPUT;
}

static bool glv_shape_ok(int c, int n_groups, int nb) {
    return kzg::launch::glv_width_supported(c) && n_groups >= 1 && n_groups <= 128 && nb >= 1 && nb <= 64;
}
int eth_kzg_amd_test_table_info(const DASContext* ctx, int kind, int which, int64_t* out8, int32_t* piece_first_block, int max_pieces) {
    return eng(ctx)->test_table_info(kind, which, out8, piece_first_block, max_pieces);
}
int eth_kzg_amd_test_table_audit(const DASContext* ctx, int kind, int which, uint64_t* visited, uint64_t* n_findings, int32_t* findings,
                                 int max_findings, double* ms) {
    return eng(ctx)->test_table_audit(kind, which, visited, n_findings, findings, max_findings, ms);
}
int eth_kzg_amd_test_table_read(const DASContext* ctx, int kind, int which, int group, int window, int base, int d0, int n, uint32_t* out) {
    return eng(ctx)->test_table_read(kind, which, group, window, base, d0, n, out);
}
int eth_kzg_amd_test_table_audit_buffer(const DASContext* ctx, int c, int n_groups, int nb, const uint32_t* table, const uint8_t* bases,
                                        int on_device, uint64_t* visited, uint64_t* n_findings, int32_t* findings, int max_findings) {
    if (!glv_shape_ok(c, n_groups, nb) || max_findings < 0) return kzg::ERR_INPUT;
    if (on_device) return eng(ctx)->test_table_audit_buffer(c, n_groups, nb, table, bases, visited, n_findings, findings, max_findings);
    // the host pass of the same source: no GPU, no context
    const int WL = kzg::launch::glv_lower_windows(c), W = kzg::launch::glv_windows(c);
    const size_t lower = kzg::launch::glv_entries_per_base(c, 0, WL) * (size_t)nb, upper = kzg::launch::glv_entries_per_base(c, WL, W) * (size_t)nb;
    std::vector<const void*> blocks((size_t)2 * n_groups);
    const char* t = (const char*)table;
    for (int g = 0; g < n_groups; g++) {
        blocks[2 * g] = t + (size_t)g * (lower + upper) * kzg::launch::SIZEOF_TABP;
        blocks[2 * g + 1] = t + ((size_t)g * (lower + upper) + lower) * kzg::launch::SIZEOF_TABP;
    }
    unsigned long long v = 0, nf = 0;
    kzg::launch::table_audit_host(blocks.data(), bases, c, n_groups, nb, &v, &nf, findings, max_findings);
    std::vector<std::array<int32_t, 5>> f(std::min<unsigned long long>(nf, (unsigned long long)max_findings));
    if (!f.empty()) {
        memcpy(f.data(), findings, f.size() * sizeof(f[0]));
        std::sort(f.begin(), f.end());
        memcpy(findings, f.data(), f.size() * sizeof(f[0]));
    }
    *visited = v;
    *n_findings = nf;
    return 0;
}

}  // extern "C"
