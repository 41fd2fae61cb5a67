// recover_cells_and_kzg_proofs: host orchestration of the Reed-Solomon decode, in the list form and the device-resident form.
// Reference: recover_polynomial_coeff (crates/eip7594/src/recovery.rs:22-151),
// ReedSolomon::{construct_vanishing_poly_from_block_erasures, recover_polynomial_coefficient}
// (crates/cryptography/erasure_codes/src/reed_solomon.rs:220-262,332-384).
// Work split: every Fr transform on the GPU (k_verify.hip: k_rec_*); the host validates the cell lists (verify_host.hpp), builds the
// presence masks and stages the cells.  Cells and proofs of the recovered polynomial come from the prover's stages.
#include "engine_internal.hpp"

namespace kzg {

// Recovery of R blobs at once.  Per blob: validated cell list -> coefficients in d_coeffs_[r].
// Returns per-blob statuses in `st_out`; blobs that fail validation / decoding are skipped by the caller.
int Engine::recover_batch_to_coeffs(int R, const uint64_t* n_cells, const uint8_t* const* const* cells,
                                    const uint64_t* const* cell_indices, int* st_out) {
    hipStream_t st = stream_;
    ensure_workspace(R);
    // host: presence masks (domain order) and the flattened cell list; the vanishing polynomials are built on the GPU
    std::vector<uint32_t> present((size_t)R * 4, 0xffffffffu);  // a blob that failed validation has nothing missing
    std::vector<int> slot, stof;
    size_t total_cells = 0;
    for (int r = 0; r < R; r++) total_cells += st_out[r] == OK ? n_cells[r] : 0;
    PoolBuf hcells_buf(*this, total_cells * BYTES_PER_CELL, true);  // pinned staging: the H2D copy below runs at link speed
    uint8_t* hcells = (uint8_t*)hcells_buf.p;
    const size_t hcells_bytes = total_cells * BYTES_PER_CELL;
    slot.reserve(total_cells);
    stof.reserve(total_cells);
    size_t pos = 0;
    for (int r = 0; r < R; r++) {
        if (st_out[r] != OK) continue;
        // domain-order index of a cell = bit-reversed cell index (cosets.rs:186-195); missing = complement (recovery.rs:69-75)
        uint32_t* m = &present[(size_t)r * 4];
        m[0] = m[1] = m[2] = m[3] = 0;
        for (uint64_t k = 0; k < n_cells[r]; k++) {
            const int i = brp7((int)cell_indices[r][k]);
            m[i >> 5] |= 1u << (i & 31);
        }
        for (uint64_t k = 0; k < n_cells[r]; k++) {
            memcpy(&hcells[pos * BYTES_PER_CELL], cells[r][k], BYTES_PER_CELL);
            slot.push_back(r * N_CELLS + (int)cell_indices[r][k]);  // scatter into blob r's 128 cell slots (cosets.rs:170-175)
            stof.push_back(r);
            pos++;
        }
    }
    PoolBuf d_cellb(*this, hcells_bytes);
    if (total_cells) HIPCK(hipMemcpyAsync(d_cellb.p, hcells, hcells_bytes, hipMemcpyHostToDevice, st));
    return rs_decode(R, (const uint8_t*)d_cellb.p, /*source index = list position*/ false, slot, stof, present, st_out);
}

// Reed-Solomon decode of R blobs whose present cells are listed in `slot` (blob * 128 + cell index), `stof` (blob of each
// list entry) and `present` (domain-order masks); the cell bytes are read from d_cells at list position k, or at
// slot[k] when the caller's buffer is the flat [R][128][2048] layout.  Leaves the coefficients in d_coeffs_.
int Engine::rs_decode(int R, const uint8_t* d_cells, bool flat_source, const std::vector<int>& slot, const std::vector<int>& stof,
                      const std::vector<uint32_t>& present, int* st_out, const RsDecodeTap* tap, const std::vector<int>* src_of, bool shared_pattern,
                      const RsCommit* commit) {
    hipStream_t st = stream_;
    const int n = (int)slot.size();
    Fr seven64 = fr_u64(7);
    for (int i = 0; i < 6; i++) seven64 = sqr(seven64);
    // Rv vanishing polynomials, blob r reading the factors at r * fac_stride: one per blob, or ONE for the call when every blob misses the same cells
    const int Rv = shared_pattern ? 1 : R, fac_stride = shared_pattern ? 0 : N_CELLS;
    PoolBuf d_slot(*this, (size_t)n * sizeof(int)), d_stof(*this, (size_t)n * sizeof(int)), d_src(*this, src_of ? (size_t)n * sizeof(int) : 0);
    PoolBuf d_E(*this, (size_t)R * N_EXT * sizeof(Fr)), d_T(*this, (size_t)R * N_EXT * sizeof(Fr)), d_U(*this, (size_t)R * N_EXT * sizeof(Fr));
    PoolBuf d_zp(*this, (size_t)Rv * 65 * sizeof(Fr)), d_deg(*this, Rv * sizeof(int)), d_present(*this, present.size() * 4);
    PoolBuf d_zeval(*this, (size_t)Rv * N_CELLS * sizeof(Fr)), d_zcinv(*this, (size_t)Rv * N_CELLS * sizeof(Fr)), d_st(*this, R * sizeof(int));
    if (n) {
        HIPCK(hipMemcpyAsync(d_slot.p, slot.data(), n * sizeof(int), hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(d_stof.p, stof.data(), n * sizeof(int), hipMemcpyHostToDevice, st));
        if (src_of) HIPCK(hipMemcpyAsync(d_src.p, src_of->data(), n * sizeof(int), hipMemcpyHostToDevice, st));
    }
    HIPCK(hipMemcpyAsync(d_present.p, present.data(), present.size() * 4, hipMemcpyHostToDevice, st));
    launch::rec_vanishing_poly((const uint32_t*)d_present.p, d_w8192_, d_zp.p, (int*)d_deg.p, Rv, st);
    HIPCK(hipMemsetAsync(d_E.p, 0, (size_t)R * N_EXT * sizeof(Fr), st));
    HIPCK(hipMemsetAsync(d_st.p, 0, R * sizeof(int), st));
    if (n) launch::cells_to_fr(d_cells, d_E.p, (const int*)d_slot.p, (int*)d_st.p, (const int*)d_stof.p,
                               src_of ? (const int*)d_src.p : flat_source ? (const int*)d_slot.p : nullptr, n, st);  // E in cell order
    launch::rec_vanishing(d_zp.p, (const int*)d_deg.p, d_w8192_, to8(seven64), d_zeval.p, d_zcinv.p, Rv, st);
    launch::rec_dit_half(R, d_E.p, d_zeval.p, d_T.p, d_w8192_, st, fac_stride);                          // (E*Z) -> IFFT ...
    launch::rec_dit_last(R, d_T.p, d_coset_, n_inv8192_, d_U.p, nullptr, nullptr, d_w8192_, 0, st);      // ... * 7^i
    launch::rec_dif_half(R, d_U.p, d_zcinv.p, d_E.p, d_w8192_, st, fac_stride);                          // coset FFT, / Z
    launch::rec_dit_half(R, d_E.p, nullptr, d_T.p, d_w8192_, st);                                        // coset IFFT ...
    launch::rec_dit_last(R, d_T.p, d_coset_inv_, n_inv8192_, nullptr, d_coeffs_, (int*)d_st.p, d_w8192_, 1, st,
                         commit ? d_canon_ : nullptr);                                                  // ... * 7^-i
    if (commit) {
        // commit = MSM_4096(coefficients, monomial SRS), the stages of blob_to_kzg_commitment_device (engine_prover.hip) on the workspace
        // this call holds: 64 groups of 64 bases into d_X_, folded over the groups, compressed -- for every blob, whatever its status
        const int bp = ((R + 63) / 64) * 64;
        const int mk = mark_begin(ST_MSM_FIXED, st);
        launch::g1_set_inf(d_X_, (size_t)64 * bp, st, launch::FMT_JACS);
        launch_msm(d_canon_, TAB_SRS, d_X_, 64, R, bp, 0, st, launch::FMT_JACS);
        launch::g1_sum_positions(d_X_, 64, bp, R, st);
        mark_end(mk, 2, st);
        const int mk2 = mark_begin(ST_COMPRESS, st);
        launch::g1_compress(d_X_, commit->d_calc, 1, bp, R, st, launch::FMT_JACS);
        mark_end(mk2, 1, st);
        if (commit->d_expected) launch::commitment_check(commit->d_calc, commit->d_expected, (int*)d_st.p, R, st);
        if (commit->d_out) HIPCK(hipMemcpyAsync(commit->d_out, commit->d_calc, (size_t)R * 48, hipMemcpyDeviceToDevice, st));
        if (commit->h_out) HIPCK(hipMemcpyAsync(commit->h_out, commit->d_calc, (size_t)R * 48, hipMemcpyDeviceToHost, st));
    }
    std::vector<int> hst(R);
    HIPCK(hipMemcpyAsync(hst.data(), d_st.p, R * sizeof(int), hipMemcpyDeviceToHost, st));
    if (tap) {  // the stage hook: what the stages left, while the pool still holds it
        if (tap->deg) HIPCK(hipMemcpyAsync(tap->deg, d_deg.p, Rv * sizeof(int), hipMemcpyDeviceToHost, st));
        if (tap->zp) HIPCK(hipMemcpyAsync(tap->zp, d_zp.p, (size_t)Rv * 65 * sizeof(Fr), hipMemcpyDeviceToHost, st));
        if (tap->zeval) HIPCK(hipMemcpyAsync(tap->zeval, d_zeval.p, (size_t)Rv * N_CELLS * sizeof(Fr), hipMemcpyDeviceToHost, st));
        if (tap->zcinv) HIPCK(hipMemcpyAsync(tap->zcinv, d_zcinv.p, (size_t)Rv * N_CELLS * sizeof(Fr), hipMemcpyDeviceToHost, st));
    }
    SYNC_CHECKED(st);
    for (int r = 0; r < R; r++) {
        if (st_out[r] != OK) continue;
        if (hst[r] & 1) st_out[r] = ERR_SCALAR;
        else if (hst[r] & 4) st_out[r] = ERR_RECOVERY;
        else if (hst[r] & launch::REC_COMMITMENT_BIT) st_out[r] = ERR_COMMITMENT;
    }
    return OK;
}

// Device-resident form: d_cells is the flat [R][128][2048] extended-blob layout in HBM, present_masks[2 r .. 2 r + 1] the
// 128-bit set of cells that hold data (bit c of word c / 64); missing cells are never read.  Outputs as in the
// device-resident prover call; status[r] per blob, outputs of a failed blob are unspecified.
int Engine::recover_cells_and_kzg_proofs_device(int R, const uint8_t* d_cells, const uint64_t* present_masks, uint8_t* d_out_cells,
                                                uint8_t* d_out_proofs, int* status, hipStream_t user_stream) {
    if (R <= 0) return OK;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    if (R > device_batch_max_) {  // sub-batches on the same streams (the scratch of one pass is 0.9 MB per blob): see compute_cells_and_kzg_proofs_device
        for (int r0 = 0; r0 < R; r0 += device_batch_max_) {
            const int nr = std::min(device_batch_max_, R - r0);
            const int rc = recover_cells_and_kzg_proofs_device(nr, d_cells + (size_t)r0 * N_CELLS * BYTES_PER_CELL, present_masks + 2 * (size_t)r0,
                                                               d_out_cells ? d_out_cells + (size_t)r0 * N_CELLS * BYTES_PER_CELL : nullptr,
                                                               d_out_proofs ? d_out_proofs + (size_t)r0 * N_CELLS * 48 : nullptr, status + r0, user_stream);
            if (rc) return rc;
        }
        return OK;
    }
    try {
        HIPCK(hipSetDevice(dev_));
        ensure_workspace(R);  // also orders stream_ behind the previous asynchronous call that used the workspace
        {   // the decode runs on the library's stream: it must see what the caller's stream (NULL: the default stream) wrote into d_cells
            HIPCK(hipEventRecord(work_[0].ev_in, user_stream));
            HIPCK(hipStreamWaitEvent(stream_, work_[0].ev_in, 0));
        }
        std::vector<uint32_t> present((size_t)R * 4, 0xffffffffu);
        std::vector<int> slot, stof;
        for (int r = 0; r < R; r++) {
            const uint64_t m0 = present_masks[2 * r], m1 = present_masks[2 * r + 1];
            const int cnt = __builtin_popcountll(m0) + __builtin_popcountll(m1);
            status[r] = cnt < N_CELLS / 2 ? ERR_INPUT : OK;  // recovery.rs:90-146: at least half of the cells
            if (status[r] != OK) continue;
            uint32_t* m = &present[(size_t)r * 4];
            m[0] = m[1] = m[2] = m[3] = 0;
            for (int c = 0; c < N_CELLS; c++) {
                if (!(((c < 64 ? m0 : m1) >> (c & 63)) & 1)) continue;
                const int i = brp7(c);
                m[i >> 5] |= 1u << (i & 31);
                slot.push_back(r * N_CELLS + c);
                stof.push_back(r);
            }
        }
        int rc = rs_decode(R, d_cells, /*flat_source=*/true, slot, stof, present, status);
        if (rc) return rc;
        hipStream_t st = user_stream ? user_stream : stream_;
        if (d_out_cells) launch::coeffs_to_cells(R, d_coeffs_, d_out_cells, d_w29_, st);
        if (d_out_proofs) run_proofs_from_coeffs(R, d_out_proofs, st);
        HIPCK(hipEventRecord(work_[0].done, st));  // the next user of the workspace waits for these kernels (ensure_workspace)
        HIPCK(hipGetLastError());
        if (!user_stream) SYNC_CHECKED(st);
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

int Engine::recover_cells_and_kzg_proofs_batch_host(int R, const uint64_t* n_cells, const uint8_t* const* const* cells,
                                                    const uint64_t* n_indices, const uint64_t* const* cell_indices,
                                                    uint8_t* const* const* out_cells, uint8_t* const* const* out_proofs,
                                                    int* status) {
    if (R <= 0) return OK;
    for (int r = 0; r < R; r++) status[r] = validate_recovery(n_cells[r], n_indices[r], cell_indices[r]);
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        TraceLap lap{knobs_.trace, "recover"};
        int rc = recover_batch_to_coeffs(R, n_cells, cells, cell_indices, status);
        if (rc) return rc;
        lap("stage in + RS decode");
        // compute_multi_opening_proofs(Input::PolyCoeff) = stages C..I (prover.rs:164-170) for the whole batch
        PoolBuf d_c(*this, (size_t)R * N_CELLS * BYTES_PER_CELL), d_p(*this, (size_t)R * N_CELLS * 48);
        launch::coeffs_to_cells(R, d_coeffs_, (uint8_t*)d_c.p, d_w29_, stream_);
        run_proofs_from_coeffs(R, (uint8_t*)d_p.p, stream_);
        PoolBuf hc_buf(*this, (size_t)R * N_CELLS * BYTES_PER_CELL, true), hp_buf(*this, (size_t)R * N_CELLS * 48, true);
        const uint8_t* hc = (const uint8_t*)hc_buf.p;
        const uint8_t* hp = (const uint8_t*)hp_buf.p;
        HIPCK(hipMemcpyAsync(hc_buf.p, d_c.p, (size_t)R * N_CELLS * BYTES_PER_CELL, hipMemcpyDeviceToHost, stream_));
        HIPCK(hipMemcpyAsync(hp_buf.p, d_p.p, (size_t)R * N_CELLS * 48, hipMemcpyDeviceToHost, stream_));
        SYNC_CHECKED(stream_);
        lap("cells + proofs + D2H");
        for (int r = 0; r < R; r++) {
            if (status[r] != OK) continue;
            for (int k = 0; k < N_CELLS; k++) {
                memcpy(out_cells[r][k], &hc[((size_t)r * N_CELLS + k) * BYTES_PER_CELL], BYTES_PER_CELL);
                memcpy(out_proofs[r][k], &hp[((size_t)r * N_CELLS + k) * 48], 48);
            }
        }
        lap("scatter to caller buffers");
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

int Engine::recover_cells_and_kzg_proofs_host(uint64_t n_cells, const uint8_t* const* cells, uint64_t n_indices,
                                              const uint64_t* cell_indices, uint8_t* const* out_cells,
                                              uint8_t* const* out_proofs) {
    int st = OK;
    const uint8_t* const* cl[1] = {cells};
    const uint64_t* ix[1] = {cell_indices};
    uint8_t* const* oc[1] = {out_cells};
    uint8_t* const* op[1] = {out_proofs};
    int rc = recover_cells_and_kzg_proofs_batch_host(1, &n_cells, cl, &n_indices, ix, oc, op, &st);
    return rc ? rc : st;
}

}  // namespace kzg
