// A block's data columns in column layout: the proposer's call (commitments, cells and proofs of every blob, cells and proofs laid
// out [column][blob] as the 128 sidecars carry them) and the supernode's call (all 128 columns from at least 64 of them).
// c_eth_kzg.h: eth_kzg_amd_compute_data_columns / _device, eth_kzg_amd_recover_data_columns / _device, and the recovery checked against
// the block's commitments, eth_kzg_amd_recover_data_columns_checked / _device.
//
// Neither call computes anything new: the prover's stages are enqueue_compute's and the decoder is rs_decode.  What is new is WHERE the
// kernels that write the outputs put them -- k_coeffs_to_cells / _scalars and k_g1_compress store every byte once, so the layout is
// their destination address (launch::Columns) and no transposition pass exists -- and what is computed once per call instead of
// once per blob or per product: the blobs' decode (one k_blob_to_coeffs launch per sub-batch feeds the commitment MSM and the
// proofs) and the vanishing polynomial of a recovery (every blob of a block misses the same columns).
#include "engine_internal.hpp"

namespace kzg {

// ---- the prover's call ---------------------------------------------------------------------------------------------------------
void Engine::ensure_commit_scratch(Work& w, int n) {
    if (n <= w.col_cap) return;
    const int cap = ((n + 63) / 64) * 64;
    void** ptrs[] = {&w.col_canon, &w.col_sums};
    for (void** p : ptrs)
        if (*p) { HIPCK(hipFree(*p)); *p = nullptr; }
    w.col_cap = 0;
    HIPCK(hipMalloc(&w.col_canon, (size_t)cap * N_BLOB * sizeof(Fr)));
    HIPCK(hipMalloc(&w.col_sums, (size_t)cap * 64 * launch::SIZEOF_JACS));
    w.col_cap = cap;
}
// blob_to_kzg_commitment_device's stages behind the decode, on the work set of the proofs instead of work_[0] under the engine's lock:
// commit = MSM_4096(canonical coefficients, monomial SRS) as 64 groups of 64 bases, folded over the groups.  (One position per blob:
// the blob-major and the column address of a commitment are the same, d_commitments + 48 b.)
void Engine::enqueue_commitments(Work& w, int n, uint8_t* d_commitments, hipStream_t st) {
    const int bp = ((n + 63) / 64) * 64;
    const int mk = mark_begin(ST_MSM_FIXED, st);
    launch::g1_set_inf(w.col_sums, (size_t)64 * bp, st, launch::FMT_JACS);
    launch_msm(w.col_canon, TAB_SRS, w.col_sums, 64, n, bp, 0, st, launch::FMT_JACS);
    launch::g1_sum_positions(w.col_sums, 64, bp, n, st);
    mark_end(mk, 2, st);
    const int mk2 = mark_begin(ST_COMPRESS, st);
    launch::g1_compress(w.col_sums, d_commitments, 1, bp, n, st, launch::FMT_JACS);
    mark_end(mk2, 1, st);
}

int Engine::compute_data_columns_device(int n, const uint8_t* d_blobs, uint8_t* d_commitments, uint8_t* d_cells, uint8_t* d_proofs, int* h_status,
                                        hipStream_t st, bool sync) {
    return prover_device(n, d_blobs, d_commitments, d_cells, d_proofs, h_status, st, sync, /*columns=*/true);
}

// Host pointers: chunks of at most CHUNK blobs through the work set's staging -- blobs gathered into pinned memory and uploaded, the
// chunk's columns computed as a [128][ns] matrix of its own (launch::Columns{ns, 0}), brought down and scattered to out_*[c][lo + b].
int Engine::compute_data_columns_host(int lo, int n, const uint8_t* const* blobs, uint8_t* const* out_commitments, uint8_t* const* const* out_cells,
                                      uint8_t* const* const* out_proofs, int* h_status) {
    if (n <= 0) return OK;
    constexpr int CHUNK = 256;  // a block holds a few dozen blobs; 256 are 105 MB of staging on either side of the link
    Work* held = nullptr;
    try {
        HIPCK(hipSetDevice(dev_));
        Work& w = lease_work(1, NW - 1);
        held = &w;
        for (int s0 = 0; s0 < n; s0 += CHUNK) {
            const int ns = std::min(CHUNK, n - s0), first = lo + s0;
            ensure_staging(w, ns);
            if (out_commitments && ns > w.comm_cap) {
                if (w.d_comm) HIPCK(hipFree(w.d_comm));
                if (w.h_comm) HIPCK(hipHostFree(w.h_comm));
                w.d_comm = w.h_comm = nullptr;
                w.comm_cap = 0;
                HIPCK(hipMalloc(&w.d_comm, (size_t)ns * 48));
                HIPCK(hipHostMalloc(&w.h_comm, (size_t)ns * 48, hipHostMallocDefault));
                w.comm_cap = ns;
            }
            for (int b = 0; b < ns; b++) memcpy(w.h_in + (size_t)b * BYTES_PER_BLOB, blobs[first + b], BYTES_PER_BLOB);
            HIPCK(hipStreamWaitEvent(w.stream, w.done, 0));
            HIPCK(hipMemcpyAsync(w.d_in, w.h_in, (size_t)ns * BYTES_PER_BLOB, hipMemcpyHostToDevice, w.stream));
            const launch::Columns cols{(size_t)ns, 0};
            enqueue_compute(w, ns, w.d_in, out_cells ? w.d_cells : nullptr, out_proofs ? w.d_proofs : nullptr, w.stream, nullptr, &cols,
                            out_commitments ? w.d_comm : nullptr);
            HIPCK(hipMemcpyAsync(w.h_status, w.status, (size_t)ns * sizeof(int), hipMemcpyDeviceToHost, w.stream));
            if (out_commitments) HIPCK(hipMemcpyAsync(w.h_comm, w.d_comm, (size_t)ns * 48, hipMemcpyDeviceToHost, w.stream));
            if (out_cells) HIPCK(hipMemcpyAsync(w.h_cells, w.d_cells, (size_t)ns * N_CELLS * BYTES_PER_CELL, hipMemcpyDeviceToHost, w.stream));
            if (out_proofs) HIPCK(hipMemcpyAsync(w.h_proofs, w.d_proofs, (size_t)ns * N_CELLS * 48, hipMemcpyDeviceToHost, w.stream));
            HIPCK(hipEventRecord(w.done, w.stream));
            HIPCK(hipGetLastError());
            HIPCK(hipStreamSynchronize(w.stream));
            for (int b = 0; b < ns; b++) {
                if (h_status) h_status[first + b] = w.h_status[b] ? ERR_SCALAR : OK;
                if (w.h_status[b]) continue;  // a refused blob: its slots stay as the caller left them
                if (out_commitments) memcpy(out_commitments[first + b], w.h_comm + (size_t)b * 48, 48);
            }
            for (int c = 0; c < N_CELLS; c++)
                for (int b = 0; b < ns; b++) {
                    if (w.h_status[b]) continue;
                    if (out_cells) memcpy(out_cells[c][first + b], w.h_cells + ((size_t)c * ns + b) * BYTES_PER_CELL, BYTES_PER_CELL);
                    if (out_proofs) memcpy(out_proofs[c][first + b], w.h_proofs + ((size_t)c * ns + b) * 48, 48);
                }
        }
        release_work(w);
        held = nullptr;
    } catch (const std::exception& e) {
        if (held) {
            (void)hipStreamSynchronize(held->stream);
            (void)hipStreamSynchronize(held->copy);
            release_work(*held);
        }
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// ---- the call of a node that holds the proofs --------------------------------------------------------------------------------------
// eth_kzg_amd_blobs_to_data_columns without its flag (with it: verify_many.hip, an output of the blob source).  No FK20, so nothing of
// the prover's stages: ONE launch of k_blob_to_columns computes every blob's cells inside the CU and stores them at their column
// addresses, one launch of k_proofs_to_columns re-orders the proofs the caller holds.  Of a work set the call takes the streams, the
// staging of the host form and the status words below; coefficients, scalars and point arrays are never allocated for it.
static void ensure_sidecar_status(Work& w, int n) {
    if (n <= w.sc_cap) return;
    if (w.sc_status) { HIPCK(hipFree(w.sc_status)); w.sc_status = nullptr; }
    w.sc_cap = 0;
    const int cap = ((n + 63) / 64) * 64;
    HIPCK(hipMalloc(&w.sc_status, (size_t)cap * sizeof(int)));
    w.sc_cap = cap;
}
int Engine::blobs_to_data_columns_device(int n, const uint8_t* d_blobs, const uint8_t* d_proofs, uint8_t* d_cells, uint8_t* d_out_proofs, int* h_status,
                                         hipStream_t st, bool sync) {
    if (n <= 0) return OK;
    Work* held = nullptr;
    try {
        HIPCK(hipSetDevice(dev_));
        Work& w = lease_work(1, NW - 1);
        held = &w;
        if (!st) {  // NULL: the library's stream, ordered behind whatever the caller has queued on the default stream so far
            st = w.stream;
            HIPCK(hipEventRecord(w.ev_in, nullptr));
            HIPCK(hipStreamWaitEvent(st, w.ev_in, 0));
        }
        const launch::Columns cols{(size_t)n, 0};
        // the status words are the set's: they are idle whenever the set is free, because a call that asks for them leaves synchronised
        if (h_status) {
            ensure_sidecar_status(w, n);
            HIPCK(hipMemsetAsync(w.sc_status, 0, (size_t)n * sizeof(int), st));
        }
        if (d_cells || h_status) launch::blob_to_columns(n, d_blobs, d_cells, cols, /*blob_half=*/true, h_status ? w.sc_status : nullptr, d_w29_, n_inv4096_, st);
        if (d_out_proofs) launch::proofs_to_columns(n, d_proofs, d_out_proofs, cols, st);
        if (h_status) HIPCK(hipMemcpyAsync(h_status, w.sc_status, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCK(hipGetLastError());
        if (sync || h_status) HIPCK(hipStreamSynchronize(st));
        release_work(w);
        held = nullptr;
    } catch (const std::exception& e) {
        if (held) {
            (void)hipStreamSynchronize(st);
            release_work(*held);
        }
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// Host pointers: chunks of at most CHUNK blobs through the work set's staging.  Every blob goes up ONCE; the kernel writes rows 64..127
// of the chunk's [128][ns] matrix only, and that half alone comes down (128 KB per blob): cells 0..63 are the caller's own blob bytes,
// which the helper threads copy across on the host together with the proofs while nothing of them crosses the link.
int Engine::blobs_to_data_columns_host(int lo, int n, const uint8_t* const* blobs, const uint8_t* const* const* proofs, uint8_t* const* const* out_cells,
                                       uint8_t* const* const* out_proofs, int* h_status) {
    if (n <= 0) return OK;
    constexpr int CHUNK = 256;
    HostPool* pool = n >= 4 ? ensure_host_pool() : nullptr;  // a couple of blobs: everything on the calling thread
    const int T = pool ? pool->threads() + 1 : 1;
    Work* held = nullptr;
    try {
        HIPCK(hipSetDevice(dev_));
        Work& w = lease_work(1, NW - 1);
        held = &w;
        for (int s0 = 0; s0 < n; s0 += CHUNK) {
            const int ns = std::min(CHUNK, n - s0), first = lo + s0;
            ensure_staging(w, ns);
            ensure_sidecar_status(w, ns);
            parallel_for(ns, T, pool, [&](int b) { memcpy(w.h_in + (size_t)b * BYTES_PER_BLOB, blobs[first + b], BYTES_PER_BLOB); });
            HIPCK(hipStreamWaitEvent(w.stream, w.done, 0));  // (the staging is shared with the prover's host forms)
            HIPCK(hipMemcpyAsync(w.d_in, w.h_in, (size_t)ns * BYTES_PER_BLOB, hipMemcpyHostToDevice, w.stream));
            HIPCK(hipMemsetAsync(w.sc_status, 0, (size_t)ns * sizeof(int), w.stream));
            const launch::Columns cols{(size_t)ns, 0};
            const size_t half = (size_t)(N_CELLS / 2) * ns * BYTES_PER_CELL;  // rows 0..63 of the chunk's matrix
            launch::blob_to_columns(ns, w.d_in, out_cells ? w.d_cells : nullptr, cols, /*blob_half=*/false, w.sc_status, d_w29_, n_inv4096_, w.stream);
            HIPCK(hipMemcpyAsync(w.h_status, w.sc_status, (size_t)ns * sizeof(int), hipMemcpyDeviceToHost, w.stream));
            if (out_cells) HIPCK(hipMemcpyAsync(w.h_cells + half, w.d_cells + half, half, hipMemcpyDeviceToHost, w.stream));
            HIPCK(hipEventRecord(w.done, w.stream));
            HIPCK(hipGetLastError());
            HIPCK(hipStreamSynchronize(w.stream));
            parallel_for(ns, T, pool, [&](int b) {
                if (h_status) h_status[first + b] = w.h_status[b] ? ERR_SCALAR : OK;
                if (w.h_status[b]) return;  // a refused blob: its slots stay as the caller left them
                for (int c = 0; c < N_CELLS && out_cells; c++) {
                    const uint8_t* from = c < N_CELLS / 2 ? blobs[first + b] + (size_t)c * BYTES_PER_CELL : w.h_cells + ((size_t)c * ns + b) * BYTES_PER_CELL;
                    memcpy(out_cells[c][first + b], from, BYTES_PER_CELL);
                }
                for (int c = 0; c < N_CELLS && out_proofs; c++) memcpy(out_proofs[c][first + b], proofs[first + b][c], 48);
            });
        }
        release_work(w);
        held = nullptr;
    } catch (const std::exception& e) {
        if (held) {
            (void)hipStreamSynchronize(held->stream);
            release_work(*held);
        }
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// ---- the supernode's call ------------------------------------------------------------------------------------------------------
// (the status of an index list: verify_host.hpp, column_list_status -- c_api.cpp asks it too, before it resolves a pointer)
// The decoder's index arrays for the column source: list entry (column rank j, blob i) lands in slot i * 128 + column_indices[j] of
// the evaluations, counts towards blob i's status and is read at cell j * n_total + i of d_cells_r0 = the call's cells + r0 cells
// (k_cells_to_fr's src_of).  ONE presence mask: every blob misses the same columns.  j * n_total + i < 127 * 2^24 + 2^24 <= 2^31 - 1.
int Engine::rs_decode_columns(int nr, size_t n_total, uint64_t n_columns, const uint64_t* column_indices, const uint8_t* d_cells_r0, int* st_out,
                              const RsCommit* commit) {
    std::vector<uint32_t> present(4, 0);
    for (uint64_t j = 0; j < n_columns; j++) {
        const int i = brp7((int)column_indices[j]);  // domain-order index of a cell = its bit-reversed index (cosets.rs:186-195)
        present[i >> 5] |= 1u << (i & 31);
    }
    std::vector<int> slot, stof, src;
    slot.reserve((size_t)nr * n_columns);
    stof.reserve((size_t)nr * n_columns);
    src.reserve((size_t)nr * n_columns);
    for (uint64_t j = 0; j < n_columns; j++)
        for (int i = 0; i < nr; i++) {
            slot.push_back(i * N_CELLS + (int)column_indices[j]);
            stof.push_back(i);
            src.push_back((int)(j * n_total + (size_t)i));
        }
    return rs_decode(nr, d_cells_r0, false, slot, stof, present, st_out, nullptr, &src, /*shared_pattern=*/true, commit);
}

int Engine::recover_data_columns_device(int R, uint64_t n_columns, const uint64_t* column_indices, const uint8_t* d_cells, uint8_t* d_out_cells,
                                        uint8_t* d_out_proofs, int* status, hipStream_t user_stream) {
    return recover_data_columns_checked_device(R, n_columns, column_indices, d_cells, RecoverCheck{}, d_out_cells, d_out_proofs, status, user_stream);
}
int Engine::recover_data_columns_host(int lo, int R, uint64_t n_columns, const uint64_t* column_indices, const uint8_t* const* const* cells,
                                      uint8_t* const* const* out_cells, uint8_t* const* const* out_proofs, int* status) {
    return recover_data_columns_checked_host(lo, R, n_columns, column_indices, cells, RecoverCheck{}, out_cells, out_proofs, status);
}

// The checked forms are the two calls above with three things more, all of them behind the decode they share: the commitment of every
// recovered polynomial from the coefficients the decoder has just left (rs_decode's `commit`: in front of its one synchronisation, so a
// sub-batch still costs one and the status words come down once), the comparison with the caller's bytes, and cells 0..63 once more in
// blob-major order -- the recovered blobs.  An empty RecoverCheck launches what the unchecked calls always launched.
int Engine::recover_data_columns_checked_device(int R, uint64_t n_columns, const uint64_t* column_indices, const uint8_t* d_cells, const RecoverCheck& chk,
                                                uint8_t* d_out_cells, uint8_t* d_out_proofs, int* status, hipStream_t user_stream) {
    if (R <= 0) return OK;
    const int list = column_list_status(n_columns, column_indices);
    for (int r = 0; r < R; r++) status[r] = list;
    if (list != OK) return OK;  // before anything is launched
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        // sub-batches as recover_cells_and_kzg_proofs_device cuts them; here a sub-batch is a range of blobs of EVERY column
        for (int r0 = 0; r0 < R; r0 += device_batch_max_) {
            const int nr = std::min(device_batch_max_, R - r0);
            ensure_workspace(nr);  // also orders stream_ behind the previous asynchronous user of the workspace (the sub-batch before this one)
            HIPCK(hipEventRecord(work_[0].ev_in, user_stream));  // the decode runs on the library's stream, behind what the caller's wrote into d_cells
            HIPCK(hipStreamWaitEvent(stream_, work_[0].ev_in, 0));
            PoolBuf d_calc(*this, chk.commits() ? (size_t)nr * 48 : 0);
            RsCommit commit;
            commit.d_calc = (uint8_t*)d_calc.p;
            commit.d_expected = chk.d_commitments ? chk.d_commitments + (size_t)r0 * 48 : nullptr;
            commit.d_out = chk.d_out_commitments ? chk.d_out_commitments + (size_t)r0 * 48 : nullptr;
            const int rc = rs_decode_columns(nr, (size_t)R, n_columns, column_indices, d_cells + (size_t)r0 * BYTES_PER_CELL, status + r0,
                                             chk.commits() ? &commit : nullptr);
            if (rc) return rc;
            hipStream_t st = user_stream ? user_stream : stream_;
            const launch::Columns cols{(size_t)R, (size_t)r0};
            if (chk.d_out_blobs) launch::coeffs_to_blobs(nr, d_coeffs_, chk.d_out_blobs + (size_t)r0 * BYTES_PER_BLOB, d_w29_, st);
            if (d_out_cells) launch::coeffs_to_cells(nr, d_coeffs_, d_out_cells, d_w29_, st, &cols);
            if (d_out_proofs) run_proofs_from_coeffs(work_[0], nr, d_out_proofs, st, nullptr, PROOFS_ALL, 0, &cols);
            HIPCK(hipEventRecord(work_[0].done, st));
            HIPCK(hipGetLastError());
        }
        if (!user_stream) SYNC_CHECKED(stream_);
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

int Engine::recover_data_columns_checked_host(int lo, int R, uint64_t n_columns, const uint64_t* column_indices, const uint8_t* const* const* cells,
                                              const RecoverCheck& chk, uint8_t* const* const* out_cells, uint8_t* const* const* out_proofs, int* status) {
    if (R <= 0) return OK;
    const int list = column_list_status(n_columns, column_indices);
    for (int r = 0; r < R; r++) status[lo + r] = list;
    if (list != OK) return OK;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        TraceLap lap{knobs_.trace, "recover columns"};
        for (int r0 = 0; r0 < R; r0 += device_batch_max_) {
            const int nr = std::min(device_batch_max_, R - r0), first = lo + r0;
            ensure_workspace(nr);
            // the present columns of these blobs as a [n_columns][nr] matrix, through pinned memory; the expected commitments go up with them
            const size_t in_bytes = (size_t)n_columns * nr * BYTES_PER_CELL, e_bytes = chk.commitments ? (size_t)nr * 48 : 0;
            const size_t k_bytes = chk.commits() ? (size_t)nr * 48 : 0;
            PoolBuf h_in(*this, in_bytes, true), d_in(*this, in_bytes), h_exp(*this, e_bytes, true), d_exp(*this, e_bytes);
            PoolBuf d_calc(*this, k_bytes), h_calc(*this, chk.out_commitments ? k_bytes : 0, true);
            for (uint64_t j = 0; j < n_columns; j++)
                for (int i = 0; i < nr; i++) memcpy((uint8_t*)h_in.p + (j * nr + i) * BYTES_PER_CELL, cells[j][first + i], BYTES_PER_CELL);
            HIPCK(hipMemcpyAsync(d_in.p, h_in.p, in_bytes, hipMemcpyHostToDevice, stream_));
            if (chk.commitments) {
                for (int i = 0; i < nr; i++) memcpy((uint8_t*)h_exp.p + (size_t)i * 48, chk.commitments[first + i], 48);
                HIPCK(hipMemcpyAsync(d_exp.p, h_exp.p, e_bytes, hipMemcpyHostToDevice, stream_));
            }
            RsCommit commit;
            commit.d_calc = (uint8_t*)d_calc.p;
            commit.d_expected = chk.commitments ? (const uint8_t*)d_exp.p : nullptr;
            commit.h_out = chk.out_commitments ? (uint8_t*)h_calc.p : nullptr;
            const int rc = rs_decode_columns(nr, (size_t)nr, n_columns, column_indices, (const uint8_t*)d_in.p, status + first, chk.commits() ? &commit : nullptr);
            if (rc) return rc;
            lap("stage in + RS decode");
            const size_t c_bytes = out_cells ? (size_t)nr * N_CELLS * BYTES_PER_CELL : 0, p_bytes = out_proofs ? (size_t)nr * N_CELLS * 48 : 0;
            const size_t b_bytes = chk.out_blobs ? (size_t)nr * BYTES_PER_BLOB : 0;
            PoolBuf d_c(*this, c_bytes), d_p(*this, p_bytes), h_c(*this, c_bytes, true), h_p(*this, p_bytes, true);
            PoolBuf d_b(*this, b_bytes), h_b(*this, b_bytes, true);
            const launch::Columns cols{(size_t)nr, 0};
            if (chk.out_blobs) {
                launch::coeffs_to_blobs(nr, d_coeffs_, (uint8_t*)d_b.p, d_w29_, stream_);
                HIPCK(hipMemcpyAsync(h_b.p, d_b.p, b_bytes, hipMemcpyDeviceToHost, stream_));
            }
            if (out_cells) {
                launch::coeffs_to_cells(nr, d_coeffs_, (uint8_t*)d_c.p, d_w29_, stream_, &cols);
                HIPCK(hipMemcpyAsync(h_c.p, d_c.p, c_bytes, hipMemcpyDeviceToHost, stream_));
            }
            if (out_proofs) {
                run_proofs_from_coeffs(work_[0], nr, (uint8_t*)d_p.p, stream_, nullptr, PROOFS_ALL, 0, &cols);
                HIPCK(hipMemcpyAsync(h_p.p, d_p.p, p_bytes, hipMemcpyDeviceToHost, stream_));
            }
            SYNC_CHECKED(stream_);
            lap("cells + proofs + D2H");
            for (int i = 0; i < nr; i++) {
                if (status[first + i] != OK) continue;  // a refused blob: its slots stay as the caller left them
                if (chk.out_commitments) memcpy(chk.out_commitments[first + i], (const uint8_t*)h_calc.p + (size_t)i * 48, 48);
                if (chk.out_blobs) memcpy(chk.out_blobs[first + i], (const uint8_t*)h_b.p + (size_t)i * BYTES_PER_BLOB, BYTES_PER_BLOB);
            }
            for (int c = 0; c < N_CELLS && (out_cells || out_proofs); c++)
                for (int i = 0; i < nr; i++) {
                    if (status[first + i] != OK) continue;
                    if (out_cells) memcpy(out_cells[c][first + i], (const uint8_t*)h_c.p + ((size_t)c * nr + i) * BYTES_PER_CELL, BYTES_PER_CELL);
                    if (out_proofs) memcpy(out_proofs[c][first + i], (const uint8_t*)h_p.p + ((size_t)c * nr + i) * 48, 48);
                }
            lap("scatter to caller buffers");
        }
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

}  // namespace kzg
