// Stage-level test hooks of the engine (include/c_eth_kzg_test_hooks.h): single stages against the oracle.
#include "engine_internal.hpp"
#include "curve29.hpp"
#include "vm_search.hpp"
#include <chrono>

#include <array>

namespace kzg {

// ---------------------------------------------------------------------------------------------
// stage-level test hooks
int Engine::test_fr_ntt4096(const uint8_t* in_be, uint8_t* out_be, int inverse_dit) {
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        uint8_t *di, *dout;
        HIPCK(hipMalloc(&di, BYTES_PER_BLOB));
        HIPCK(hipMalloc(&dout, BYTES_PER_BLOB));
        HIPCK(hipMemcpy(di, in_be, BYTES_PER_BLOB, hipMemcpyHostToDevice));
        launch::test_ntt4096(di, dout, d_w29_, n_inv4096_, inverse_dit, stream_);
        HIPCK(hipStreamSynchronize(stream_));
        HIPCK(hipMemcpy(out_be, dout, BYTES_PER_BLOB, hipMemcpyDeviceToHost));
        HIPCK(hipFree(di));
        HIPCK(hipFree(dout));
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

int Engine::test_sha256_many(int n, const uint8_t* prefix, uint32_t prefix_len, const uint8_t* d_body, size_t body_stride, uint32_t body_len,
                             const uint8_t* d_tail, size_t tail_stride, uint32_t tail_len, uint8_t* d_out) {
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        PoolBuf d_prefix(*this, prefix_len);
        if (prefix_len) HIPCK(hipMemcpyAsync(d_prefix.p, prefix, prefix_len, hipMemcpyHostToDevice, stream_));
        launch::sha256_many(n, (const uint8_t*)d_prefix.p, prefix_len, d_body, body_stride, body_len, d_tail, tail_stride, tail_len, d_out, stream_);
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(stream_));
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// in/out: [lane][128][48 B]; both directions natural in -> natural out (inverse is unscaled)
int Engine::test_g1_fft128(const uint8_t* in, uint8_t* out, int n_lanes, int inverse) {
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        int stride = ((n_lanes + 63) / 64) * 64;
        size_t bytes = (size_t)n_lanes * 128 * 48;
        uint8_t *di, *dout;
        void* X;
        HIPCK(hipMalloc(&di, bytes));
        HIPCK(hipMalloc(&dout, bytes));
        size_t nx = (size_t)128 * stride;
        const size_t PS = launch::SIZEOF_JACQ;
        HIPCK(hipMalloc(&X, nx * PS));
        HIPCK(hipMemcpy(di, in, bytes, hipMemcpyHostToDevice));
        launch::g1_set_inf(X, nx, stream_, launch::FMT_JACQ);
        launch::test_load_points(di, X, n_lanes, stride, stream_);
        HIPCK(hipStreamSynchronize(stream_));
        std::vector<uint8_t> hx(nx * PS), hy(nx * PS);
        auto brp = [](int v) { int r = 0; for (int i = 0; i < 7; i++) r |= ((v >> i) & 1) << (6 - i); return r; };
        auto permute = [&]() {
            HIPCK(hipMemcpy(hx.data(), X, nx * PS, hipMemcpyDeviceToHost));
            for (int p = 0; p < 128; p++) memcpy(&hy[(size_t)brp(p) * stride * PS], &hx[(size_t)p * stride * PS], stride * PS);
            HIPCK(hipMemcpy(X, hy.data(), nx * PS, hipMemcpyHostToDevice));
        };
        if (inverse) permute();  // DIT wants bit-reversed input
        g1_fft128_full(X, stride, inverse, stream_);
        HIPCK(hipStreamSynchronize(stream_));
        if (!inverse) permute();  // DIF leaves bit-reversed output
        launch::g1_compress(X, dout, 128, stride, n_lanes, stream_, launch::FMT_JACQ);
        HIPCK(hipStreamSynchronize(stream_));
        HIPCK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
        HIPCK(hipFree(di)); HIPCK(hipFree(dout)); HIPCK(hipFree(X));
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// scalars: [n_msm][128 groups][64] BE -> out [n_msm][128][48]: the 128 fixed-base MSMs of stage D
int Engine::test_fixed_msm(const uint8_t* scalars_be, int n_msm, uint8_t* out) {
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        size_t ns = (size_t)n_msm * 128 * 64;
        int stride = ((n_msm + 63) / 64) * 64;
        uint8_t *di, *dout;
        void *sc, *X;
        HIPCK(hipMalloc(&di, ns * 32));
        HIPCK(hipMalloc(&sc, ns * sizeof(Fr)));
        HIPCK(hipMalloc(&X, (size_t)128 * stride * launch::SIZEOF_JACQ));
        HIPCK(hipMalloc(&dout, (size_t)n_msm * 128 * 48));
        HIPCK(hipMemcpy(di, scalars_be, ns * 32, hipMemcpyHostToDevice));
        launch::test_scalars_be(di, sc, ns, stream_);
        launch::g1_set_inf(X, (size_t)128 * stride, stream_, launch::FMT_JACQ);
        launch_msm(sc, TAB_FK, X, 128, n_msm, stride, 0, stream_, launch::FMT_JACQ);
        launch::g1_compress(X, dout, 128, stride, n_msm, stream_, launch::FMT_JACQ);
        HIPCK(hipStreamSynchronize(stream_));
        HIPCK(hipMemcpy(out, dout, (size_t)n_msm * 128 * 48, hipMemcpyDeviceToHost));
        HIPCK(hipFree(di)); HIPCK(hipFree(sc)); HIPCK(hipFree(X)); HIPCK(hipFree(dout));
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// One stated schedule of the fixed-base MSM.  table_kind: TAB_FK (128 groups) or TAB_SRS (64 groups: the group sums of a commitment, before its
// fold).  mode: -1 = what launch_msm_range picks for n_slices (its two-launch overflow form included), else the mode handed to launch::msm_glv
// (0 flat, 1 a lane per window, 3 two lanes per window, 2 four chunks).  scalar_form 0: canonical big-endian scalars, split by
// launch::glv_split; 1: the balanced halves themselves, 8 little-endian words per scalar (|k1|, |k2|, the sign in bit 127 of a half) as the
// prover's Fr kernels leave them -- launch_msm's scalars_split overload, which the prover calls.  scalars [n_slices][groups][64] ->
// out [n_slices][groups][48]; modes5[0] = launches made, modes5[1 ..] their modes.  The complete table only (a wider one still being built is
// left alone: one table per call).
int Engine::test_fixed_msm_ex(int table_kind, int mode, int scalar_form, const uint8_t* scalars, int n_slices, uint8_t* out, int32_t* modes5) {
    if ((table_kind != TAB_FK && table_kind != TAB_SRS) || mode < -1 || mode > 3 || (scalar_form != 0 && scalar_form != 1) || n_slices < 1 || n_slices > 4096)
        return ERR_INPUT;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    struct DevBuf {  // (freed on every way out)
        void* p = nullptr;
        ~DevBuf() { if (p) (void)hipFree(p); }
    } d_in, d_sc, d_X, d_out;
    try {
        HIPCK(hipSetDevice(dev_));
        TableView tv = table_view((TableSel)table_kind);
        if (!tv.main) return ERR_INPUT;
        tv.next.reset();
        const int n_groups = tv.main->n_groups, stride = ((n_slices + 63) / 64) * 64;
        const size_t ns = (size_t)n_slices * n_groups * 64;
        HIPCK(hipMalloc(&d_sc.p, ns * sizeof(Fr)));
        HIPCK(hipMalloc(&d_X.p, (size_t)n_groups * stride * launch::SIZEOF_JACQ));
        HIPCK(hipMalloc(&d_out.p, (size_t)n_slices * n_groups * 48));
        if (scalar_form == 0) {
            HIPCK(hipMalloc(&d_in.p, ns * 32));
            HIPCK(hipMemcpy(d_in.p, scalars, ns * 32, hipMemcpyHostToDevice));
            launch::test_scalars_be((const uint8_t*)d_in.p, d_sc.p, ns, stream_);
        } else {
            static_assert(sizeof(Fr) == 32, "a split scalar takes the place of the scalar");
            HIPCK(hipMemcpy(d_sc.p, scalars, ns * sizeof(Fr), hipMemcpyHostToDevice));
        }
        MsmTap tap;
        tap.force = mode;
        launch::g1_set_inf(d_X.p, (size_t)n_groups * stride, stream_, launch::FMT_JACQ);
        launch_msm(d_sc.p, tv, scalar_form == 1, d_X.p, n_groups, n_slices, stride, 0, stream_, launch::FMT_JACQ, &tap);
        launch::g1_compress(d_X.p, (uint8_t*)d_out.p, n_groups, stride, n_slices, stream_, launch::FMT_JACQ);
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(stream_));
        HIPCK(hipMemcpy(out, d_out.p, (size_t)n_slices * n_groups * 48, hipMemcpyDeviceToHost));
        modes5[0] = tap.n;
        for (int i = 0; i < 4; i++) modes5[1 + i] = i < tap.n ? tap.modes[i] : -1;
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// The prover's own schedule (enqueue_compute, both outputs asked for) on n blobs, then the MSM scalars it left in the work set, word for
// word: which kernels wrote them is the context's ETH_KZG_AMD_FUSED_SCALARS; *fused_launches = launches of k_coeffs_to_cells_scalars.
int Engine::test_prover_scalars(int n, const uint8_t* blobs, uint32_t* scalars, uint64_t max_words, uint64_t* n_words, uint8_t* cells,
                                uint8_t* proofs, int32_t* status, int32_t* fused_launches) {
    if (n < 1 || n > 4096) return ERR_INPUT;
    const uint64_t words = (uint64_t)fk20_segs(n) * n * N_EXT * 8;
    if (words > max_words) return ERR_INPUT;
    struct DevBuf {  // (freed on every way out)
        void* p = nullptr;
        ~DevBuf() { if (p) (void)hipFree(p); }
    } d_in, d_cells, d_proofs;
    Work* held = nullptr;
    try {
        HIPCK(hipSetDevice(dev_));
        Work& w = lease_work(1, NW - 1);
        held = &w;
        HIPCK(hipMalloc(&d_in.p, (size_t)n * BYTES_PER_BLOB));
        HIPCK(hipMalloc(&d_cells.p, (size_t)n * N_CELLS * BYTES_PER_CELL));
        HIPCK(hipMalloc(&d_proofs.p, (size_t)n * N_CELLS * 48));
        HIPCK(hipMemcpyAsync(d_in.p, blobs, (size_t)n * BYTES_PER_BLOB, hipMemcpyHostToDevice, w.stream));
        const uint64_t before = fused_launches_.load();
        enqueue_compute(w, n, (const uint8_t*)d_in.p, (uint8_t*)d_cells.p, (uint8_t*)d_proofs.p, w.stream, nullptr);
        HIPCK(hipEventRecord(w.done, w.stream));
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(w.stream));
        *fused_launches = (int32_t)(fused_launches_.load() - before);
        *n_words = words;
        HIPCK(hipMemcpy(scalars, w.scalars, words * 4, hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(cells, d_cells.p, (size_t)n * N_CELLS * BYTES_PER_CELL, hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(proofs, d_proofs.p, (size_t)n * N_CELLS * 48, hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(status, w.status, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        release_work(w);
        held = nullptr;
    } catch (const std::exception& e) {
        if (held) { (void)hipStreamSynchronize(held->stream); (void)hipStreamSynchronize(held->copy); release_work(*held); }
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// The G1 stage of the prover on sums of the caller's: the words go where the MSM would have left them (stride bp, the identity in the
// padding lanes, as g1_set_inf leaves them in front of the MSM), then run_g1_stage -- the launches run_proofs_from_coeffs makes.
// sums_words: [128][lanes][39], lanes = n in linear-map mode, fk20_segs(n) * n (lane seg * n + b) in the circulant mode.
int Engine::test_proofs_from_sums(int program, int n, const int32_t* sums_words, uint8_t* out_proofs) {
    if (n < 1 || n > 256 || program < -1 || program >= SLP_COUNT) return ERR_INPUT;
    if (program >= 0 && n <= circ_max_) return ERR_INPUT;  // the circulant form runs no program
    struct DevBuf {  // (freed on every way out)
        void* p = nullptr;
        ~DevBuf() { if (p) (void)hipFree(p); }
    } d_proofs;
    Work* held = nullptr;
    try {
        HIPCK(hipSetDevice(dev_));
        Work& w = lease_work(1, NW - 1);
        held = &w;
        hipStream_t st = w.stream;
        ensure_workspace(w, n);
        HIPCK(hipStreamWaitEvent(st, w.done, 0));
        HIPCK(hipMalloc(&d_proofs.p, (size_t)n * N_CELLS * 48));
        const G1Stage g = prepare_g1_stage(w, n, st, program);
        constexpr size_t pt = launch::SIZEOF_JACS;
        static_assert(pt == 39 * sizeof(int32_t), "the hook's callers give 39 words per point");
        const size_t lanes = (size_t)(g.linmap_mode ? 1 : g.segs) * n;
        if (lanes > (size_t)g.bp) throw std::logic_error("test_proofs_from_sums: more lanes than the stride holds");
        launch::g1_set_inf(g.X, (size_t)128 * g.bp, st, launch::FMT_JACS);
        HIPCK(hipMemcpy2DAsync(g.X, (size_t)g.bp * pt, sums_words, lanes * pt, lanes * pt, 128, hipMemcpyHostToDevice, st));
        run_g1_stage(w, g, n, (uint8_t*)d_proofs.p, st);
        HIPCK(hipEventRecord(w.done, st));
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(st));
        HIPCK(hipMemcpy(out_proofs, d_proofs.p, (size_t)n * N_CELLS * 48, hipMemcpyDeviceToHost));
        release_work(w);
        held = nullptr;
    } catch (const std::exception& e) {
        if (held) { (void)hipStreamSynchronize(held->stream); (void)hipStreamSynchronize(held->copy); release_work(*held); }
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

static void fr_mont_to_be(uint8_t* out, const uint32_t* mont);
// What the engine uploaded for compilation `program` of the linear map: the words as the device holds them, the launches as (kind,
// first, count), the arena's slot count, the constants (canonical big-endian) the recoded digits were made from.
int Engine::test_linmap_program(int program, uint32_t* words, uint64_t max_words, uint64_t* n_words, int32_t* launches3, uint64_t max_launches,
                                uint64_t* n_launches, int32_t* n_slots, uint8_t* consts_be, uint64_t max_consts, uint64_t* n_consts) {
    if (program < 0 || program >= SLP_COUNT) return ERR_INPUT;
    try {
        HIPCK(hipSetDevice(dev_));
        const SlpProgram& P = slp_program(program);
        *n_words = P.n_words;
        *n_launches = P.launches.size();
        *n_consts = P.consts.size();
        *n_slots = P.n_slots;
        if (P.n_words > max_words || P.launches.size() > max_launches || P.consts.size() > max_consts) return ERR_INPUT;
        HIPCK(hipMemcpy(words, P.d_words, P.n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < P.launches.size(); i++) {
            launches3[3 * i] = P.launches[i].kind;
            launches3[3 * i + 1] = P.launches[i].first;
            launches3[3 * i + 2] = P.launches[i].count;
        }
        for (size_t i = 0; i < P.consts.size(); i++) fr_mont_to_be(consts_be + 32 * i, P.consts[i].v);
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

int Engine::test_g1_decompress(const uint8_t* in, int n, int subgroup_check, int* h_status, uint8_t* out) {
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        uint8_t *di, *dout;
        void* pts;
        int* st;
        HIPCK(hipMalloc(&di, (size_t)n * 48)); HIPCK(hipMalloc(&dout, (size_t)n * 48));
        HIPCK(hipMalloc(&pts, (size_t)n * sizeof(G1Affine))); HIPCK(hipMalloc(&st, n * sizeof(int)));
        HIPCK(hipMemcpy(di, in, (size_t)n * 48, hipMemcpyHostToDevice));
        launch::g1_decompress(di, pts, st, n, subgroup_check, beta_, stream_);
        launch::test_recompress(pts, dout, n, stream_);
        HIPCK(hipStreamSynchronize(stream_));
        HIPCK(hipMemcpy(h_status, st, n * sizeof(int), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(out, dout, (size_t)n * 48, hipMemcpyDeviceToHost));
        HIPCK(hipFree(di)); HIPCK(hipFree(dout)); HIPCK(hipFree(pts)); HIPCK(hipFree(st));
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// The decoded coordinates themselves, through each of the product's decode / subgroup launch calls (test_g1_decompress re-compresses
// on the device with the decoder's own sign predicate, which hides an error that is wrong both ways).  Two segments [n0 | n1] as a
// verification passes its proofs and commitments; the status words start at the arena's 0xff poison.  Which kernel a form runs is
// the launcher's rule, with N = n0 + n1 and M = launch::coop_points_max():
//   0  g1_decompress, check 0      k_g1_decompress (one lane per point) at every N: no subgroup test
//   1  g1_decompress, check 1      k_g1_decompress_coop for N <= M, k_g1_decompress above (one segment: n1 must be 0)
//   2  g1_decompress2              k_g1_decompress_coop for N <= M, k_g1_decompress above
//   3  g1_decode2 + g1_subgroup2   k_g1_decompress (check 0), then k_g1_subgroup_coop for N <= M, k_g1_subgroup above
//   4  g1_decode2 + pip_shift_prepare_and_subgroup over all N points: the quad branch (k_pip_shift_subgroup_coop) for 2 N <= M, the
//      one-lane branch (k_pip_shift_subgroup) above
// out_xy: what the point array holds behind the launches, x | y canonical big-endian; the identity (0, 0) is 96 zero bytes.  The
// decoders write the identity over a point they refuse; the subgroup-only kernels of forms 3 and 4 read the points and write the status
// word alone, so there a point refused with 2 keeps its decoded coordinates.
int Engine::test_g1_decode(int form, const uint8_t* in, int n0, int n1, int32_t* h_status, uint8_t* out_xy) {
    if (form < 0 || form > 4 || n0 < 1 || n1 < 0 || (form <= 1 && n1 != 0) || (long)n0 + n1 > (1 << 20)) return ERR_INPUT;
    const int n = n0 + n1;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    struct DevBuf {  // (freed on every way out)
        void* p = nullptr;
        ~DevBuf() { if (p) (void)hipFree(p); }
    } d_in, d_pts, d_st, d_ws;
    try {
        HIPCK(hipSetDevice(dev_));
        HIPCK(hipMalloc(&d_in.p, (size_t)n * 48));
        HIPCK(hipMalloc(&d_pts.p, (size_t)n * sizeof(G1Affine)));
        HIPCK(hipMalloc(&d_st.p, (size_t)n * sizeof(int)));
        if (form == 4) HIPCK(hipMalloc(&d_ws.p, launch::pip_shift_workspace_bytes(n)));
        hipStream_t st = stream_;
        HIPCK(hipMemcpyAsync(d_in.p, in, (size_t)n * 48, hipMemcpyHostToDevice, st));
        HIPCK(hipMemsetAsync(d_st.p, 0xff, (size_t)n * sizeof(int), st));
        HIPCK(hipMemsetAsync(d_pts.p, 0xff, (size_t)n * sizeof(G1Affine), st));
        const uint8_t* in0 = (const uint8_t*)d_in.p;
        G1Affine* p0 = (G1Affine*)d_pts.p;
        int* st0 = (int*)d_st.p;
        if (form <= 1) launch::g1_decompress(in0, p0, st0, n, form, beta_, st);
        else if (form == 2) launch::g1_decompress2(in0, p0, st0, n0, in0 + (size_t)n0 * 48, p0 + n0, st0 + n0, n1, beta_, st);
        else {
            launch::g1_decode2(in0, p0, st0, n0, in0 + (size_t)n0 * 48, p0 + n0, st0 + n0, n1, beta_, st);
            if (form == 3) launch::g1_subgroup2(p0, st0, n0, p0 + n0, st0 + n0, n1, beta_, st);
            else launch::pip_shift_prepare_and_subgroup(p0, n, n, d_ws.p, p0, st0, n0, p0 + n0, st0 + n0, n1, beta_, st);
        }
        HIPCK(hipGetLastError());
        std::vector<G1Affine> pts(n);
        HIPCK(hipMemcpyAsync(h_status, d_st.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(pts.data(), d_pts.p, (size_t)n * sizeof(G1Affine), hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        for (int i = 0; i < n; i++) {
            for (int c = 0; c < 2; c++) {
                const Fp& m = c ? pts[i].y : pts[i].x;
                uint8_t* o = out_xy + (size_t)i * 96 + 48 * c;
                if (geq_mod<FpParams>(m.v)) {  // not a reduced coordinate (the 0xff the array started at): nothing was written
                    memset(o, 0xff, 48);
                    continue;
                }
                const Fp v = from_mont(m);
                for (int k = 0; k < 12; k++) {
                    const uint32_t w = v.v[11 - k];
                    o[4 * k] = (uint8_t)(w >> 24); o[4 * k + 1] = (uint8_t)(w >> 16); o[4 * k + 2] = (uint8_t)(w >> 8); o[4 * k + 3] = (uint8_t)w;
                }
            }
        }
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

int Engine::test_field_mul(const uint8_t* a, const uint8_t* b, uint8_t* out, int n, int is_fp) {
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        size_t nb = (size_t)n * (is_fp ? 48 : 32);
        uint8_t *da, *db, *dout;
        HIPCK(hipMalloc(&da, nb)); HIPCK(hipMalloc(&db, nb)); HIPCK(hipMalloc(&dout, nb));
        HIPCK(hipMemcpy(da, a, nb, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(db, b, nb, hipMemcpyHostToDevice));
        launch::test_field_mul(da, db, dout, n, is_fp, stream_);
        HIPCK(hipStreamSynchronize(stream_));
        HIPCK(hipMemcpy(out, dout, nb, hipMemcpyDeviceToHost));
        HIPCK(hipFree(da)); HIPCK(hipFree(db)); HIPCK(hipFree(dout));
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// one operation of k_test_ops.hip per element: n elements of the op's input words in, n of its output words out
int Engine::test_op(int op, int n, const int32_t* in, int32_t* out) {
    int in_w, out_w, dev_only;
    const char* name;
    if (launch::test_op_info(op, &in_w, &out_w, &dev_only, &name) != 0 || n <= 0) return ERR_INPUT;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        const size_t ni = (size_t)n * in_w * sizeof(int32_t), no = (size_t)n * out_w * sizeof(int32_t);
        int32_t *di, *dout;
        HIPCK(hipMalloc(&di, ni)); HIPCK(hipMalloc(&dout, no));
        HIPCK(hipMemcpy(di, in, ni, hipMemcpyHostToDevice));
        HIPCK(hipMemset(dout, 0, no));
        launch::test_op_device(op, n, di, dout, stream_);
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(stream_));
        HIPCK(hipMemcpy(out, dout, no, hipMemcpyDeviceToHost));
        HIPCK(hipFree(di)); HIPCK(hipFree(dout));
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// The two-job bucket MSM of a verification on its own (k_verify.hip; verify.hip: verify_cells_partial runs it behind the challenge).
// points: n_pts compressed; job 0 = sum_{i < n0} sc0[i] P_i, job 1 = sum_{i < n1} sc1[i] P_i over the same array; out96: both sums, compressed.
// form 0: msm_pippenger2.  form 1: pip_shift_prepare + msm_pippenger2_shifted.  form 2: the decode without the subgroup tests, then
// pip_shift_prepare_and_subgroup (statuses of the first n0 points | of the rest) + msm_pippenger2_shifted, as a verification launches them.
// The shifted forms leave two Jacobian sums that the host normalises, as verify.hip does.  h_status: the n_pts status words.
int Engine::test_verify_msm(int form, const uint8_t* points, int n_pts, const uint8_t* sc0_be, int n0, const uint8_t* sc1_be, int n1,
                            uint8_t* out96, int32_t* h_status) {
    if (form < 0 || form > 2 || n0 < 1 || n1 < n0 || n_pts < n1 || n_pts > (1 << 20)) return ERR_INPUT;
    std::vector<Fr> sc((size_t)n0 + n1);
    for (int j = 0; j < n0 + n1; j++) {  // canonical big-endian -> canonical words
        const uint8_t* b = j < n0 ? sc0_be + (size_t)j * 32 : sc1_be + (size_t)(j - n0) * 32;
        Fr& x = sc[j];
        for (int i = 0; i < 8; i++)
            x.v[7 - i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
        if (geq_mod<FrParams>(x.v)) return ERR_SCALAR;
    }
    std::lock_guard<std::recursive_mutex> lk(mu_);
    struct DevBuf {  // (freed on every way out)
        void* p = nullptr;
        ~DevBuf() { if (p) (void)hipFree(p); }
    } d_in, d_pts, d_st, d_sc, d_ws, d_out;
    try {
        HIPCK(hipSetDevice(dev_));
        const bool shifted = form != 0;
        HIPCK(hipMalloc(&d_in.p, (size_t)n_pts * 48));
        HIPCK(hipMalloc(&d_pts.p, (size_t)n_pts * sizeof(G1Affine)));
        HIPCK(hipMalloc(&d_st.p, (size_t)n_pts * sizeof(int)));
        HIPCK(hipMalloc(&d_sc.p, sc.size() * sizeof(Fr)));
        HIPCK(hipMalloc(&d_ws.p, shifted ? launch::pip_shift_workspace_bytes(n_pts) : launch::pip_workspace_bytes(n_pts)));
        HIPCK(hipMalloc(&d_out.p, 512));  // two affine points, or two Jacobian sums (shifted form)
        hipStream_t st = stream_;
        HIPCK(hipMemcpyAsync(d_in.p, points, (size_t)n_pts * 48, hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(d_sc.p, sc.data(), sc.size() * sizeof(Fr), hipMemcpyHostToDevice, st));
        HIPCK(hipMemsetAsync(d_st.p, 0xff, (size_t)n_pts * sizeof(int), st));  // poisoned like a verification's arena: stale contents fail closed
        HIPCK(hipMemsetAsync(d_out.p, 0xff, 512, st));
        const uint8_t* in0 = (const uint8_t*)d_in.p;
        G1Affine* p0 = (G1Affine*)d_pts.p;
        int* st0 = (int*)d_st.p;
        const int rest = n_pts - n0;
        const Fr *s0 = (const Fr*)d_sc.p, *s1 = s0 + n0;
        G1Affine out[2];
        if (form == 2) {
            launch::g1_decode2(in0, p0, st0, n0, in0 + (size_t)n0 * 48, p0 + n0, st0 + n0, rest, beta_, st);
            launch::pip_shift_prepare_and_subgroup(p0, n_pts, n_pts, d_ws.p, p0, st0, n0, p0 + n0, st0 + n0, rest, beta_, st);
        } else {
            launch::g1_decompress2(in0, p0, st0, n0, in0 + (size_t)n0 * 48, p0 + n0, st0 + n0, rest, beta_, st);
            if (form == 1) launch::pip_shift_prepare(p0, n_pts, n_pts, d_ws.p, beta_, st);
        }
        std::vector<int32_t> status(n_pts);
        HIPCK(hipMemcpyAsync(status.data(), d_st.p, (size_t)n_pts * sizeof(int), hipMemcpyDeviceToHost, st));
        if (shifted) {
            launch::msm_pippenger2_shifted(s0, n0, s1, n1, n_pts, d_ws.p, d_out.p, st);
            JacQ sums[2];
            static_assert(sizeof(sums) <= 512 && sizeof(JacQ) == launch::SIZEOF_JACQ, "result slot");
            HIPCK(hipMemcpyAsync(sums, d_out.p, sizeof sums, hipMemcpyDeviceToHost, st));
            HIPCK(hipGetLastError());
            HIPCK(hipStreamSynchronize(st));
            for (int i = 0; i < 2; i++) {
                if (sums[i].x.v[0] == 0xffffffffu && sums[i].z.v[0] == 0xffffffffu) throw std::runtime_error("verification MSM left no result");
                out[i] = to_affine(jac_from_jacq(sums[i]));
            }
        } else {
            launch::msm_pippenger2(p0, s0, n0, s1, n1, d_ws.p, d_out.p, beta_, st);
            HIPCK(hipMemcpyAsync(out, d_out.p, 2 * sizeof(G1Affine), hipMemcpyDeviceToHost, st));
            HIPCK(hipGetLastError());
            HIPCK(hipStreamSynchronize(st));
        }
        for (int i = 0; i < 2; i++)  // the poison pattern (or anything else that is not a reduced coordinate) is a device failure
            if (out[i].x.v[11] > FpParams::MOD[11] || out[i].y.v[11] > FpParams::MOD[11]) throw std::runtime_error("verification MSM left no result");
        if (h_status) memcpy(h_status, status.data(), (size_t)n_pts * sizeof(int32_t));
        for (int i = 0; i < 2; i++) g1_compress(out96 + 48 * i, out[i]);
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// What the batch verifiers hand to their pairing checks, as bytes.  The device-resident cell verifier: the product's own set-up
// (verify.hip: verify_cells_partial_device) with a range; an empty range gives two identities, as the host form's partial call.
int Engine::test_verify_cells_partial_device(uint64_t n, const uint8_t* d_commitments, const uint64_t* d_cell_indices, const uint8_t* d_cells,
                                             const uint8_t* d_proofs, uint64_t lo, uint64_t hi, uint8_t* out96) {
    if (n < 1 || n > MAX_CELLS_PER_VERIFICATION || lo > hi || hi > n) return ERR_INPUT;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    G1Affine pts[2];
    bool empty = false;
    const int rc = verify_cells_partial_device(n, d_commitments, d_cell_indices, d_cells, d_proofs, lo, hi, pts, &empty, nullptr);
    if (rc) return rc;
    g1_compress(out96, pts[0]);
    g1_compress(out96 + 48, pts[1]);
    return OK;
}
// The leaf-hashed challenge (verify.hip).  The leaf digests: the flagged verification's own pass over flat host arrays, with the tap
// that hands the digests out and ends the call behind them.
int Engine::test_cell_leaf_digests(uint64_t n, const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs,
                                   uint8_t* out_digests) {
    if (n < 1 || n > MAX_CELLS_PER_VERIFICATION) return ERR_INPUT;
    std::vector<const uint8_t*> cp, lp, pp;
    try {
        cp.resize(n); lp.resize(n); pp.resize(n);
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    for (uint64_t k = 0; k < n; k++) {
        cp[k] = commitments + k * 48;
        lp[k] = cells + k * (size_t)BYTES_PER_CELL;
        pp[k] = proofs + k * 48;
    }
    CellChallengeMode mode;
    mode.leaf = true;
    mode.leaves_out = out_digests;
    G1Affine pts[2];
    bool empty = false;
    return verify_cells_partial(n, cp.data(), n, cell_indices, n, lp.data(), n, pp.data(), 0, n, pts, &empty, nullptr, nullptr, &mode);
}
// The whole batch's challenge digest and pairing inputs under either transcript, host or device-resident form.
int Engine::test_verify_cells_inputs_ex(uint64_t n, int on_device, const void* commitments, const void* cell_indices, const void* cells,
                                        const void* proofs, uint32_t flags, uint8_t* root32, uint8_t* out96) {
    if (n < 1 || n > MAX_CELLS_PER_VERIFICATION) return ERR_INPUT;
    CellChallengeMode mode;
    mode.leaf = flags != 0;
    mode.digest_out = root32;
    G1Affine pts[2];
    bool empty = false;
    int rc;
    if (on_device) {
        std::lock_guard<std::recursive_mutex> lk(mu_);
        rc = verify_cells_partial_device(n, (const uint8_t*)commitments, (const uint64_t*)cell_indices, (const uint8_t*)cells, (const uint8_t*)proofs, 0, n,
                                         pts, &empty, nullptr, &mode);
    } else {
        rc = verify_cells_partial(n, (const uint8_t* const*)commitments, n, (const uint64_t*)cell_indices, n, (const uint8_t* const*)cells, n,
                                  (const uint8_t* const*)proofs, 0, n, pts, &empty, nullptr, nullptr, &mode);
    }
    if (rc) return rc;
    g1_compress(out96, pts[0]);
    g1_compress(out96 + 48, pts[1]);
    return OK;
}
// The blob batch verifier, host or device-resident form: the product's call with the out-pointer of pairing_check_4844 set.
int Engine::test_verify_blob_batch_inputs(uint64_t n, int on_device, const void* blobs, const void* commitments, const void* proofs,
                                          uint8_t* out96, int* verified) {
    if (n < 1 || n > (1u << 24)) return ERR_INPUT;  // (an empty batch verifies without a pairing check: there are no sums)
    G1Affine sums[2] = {aff_inf(), aff_inf()};
    const int rc = on_device ? verify_blob_kzg_proof_batch_device(n, (const uint8_t*)blobs, (const uint8_t*)commitments, (const uint8_t*)proofs, verified,
                                                                  nullptr, sums)
                             : verify_blob_kzg_proof_batch_host(n, (const uint8_t* const*)blobs, n, (const uint8_t* const*)commitments, n,
                                                                (const uint8_t* const*)proofs, verified, sums);
    if (rc) return rc;
    g1_compress(out96, sums[0]);
    g1_compress(out96 + 48, sums[1]);
    return OK;
}

// One pass of the many-verification with its tap set (verify_many.hip): the launches are the public call's, the tap copies the pinned
// read-backs after the pass's own syncs, and the points are compressed here, on the host.  The caller (c_api_hooks.cpp) has refused
// null buffers; a call the engine would cut into parts or chunks is refused before anything is launched.
// Over any source and with either challenge (the hooks' makers: c_api_hooks.cpp); digests32 and leaves32 may be null.
int Engine::test_verify_many_sums_in(uint64_t n_batches, const VerifyManyInput& in, int32_t* verified, int32_t* status, int32_t* form4, uint8_t* sums96,
                                     uint32_t* rho, uint8_t* fold96, int32_t* probe_ranges, uint8_t* probe_sums96, uint64_t max_probes, uint64_t* n_probes,
                                     uint8_t* digests32, uint8_t* leaves32, uint64_t* counts2) {
    if (counts2) counts2[0] = counts2[1] = 0;
    if (n_batches < 1 || n_batches > (1u << 20)) return ERR_INPUT;
    uint64_t total_cells = 0;
    for (uint64_t b = 0; b < n_batches; b++) {
        if (in.cells_of(b) > (uint64_t)VM_CHUNK_CELLS) return ERR_INPUT;
        total_cells += in.cells_of(b);
    }
    if (total_cells > (uint64_t)VM_CHUNK_CELLS) return ERR_INPUT;                                                        // chunks
    if (n_batches >= (uint64_t)VM_SPLIT_MIN_PROBLEMS && total_cells >= (uint64_t)VM_SPLIT_MIN_CELLS) return ERR_INPUT;  // parts
    const int B = (int)n_batches;
    std::vector<int> ver(B), st(B);
    VerifyManyTap tap;
    const int rc = verify_cell_kzg_proof_batch_many(n_batches, in, ver.data(), st.data(), &tap);
    if (rc) return rc;
    if (tap.passes > 1) return ERR_INPUT;  // (cannot happen behind the checks above)
    test_search_stats_[0] = (uint64_t)tap.device_probes;
    test_search_stats_[1] = tap.probes.size() / 3;
    static_assert(sizeof(JacQ) == launch::SIZEOF_JACQ, "the tap holds JacQ words");
    auto compress2 = [](uint8_t* out96, const uint8_t* two) {  // a slot that still holds its poison comes out as 0xff bytes
        for (int j = 0; j < 2; j++) {
            JacQ s;
            memcpy(&s, two + (size_t)j * sizeof(JacQ), sizeof(JacQ));
            if (s.x.v[0] == 0xffffffffu && s.z.v[0] == 0xffffffffu) memset(out96 + 48 * j, 0xff, 48);
            else g1_compress(out96 + 48 * j, to_affine(jac_from_jacq(s)));
        }
    };
    for (int b = 0; b < B; b++) {
        verified[b] = st[b] == OK && ver[b] != 0;
        status[b] = st[b];
        memset(sums96 + 96 * (size_t)b, 0, 96);
        rho[4 * b] = rho[4 * b + 1] = rho[4 * b + 2] = rho[4 * b + 3] = 0;
    }
    form4[0] = tap.small; form4[1] = tap.folded; form4[2] = tap.searched; form4[3] = tap.fold_verdict;
    memset(fold96, 0, 96);
    *n_probes = tap.probes.size() / 3;
    if (digests32) memset(digests32, 0, (size_t)B * 32);
    if (leaves32 && in.leaf) memset(leaves32, 0, (size_t)total_cells * 32);
    if (tap.passes == 0) return OK;  // no cell in the whole call: nothing was launched
    if (counts2) { counts2[0] = tap.commitments_decoded; counts2[1] = tap.scalar_muls; }
    if (digests32) memcpy(digests32, tap.digests.data(), (size_t)B * 32);
    if (leaves32 && in.leaf) {  // the pass holds the cells of the problems that passed validation, back to back: into the caller's order
        size_t at = 0, flat = 0;
        for (int b = 0; b < B; b++) {
            const size_t nb = (size_t)in.cells_of((uint64_t)b);
            if (st[b] != ERR_INPUT && nb) { memcpy(leaves32 + flat * 32, tap.leaves.data() + at * 32, nb * 32); at += nb; }
            flat += nb;
        }
    }
    for (int b = 0; b < B; b++) {
        if (st[b] == OK && in.cells_of((uint64_t)b) > 0) compress2(sums96 + 96 * (size_t)b, tap.sums.data() + (size_t)2 * b * sizeof(JacQ));
        for (int j = 0; j < 4; j++) rho[4 * b + j] = tap.rho[4 * (size_t)b + j];
    }
    if (tap.folded) compress2(fold96, tap.fold.data());
    for (uint64_t q = 0; q < *n_probes && q < max_probes; q++) {
        for (int j = 0; j < 3; j++) probe_ranges[3 * q + j] = tap.probes[3 * q + j];
        compress2(probe_sums96 + 96 * q, tap.probe_sums.data() + (size_t)2 * q * sizeof(JacQ));
    }
    return OK;
}

// The public call's passes with their tap set (point_many.hip), optionally cut at a forced pass size.
int Engine::test_verify_kzg_proof_many_sums(uint64_t n, const PointManyInput& in, uint64_t forced_pass, int32_t* verified, int32_t* status,
                                            uint64_t* pass_starts, uint64_t max_passes, uint64_t* n_passes, uint8_t* leaves32, uint8_t* seeds32, uint32_t* rho,
                                            uint8_t* fold96, int32_t* fold_verdicts, int32_t* probes4, uint8_t* probe_sums96, uint64_t max_probes,
                                            uint64_t* n_probes, uint8_t* zs32, uint8_t* ys32) {
    if (n < 1 || n > (1u << 20) || forced_pass > (1u << 20)) return ERR_INPUT;
    if (in.from_blobs && (!zs32 || !ys32)) return ERR_INPUT;
    const uint64_t pass = forced_pass ? forced_pass : (uint64_t)(in.from_blobs ? BLOB_MANY_PASS : POINT_MANY_PASS);
    if ((n + pass - 1) / pass > max_passes) return ERR_INPUT;
    std::vector<int> ver(n), st(n);
    PointManyTap tap;
    tap.pass_size = (int)forced_pass;
    const int rc = verify_kzg_proof_many(n, in, ver.data(), st.data(), &tap);
    if (rc) return rc;
    test_search_stats_[0] = (uint64_t)tap.device_probes;
    test_search_stats_[1] = tap.probes.size() / 4;
    auto compress2 = [](uint8_t* out96, const uint8_t* two) {  // a slot that still holds its poison comes out as 0xff bytes
        for (int j = 0; j < 2; j++) {
            JacQ s;
            memcpy(&s, two + (size_t)j * sizeof(JacQ), sizeof(JacQ));
            if (s.x.v[0] == 0xffffffffu && s.z.v[0] == 0xffffffffu) memset(out96 + 48 * j, 0xff, 48);
            else g1_compress(out96 + 48 * j, to_affine(jac_from_jacq(s)));
        }
    };
    for (uint64_t i = 0; i < n; i++) { verified[i] = st[i] == OK && ver[i] != 0; status[i] = st[i]; }
    const uint64_t np = tap.pass_starts.size() - 1;
    *n_passes = np;
    for (uint64_t p = 0; p <= np; p++) pass_starts[p] = tap.pass_starts[p];
    memcpy(leaves32, tap.leaves.data(), (size_t)n * 32);
    if (in.from_blobs) {
        memcpy(zs32, tap.zs.data(), (size_t)n * 32);
        memcpy(ys32, tap.ys.data(), (size_t)n * 32);
    }
    memcpy(rho, tap.rho.data(), (size_t)n * 16);
    memcpy(seeds32, tap.seeds.data(), (size_t)np * 32);
    for (uint64_t p = 0; p < np; p++) {
        compress2(fold96 + 96 * p, tap.fold.data() + (size_t)2 * p * sizeof(JacQ));
        fold_verdicts[p] = tap.fold_verdict[p];
    }
    *n_probes = tap.probes.size() / 4;
    for (uint64_t q = 0; q < *n_probes && q < max_probes; q++) {
        for (int j = 0; j < 4; j++) probes4[4 * q + j] = tap.probes[4 * q + j];
        compress2(probe_sums96 + 96 * q, tap.probe_sums.data() + (size_t)2 * q * sizeof(JacQ));
    }
    return OK;
}

// k_pairing_check on its own, next to the host's checks of the same pairs.  The pairs are decompressed here, on the host (on the curve;
// no subgroup test: the pairing of the test's points is what it is either way), and become JacQ as the passes' folds are.
int Engine::test_pairing_check_many(int key, uint64_t n64, const uint8_t* pairs48, int flags, int8_t* out_gpu, int8_t* out_host, uint8_t* out_miller_gpu,
                                    uint8_t* out_miller_host) {
    if (!d_pairing_) return ERR_INPUT;  // (a setup with a key at infinity: no device route)
    const int n = (int)n64;
    std::vector<JacQ> pq((size_t)2 * n);
    for (int i = 0; i < 2 * n; i++) {
        G1Affine a;
        if (g1_decompress(a, pairs48 + (size_t)i * 48) != 0) return ERR_G1;
        G1Jac j = to_jac(a);
        if ((flags & 1) && !is_inf(a)) {  // the same point with Z = i + 2
            Fp z = zero<FpParams>();
            z.v[0] = (uint32_t)i + 2;
            z = to_mont(z);
            const Fp z2 = sqr(z);
            j.x = mul(a.x, z2); j.y = mul(a.y, mul(z2, z)); j.z = z;
        }
        pq[(size_t)i] = jacq_from_jac(j);
    }
    if (flags & 2) {
        const size_t e = (size_t)((unsigned)flags >> 8);
        if (e >= (size_t)n) return ERR_INPUT;
        memset(&pq[2 * e + 1], 0xff, sizeof(JacQ));
    }
    const pairing::G2Prepared* const vk[2] = {key ? g2_tau1_.get() : g2_tau_.get(), g2_neg_gen_.get()};
    const int T = vm_host().T;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        hipStream_t st = stream_;
        PoolBuf d_pairs(*this, pq.size() * sizeof(JacQ)), d_verd(*this, (size_t)n), d_mil(*this, out_miller_gpu ? (size_t)n * sizeof(pairing::Fp12) : 256);
        HIPCK(hipMemcpyAsync(d_pairs.p, pq.data(), pq.size() * sizeof(JacQ), hipMemcpyHostToDevice, st));
        HIPCK(hipMemsetAsync(d_verd.p, 0x7f, (size_t)n, st));  // what the kernel does not write shows
        SYNC_CHECKED(st);
        const auto t0 = std::chrono::steady_clock::now();
        launch::pairing_check(d_pairs.p, d_pairing_key(key ? 2 : 0), d_pairing_key(1), d_pairing_frob(), (int8_t*)d_verd.p, n, st,
                              out_miller_gpu ? d_mil.p : nullptr);
        HIPCK(hipMemcpyAsync(out_gpu, d_verd.p, (size_t)n, hipMemcpyDeviceToHost, st));
        SYNC_CHECKED(st);
        const auto t1 = std::chrono::steady_clock::now();
        if (out_miller_gpu) HIPCK(hipMemcpy(out_miller_gpu, d_mil.p, (size_t)n * sizeof(pairing::Fp12), hipMemcpyDeviceToHost));
        parallel_for(n, T, vm_pool_.get(), [&](int i) { out_host[i] = (int8_t)vm::check_pair(&pq[2 * (size_t)i], vk); });
        const auto t2 = std::chrono::steady_clock::now();
        test_search_stats_[2] = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
        test_search_stats_[3] = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t2 - t1).count();
        if (out_miller_host)
            parallel_for(n, T, vm_pool_.get(), [&](int i) {
                pairing::Fp12 f = pairing::one12();
                if (!vm::poisoned(pq[2 * (size_t)i]) && !vm::poisoned(pq[2 * (size_t)i + 1]))
                    f = pairing::fp12_mul(pairing::miller_loop(to_affine(jac_from_jacq(pq[2 * (size_t)i])), *vk[0]),
                                          pairing::miller_loop(to_affine(jac_from_jacq(pq[2 * (size_t)i + 1])), *vk[1]));
                memcpy(out_miller_host + (size_t)i * sizeof(f), &f, sizeof(f));
            });
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// k_blob_eval_at on its own: blobs and points up, one launch, y and the refusal flags down.
int Engine::test_blob_eval_at(int n, const uint8_t* const* blobs, const uint8_t* zs_be32, uint8_t* out_ys_be32, int32_t* out_bad) {
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        hipStream_t st = stream_;
        PoolBuf d_blobs(*this, (size_t)n * BYTES_PER_BLOB), d_z(*this, (size_t)n * 32), d_zm(*this, (size_t)n * sizeof(Fr)), d_y(*this, (size_t)n * 32),
            d_ym(*this, (size_t)n * sizeof(Fr)), d_bad(*this, (size_t)n * sizeof(int));
        for (int b = 0; b < n; b++)
            HIPCK(hipMemcpyAsync((uint8_t*)d_blobs.p + (size_t)b * BYTES_PER_BLOB, blobs[b], BYTES_PER_BLOB, hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(d_z.p, zs_be32, (size_t)n * 32, hipMemcpyHostToDevice, st));
        HIPCK(hipMemsetAsync(d_y.p, 0xff, (size_t)n * 32, st));  // what the kernel does not write shows
        HIPCK(hipMemsetAsync(d_bad.p, 0xff, (size_t)n * sizeof(int), st));
        launch::fr_from_be32(n, (const uint8_t*)d_z.p, d_zm.p, nullptr, /*reduce=*/true, st);
        launch::blob_eval_at(n, (const uint8_t*)d_blobs.p, d_zm.p, (uint8_t*)d_y.p, d_ym.p, (int*)d_bad.p, d_w29_, n_inv4096_, st);
        HIPCK(hipGetLastError());
        // the Montgomery copy must say the same: it comes down through the existing codec
        launch::fr_mont_to_be32(n, d_ym.p, (uint8_t*)d_z.p, st);
        std::vector<uint8_t> y2((size_t)n * 32);
        HIPCK(hipMemcpyAsync(out_ys_be32, d_y.p, (size_t)n * 32, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(y2.data(), d_z.p, (size_t)n * 32, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(out_bad, d_bad.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
        SYNC_CHECKED(st);
        if (memcmp(y2.data(), out_ys_be32, (size_t)n * 32) != 0) throw std::runtime_error("k_blob_eval_at: the two forms of y differ");
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// k_blob_to_extension on its own: the blobs up into the first halves of their slices (the copy of cells 0..63), one launch, the slices down.
int Engine::test_blob_extension(int n, const uint8_t* const* blobs, uint8_t* out_cells, int32_t* out_bad) {
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        hipStream_t st = stream_;
        PoolBuf d_cells(*this, (size_t)n * 2 * BYTES_PER_BLOB), d_bad(*this, (size_t)n * sizeof(int));
        HIPCK(hipMemsetAsync(d_cells.p, 0xff, (size_t)n * 2 * BYTES_PER_BLOB, st));  // what the kernel does not write shows
        HIPCK(hipMemsetAsync(d_bad.p, 0, (size_t)n * sizeof(int), st));              // the status word is OR-ed into, as in a pass
        for (int b = 0; b < n; b++)
            HIPCK(hipMemcpyAsync((uint8_t*)d_cells.p + blob_cells_slice((size_t)b).blob_at, blobs[b], BYTES_PER_BLOB, hipMemcpyHostToDevice, st));
        launch::blob_to_extension(n, (uint8_t*)d_cells.p, (int*)d_bad.p, d_w29_, n_inv4096_, st);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(out_cells, d_cells.p, (size_t)n * 2 * BYTES_PER_BLOB, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(out_bad, d_bad.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
        SYNC_CHECKED(st);
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// k_blob_to_columns on its own: the blobs and the caller's matrix (its guard pattern) up, one launch over blobs [b0, b0 + n) of n_total, the
// matrix down.  The caller (c_api_hooks.cpp) has checked b0 + n <= n_total: every address the launch forms lies inside the matrix.
int Engine::test_blob_to_columns(int n, const uint8_t* const* blobs, uint64_t n_total, uint64_t b0, int blob_half, uint8_t* matrix, int32_t* out_bad) {
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        hipStream_t st = stream_;
        const size_t m_bytes = (size_t)N_CELLS * n_total * BYTES_PER_CELL;
        PoolBuf d_blobs(*this, (size_t)n * BYTES_PER_BLOB), d_m(*this, m_bytes), d_bad(*this, (size_t)n * sizeof(int));
        for (int b = 0; b < n; b++)
            HIPCK(hipMemcpyAsync((uint8_t*)d_blobs.p + (size_t)b * BYTES_PER_BLOB, blobs[b], BYTES_PER_BLOB, hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(d_m.p, matrix, m_bytes, hipMemcpyHostToDevice, st));
        HIPCK(hipMemsetAsync(d_bad.p, 0, (size_t)n * sizeof(int), st));  // the status word is OR-ed into
        launch::blob_to_columns(n, (const uint8_t*)d_blobs.p, (uint8_t*)d_m.p, launch::Columns{(size_t)n_total, (size_t)b0}, blob_half != 0, (int*)d_bad.p, d_w29_,
                                n_inv4096_, st);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(matrix, d_m.p, m_bytes, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(out_bad, d_bad.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
        SYNC_CHECKED(st);
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// The Reed-Solomon decoder of recovery on its own: the masks, slots and cell bytes staged as recover_batch_to_coeffs (list form) or
// recover_cells_and_kzg_proofs_device (flat form) stage them, then rs_decode with its tap.  The caller (c_api_hooks.cpp) has validated
// the counts and indices.  Outputs canonical big-endian.
static void fr_mont_to_be(uint8_t* out, const uint32_t* mont) {
    Fr x;
    for (int i = 0; i < 8; i++) x.v[i] = mont[i];
    x = from_mont(x);
    for (int i = 0; i < 8; i++) {
        const uint32_t w = x.v[7 - i];
        out[4 * i] = (uint8_t)(w >> 24); out[4 * i + 1] = (uint8_t)(w >> 16); out[4 * i + 2] = (uint8_t)(w >> 8); out[4 * i + 3] = (uint8_t)w;
    }
}
int Engine::test_rs_decode(int R, const uint64_t* n_cells, const uint64_t* const* cell_indices, const uint8_t* const* const* cells, int flat_source,
                           int32_t* status, int32_t* deg, uint8_t* zp, uint8_t* zeval, uint8_t* zcinv, uint8_t* coeffs) {
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        ensure_workspace(R);
        std::vector<uint32_t> present((size_t)R * 4, 0);
        std::vector<int> slot, stof, st_out(R, OK);
        size_t total_cells = 0;
        for (int r = 0; r < R; r++) total_cells += n_cells[r];
        const size_t src_bytes = (flat_source ? (size_t)R * N_CELLS : total_cells) * BYTES_PER_CELL;
        PoolBuf h_src(*this, src_bytes, true), d_src(*this, src_bytes);
        uint8_t* h = (uint8_t*)h_src.p;
        size_t pos = 0;
        for (int r = 0; r < R; r++) {
            if (flat_source) memcpy(h + (size_t)r * N_CELLS * BYTES_PER_CELL, cells[r][0], (size_t)N_CELLS * BYTES_PER_CELL);
            for (uint64_t k = 0; k < n_cells[r]; k++) {
                const int c = (int)cell_indices[r][k], i = brp7(c);
                present[(size_t)r * 4 + (i >> 5)] |= 1u << (i & 31);
                if (!flat_source) memcpy(h + pos * BYTES_PER_CELL, cells[r][k], BYTES_PER_CELL);
                slot.push_back(r * N_CELLS + c);
                stof.push_back(r);
                pos++;
            }
        }
        HIPCK(hipMemcpyAsync(d_src.p, h, src_bytes, hipMemcpyHostToDevice, stream_));
        std::vector<int> h_deg(R);
        std::vector<Fr8> h_zp((size_t)R * 65), h_zeval((size_t)R * N_CELLS), h_zcinv((size_t)R * N_CELLS);
        RsDecodeTap tap;
        tap.deg = h_deg.data(); tap.zp = h_zp.data(); tap.zeval = h_zeval.data(); tap.zcinv = h_zcinv.data();
        const int rc = rs_decode(R, (const uint8_t*)d_src.p, flat_source != 0, slot, stof, present, st_out.data(), &tap);
        if (rc) return rc;
        for (int r = 0; r < R; r++) {
            if (status) status[r] = st_out[r];
            if (deg) deg[r] = h_deg[r];
        }
        for (size_t i = 0; i < h_zp.size() && zp; i++) fr_mont_to_be(zp + 32 * i, h_zp[i].v);
        for (size_t i = 0; i < h_zeval.size() && zeval; i++) fr_mont_to_be(zeval + 32 * i, h_zeval[i].v);
        for (size_t i = 0; i < h_zcinv.size() && zcinv; i++) fr_mont_to_be(zcinv + 32 * i, h_zcinv[i].v);
        if (coeffs) {
            std::vector<Fr8> h_c((size_t)R * N_BLOB);
            HIPCK(hipMemcpy(h_c.data(), d_coeffs_, h_c.size() * sizeof(Fr8), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < h_c.size(); i++) fr_mont_to_be(coeffs + 32 * i, h_c[i].v);
        }
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// ---------------------------------------------------------------------------------------------
// the window tables themselves: introspection, raw entries, the exact audit of table_audit.hpp
std::shared_ptr<Engine::SharedTable> Engine::test_table(int kind, int which) const {
    if (primary_) return primary_->test_table(kind, which);
    if (kind != TAB_FK && kind != TAB_SRS) return nullptr;
    if (which == 2) return start_tab_[kind].lock();
    const TableView v = table_view((TableSel)kind);
    return which == 0 ? v.main : which == 1 ? v.next : nullptr;
}

// out8: nominal width, groups, bases per group, state, ready groups, payload bytes (all blocks, nothing else), groups per builder
// launch (0: unknown), pieces; piece_first_block: the first block (2 group + upper) of each piece.  Returns ERR_INPUT if there is no such table.
int Engine::test_table_info(int kind, int which, int64_t* out8, int32_t* piece_first_block, int max_pieces) {
    const auto t = test_table(kind, which);
    if (!t) return ERR_INPUT;
    const int ready = t->state.load() == 1 ? t->n_groups : t->ready_groups.load(std::memory_order_acquire);
    const int n_pieces = (int)t->piece_count.load(std::memory_order_acquire);
    out8[0] = t->c; out8[1] = t->n_groups; out8[2] = t->nb; out8[3] = t->state.load(); out8[4] = ready;
    out8[5] = (int64_t)t->bytes; out8[6] = t->build_chunk; out8[7] = n_pieces;
    for (int k = 0; k < n_pieces && k < max_pieces && piece_first_block; k++) piece_first_block[k] = t->piece_first_block[k];
    return OK;
}

static const void* table_bases(const void* fk, const void* srs, int kind) { return kind == 0 ? fk : srs; }

// every entry of the table's ready groups through audit::audit_entry on the GPU; findings sorted by (group, window, base, d)
int Engine::test_table_audit(int kind, int which, uint64_t* visited, uint64_t* n_findings, int32_t* findings, int max_findings, double* ms) {
    const auto t = test_table(kind, which);
    if (!t || max_findings < 0) return ERR_INPUT;
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        const int groups = t->state.load() == 1 ? t->n_groups : t->ready_groups.load(std::memory_order_acquire);
        const int FW = launch::TABLE_FINDING_WORDS;
        char* d_out;
        int32_t* d_find;
        HIPCK(hipMalloc(&d_out, launch::SIZEOF_AUDIT_OUT));
        HIPCK(hipMalloc(&d_find, (size_t)std::max(1, max_findings) * FW * sizeof(int32_t)));
        struct { unsigned long long visited; unsigned int n, max; int32_t* f; } h = {0, 0, (unsigned)max_findings, d_find};
        static_assert(sizeof(h) == launch::SIZEOF_AUDIT_OUT, "audit::Out");
        HIPCK(hipMemcpy(d_out, &h, sizeof(h), hipMemcpyHostToDevice));
        hipEvent_t e0, e1;
        HIPCK(hipEventCreate(&e0)); HIPCK(hipEventCreate(&e1));
        HIPCK(hipEventRecord(e0, stream_));
        if (groups > 0) launch::table_audit_device(t->d_blocks, table_bases(d_fk_bases_, d_srs_, kind), t->c, groups, t->nb, d_out, stream_);
        HIPCK(hipGetLastError());
        HIPCK(hipEventRecord(e1, stream_));
        HIPCK(hipStreamSynchronize(stream_));
        float dt = 0;
        HIPCK(hipEventElapsedTime(&dt, e0, e1));
        HIPCK(hipEventDestroy(e0)); HIPCK(hipEventDestroy(e1));
        HIPCK(hipMemcpy(&h, d_out, sizeof(h), hipMemcpyDeviceToHost));
        const int kept = (int)std::min<unsigned>(h.n, (unsigned)max_findings);
        std::vector<std::array<int32_t, 5>> f(kept);
        if (kept) HIPCK(hipMemcpy(f.data(), d_find, (size_t)kept * FW * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::sort(f.begin(), f.end());
        if (kept) memcpy(findings, f.data(), (size_t)kept * FW * sizeof(int32_t));
        *visited = h.visited;
        *n_findings = h.n;
        if (ms) *ms = dt;
        HIPCK(hipFree(d_out)); HIPCK(hipFree(d_find));
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// the 24 words of the entries d0 .. d0 + n - 1 of row (group, window, base), as stored
int Engine::test_table_read(int kind, int which, int group, int window, int base, int d0, int n, uint32_t* out) {
    const auto t = test_table(kind, which);
    if (!t) return ERR_INPUT;
    const int c = t->c, W = launch::glv_windows(c), WL = launch::glv_lower_windows(c);
    const int ready = t->state.load() == 1 ? t->n_groups : t->ready_groups.load(std::memory_order_acquire);
    if (group < 0 || group >= ready || window < 0 || window >= W || base < 0 || base >= t->nb || d0 < 1 || n < 1) return ERR_INPUT;
    const long T = 1l << (launch::glv_window_bits(c, window) - 1);
    if ((long)d0 - 1 + n > T) return ERR_INPUT;
    const int upper = window >= WL ? 1 : 0;
    const size_t in_block = launch::glv_entries_per_base(c, upper ? WL : 0, window) * (size_t)t->nb + (size_t)base * T + (size_t)(d0 - 1);
    const char* blk = (const char*)t->h_blocks[(size_t)group * t->halves + upper];
    if (!blk || in_block + n > t->block_entries[upper]) return ERR_INPUT;
    try {
        HIPCK(hipSetDevice(dev_));
        HIPCK(hipMemcpy(out, blk + in_block * launch::SIZEOF_TABP, (size_t)n * launch::SIZEOF_TABP, hipMemcpyDeviceToHost));
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

// a caller's table (its blocks one after the other: [group][lower | upper], inside a block [window][base][digit]) and its n_groups x nb
// bases (G1Affine), audited on the GPU
int Engine::test_table_audit_buffer(int c, int n_groups, int nb, const uint32_t* table, const uint8_t* bases, uint64_t* visited, uint64_t* n_findings,
                                    int32_t* findings, int max_findings) {
    std::lock_guard<std::recursive_mutex> lk(mu_);
    try {
        HIPCK(hipSetDevice(dev_));
        const int FW = launch::TABLE_FINDING_WORDS, WL = launch::glv_lower_windows(c), W = launch::glv_windows(c);
        const size_t entries = launch::table_glv_entries(c, n_groups, nb), lower = launch::glv_entries_per_base(c, 0, WL) * (size_t)nb,
                     upper = launch::glv_entries_per_base(c, WL, W) * (size_t)nb;
        char *d_tab, *d_bases, *d_out;
        void** d_blocks;
        int32_t* d_find;
        HIPCK(hipMalloc(&d_tab, entries * launch::SIZEOF_TABP));
        HIPCK(hipMalloc(&d_bases, (size_t)n_groups * nb * sizeof(G1Affine)));
        HIPCK(hipMalloc(&d_blocks, (size_t)2 * n_groups * sizeof(void*)));
        HIPCK(hipMalloc(&d_out, launch::SIZEOF_AUDIT_OUT));
        HIPCK(hipMalloc(&d_find, (size_t)std::max(1, max_findings) * FW * sizeof(int32_t)));
        std::vector<void*> hb((size_t)2 * n_groups);
        for (int g = 0; g < n_groups; g++) {
            hb[2 * g] = d_tab + (size_t)g * (lower + upper) * launch::SIZEOF_TABP;
            hb[2 * g + 1] = d_tab + ((size_t)g * (lower + upper) + lower) * launch::SIZEOF_TABP;
        }
        struct { unsigned long long visited; unsigned int n, max; int32_t* f; } h = {0, 0, (unsigned)max_findings, d_find};
        HIPCK(hipMemcpy(d_tab, table, entries * launch::SIZEOF_TABP, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(d_bases, bases, (size_t)n_groups * nb * sizeof(G1Affine), hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(d_blocks, hb.data(), hb.size() * sizeof(void*), hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(d_out, &h, sizeof(h), hipMemcpyHostToDevice));
        launch::table_audit_device(d_blocks, d_bases, c, n_groups, nb, d_out, stream_);
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(stream_));
        HIPCK(hipMemcpy(&h, d_out, sizeof(h), hipMemcpyDeviceToHost));
        const int kept = (int)std::min<unsigned>(h.n, (unsigned)max_findings);
        std::vector<std::array<int32_t, 5>> f(kept);
        if (kept) HIPCK(hipMemcpy(f.data(), d_find, (size_t)kept * FW * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::sort(f.begin(), f.end());
        if (kept) memcpy(findings, f.data(), (size_t)kept * FW * sizeof(int32_t));
        *visited = h.visited;
        *n_findings = h.n;
        HIPCK(hipFree(d_tab)); HIPCK(hipFree(d_bases)); HIPCK(hipFree(d_blocks)); HIPCK(hipFree(d_out)); HIPCK(hipFree(d_find));
    } catch (const std::exception& e) {
        set_error(e);
        return ERR_DEVICE;
    }
    return OK;
}

}  // namespace kzg
