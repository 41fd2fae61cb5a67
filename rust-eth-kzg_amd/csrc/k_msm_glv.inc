// Fixed-base MSM over a GLV window table of width GLV_WIDTH (stage D of compute_cells_and_kzg_proofs; replaces
// FixedBaseMSMPrecompWindow::msm, crates/cryptography/bls12_381/src/fixed_base_msm_window.rs:102-168, and its batched
// affine adder, batch_addition.rs:142-232).  Included by k_msm_glv<width>.hip: one translation unit per width, so that
// `make -j` compiles the widths in parallel.
//
// Every FK20 scalar is split k = k1 + k2 lambda with |k1|, |k2| < 2^127 (glv.hpp; k_glv_split in k_msm.hip does it in
// place: 32 bytes = |k1| (sign in bit 127) | |k2| (sign in bit 127)), and phi(x, y) = (beta x, y) = [lambda](x, y) is
// applied once to the SUM of the k2 terms (phi is a homomorphism), so ONE table over W = ceil(128 / C) windows of C bits
// serves both halves: T[group][w][base][d] = d 2^(C w) P, d = 1 .. 2^(C-1), packed canonical coordinates (TabS, 2 x 48 B:
// the centred 30-bit digits of the signed 13-digit field, curve30.hpp; k_table.hip: k_table_fill_packed).  The top window
// never carries out: its value is below 2^(127 - C (W - 1)) <= 2^(C-1).
// ARITHMETIC (round 5): the sums run in the signed 13 x 30-bit field (fp30.hpp, curve30.hpp: 3,055 multiply-adds per gathered
// addition instead of 3,542, no carry sweeps, floor-digit products, fused subtractions); the folds too; a kernel's results
// leave in the 14 x 29-bit form (JacQ) that the G1 linear map reads.
// The table is NOT one allocation: a group's lower WL = ceil(W / 2) windows and its upper W - WL windows are two blocks reached
// through a device array of pointers (TabBlocks: blocks[2 group + upper]), so that the engine can allocate the 206 GB of
// the widest table in pieces of 0.8 GB (a single hipMalloc of that size stalls every other HIP call of the process for
// seconds), publish it group by group while it is built, and run the groups not yet built on the table the context
// started on: every kernel takes a group range [g0, g0 + gcnt) of the n_groups MSMs per slice.
// 2 W gathered additions per (scalar, base): 16 at C = 16 (206 GB), 18 at 15 (116 GB), 20 at 14 (64 GB), 22 at 12
// (18 GB), 32 at 8 (1.6 GB: the table a context starts on while the wide one is built) -- against 19 for a plain
// table of width 14 that needs 163 GB: the endomorphism halves the memory per window bit.
#include "engine.hpp"
#include <stdexcept>
#include "kcommon.hpp"
#include "curve30.hpp"
#include "g1_coop.hpp"
#include "g1_coop30.hpp"
#include "launch.hpp"

#ifndef GLV_WIDTH
#error "define GLV_WIDTH before including k_msm_glv.inc"
#endif

#ifndef GLV_GROUP_MAJOR
#define GLV_GROUP_MAJOR 1
#endif
#define GLV_CAT_(a, b) a##b
#define GLV_CAT(a, b) GLV_CAT_(a, b)
namespace kzg {
namespace GLV_CAT(glv, GLV_WIDTH) {  // one copy per width (a named namespace: profilers show kzg::glv16::k_msm_glv_lane<1> ...)

constexpr int C = GLV_WIDTH, W = launch::glv_windows(GLV_WIDTH);
constexpr int WL = (W + 1) / 2;  // windows of the lower block of a group; the upper block has W - WL
// MIXED window widths (launch.hpp): W windows cover exactly 128 bits, the lowest RW of them BW + 1 bits wide, the others BW
// (width 16: 8 x 16; 15: 2 x 15 + 7 x 14; 14: 8 x 13 + 2 x 12; 12: 7 x 12 + 4 x 11; 8: 16 x 8).  C names the table and bounds a digit.
constexpr int BW = launch::glv_base_bits(GLV_WIDTH), RW = launch::glv_wide_windows(GLV_WIDTH);
__device__ __forceinline__ int win_bits(int w) { return BW + (w < RW ? 1 : 0); }
__device__ __forceinline__ int win_lo(int w) { return w * BW + (w < RW ? w : RW); }
// entries per base of the windows [w0, w): sum of 2^(bits - 1) = those of base width + one more 2^(BW - 1) per wide window
__device__ __forceinline__ size_t win_entries(int w0, int w) {
    const int wide = (w < RW ? w : RW) - (w0 < RW ? w0 : RW);
    return ((size_t)(w - w0) << (BW - 1)) + ((size_t)wide << (BW - 1));
}
// entry (w, i, a) of `group`: the block pointer and the window's index inside its block
__device__ __forceinline__ const TabS* tab_block(const launch::TabBlocks& tb, int group, int upper) {
    return reinterpret_cast<const TabS*>(tb.blocks[2 * group + upper]);
}
__device__ __forceinline__ const TabS* tab_window(const launch::TabBlocks& tb, int group, int w, int nb) {
    const int upper = w >= WL ? 1 : 0;
    return tab_block(tb, group, upper) + win_entries(upper ? WL : 0, w) * (size_t)nb;
}
static_assert(W * BW + RW == 128 && RW < W, "the W windows cover the 128-bit half exactly");
static_assert(BW >= 7 && BW + (RW ? 1 : 0) <= 16 && BW + (RW ? 1 : 0) <= C, "wave-wide table fill needs 64 entries per window; digits are taken from 17 bits at most");

using MsmAcc = XyzzS;
struct GlvScalar { uint32_t h[2][4]; };
static_assert(sizeof(GlvScalar) == sizeof(Fr), "split in place");

// Where an MSM's sum goes: out_fmt 0 = the 14 x 29-bit form (JacQ: the stage hook, the interpolation MSM of verify_many.hip), 1 = the
// signed 13 x 30-bit form as it stands (JacS, 156 B: the prover, recovery and the commitments compute in it -- k_g1slp.hip,
// k_g1circ.hip, k_g1misc.hip -- so nothing is converted between the MSM and the compression).  `out` then addresses JacS.
__device__ __forceinline__ void store_sum(JacQ* __restrict__ out, size_t idx, const JacS& s, int out_fmt) {
    if (out_fmt) reinterpret_cast<JacS*>(out)[idx] = s;
    else out[idx] = jacq_from_jacs(s);
}
struct PackLine { uint4 q[6]; };
// The entry pointer comes out of the block-pointer array, so the compiler cannot tell its address space and would emit FLAT
// loads; those return out of order against other memory operations, every wait on one becomes vmcnt(0), and the loop then
// waits for the entry it has just requested (a full memory latency per addition).  The table is global memory: say so.
__device__ __forceinline__ PackLine load_pack(const TabS* p) {
    PackLine l;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const uint32_t __attribute__((address_space(1))) * GlobalWordPtr;
    GlobalWordPtr s = (GlobalWordPtr)(uintptr_t)p;
#pragma unroll
    for (int i = 0; i < 6; i++) l.q[i] = make_uint4(s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3]);  // merged into six 16-byte loads
#else
    const uint4* s = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int i = 0; i < 6; i++) l.q[i] = s[i];
#endif
    return l;
}
__device__ __forceinline__ AffS pack_to_affs(const PackLine& l) {  // 12 sign extensions + 11 funnel shifts per coordinate
    uint32_t w[24];
#pragma unroll
    for (int i = 0; i < 6; i++) { w[4 * i] = l.q[i].x; w[4 * i + 1] = l.q[i].y; w[4 * i + 2] = l.q[i].z; w[4 * i + 3] = l.q[i].w; }
    return tabs_unpack(w);
}
// signed Booth digit of window w (< W) of a 128-bit magnitude read from memory (sign bit 127 ignored): the C bits of the
// window and the bit below it (booth_encoding.rs:4-46; window 0 is padded with a zero bit)
__device__ __forceinline__ int booth_mem(const uint32_t* m, int w) {
    const int cw = win_bits(w);
    const uint32_t MASK = (1u << (cw + 1)) - 1;
    uint32_t x;
    if (w == 0) x = (m[0] << 1) & MASK;
    else {
        const int lo = win_lo(w) - 1, word = lo >> 5, sh = lo & 31;  // lo < 127: word <= 3
        uint64_t two = word == 3 ? (m[3] & 0x7fffffffu) : m[word];
        if (word + 1 < 4) two |= (uint64_t)(word + 1 == 3 ? (m[3] & 0x7fffffffu) : m[word + 1]) << 32;
        x = (uint32_t)(two >> sh) & MASK;
    }
    const int t = (int)((x + 1) >> 1);
    return (x >> cw) ? t - (1 << cw) : t;
}
__device__ __forceinline__ int out_pos(int group, int brp_bits) {
    return brp_bits ? (int)(__brev((unsigned)group) >> (32 - brp_bits)) : group;
}

#if GLV_WIDTH == 16
// four chunks per MSM (the large-batch schedule; round 2's kernel, its digits from a 65-bit shift register): block = 64 MSMs x 4
// waves, wave = chunk: k1 windows 0-3, k1 windows 4-7, k2 windows 0-3, k2 windows 4-7; fold (c0 + c1) + phi(c2 + c3) through LDS
__global__ __launch_bounds__(256, 2) void k_msm_glv_chunked(const GlvScalar* __restrict__ scalars, launch::TabBlocks table,
                                                            JacQ* __restrict__ out, int n_groups, int n_slices, int nb,
                                                            int out_stride, int brp_bits, Fs<1, DC> beta, int out_fmt) {
    __shared__ JacS red[256];
    const int tid = threadIdx.x, chunk = tid >> 6, lane = tid & 63;
    const int half = chunk >> 1, w0 = (chunk & 1) * 4;
#if GLV_GROUP_MAJOR
    // a wave's 64 lanes are 64 slices (blobs) of ONE group: they gather from the same 3 MB table row per (window, base) instead of
    // from 64 table regions 1.6 GB apart, and consecutive blocks stay in the group (16 groups' tables in use at a time, not all 128)
    const int slice_blocks = (n_slices + 63) / 64;
    const int group_of_block = table.g0 + (int)(blockIdx.x / slice_blocks), slice_of_lane = (int)(blockIdx.x % slice_blocks) * 64 + lane;
    const long m = (long)slice_of_lane * n_groups + group_of_block;  // MSM index = slice * n_groups + group
    const bool active = slice_of_lane < n_slices;
#else
#error "the slice-major block order has no group range"
#endif
    int slice = 0, group = 0;
    MsmAcc acc = xyzz30_inf();
    if (active) {
        slice = (int)(m / n_groups);
        group = (int)(m % n_groups);
        const GlvScalar* sc = scalars + (size_t)m * nb;
        static_assert(WL == 4, "a chunk of the width-16 kernel is one block of its group");
        const TabS* tb = tab_block(table, group, chunk & 1);  // entry (w, i, a): tb[(((w - w0) * nb + i) << 15) + a]
        // this chunk's 64 bits of the half, kept as a 65-bit shift register v = (bits << 1) | the bit below
        uint64_t v = 0;
        uint32_t vtop = 0, sneg = 0;
        auto fetch = [&](int i) {
            const uint32_t* h = sc[i].h[half];
            const uint32_t a0 = h[0], a1 = h[1], a2 = h[2], a3 = h[3];
            sneg = a3 >> 31;
            const uint64_t bits = (chunk & 1) ? (((uint64_t)(a3 & 0x7fffffffu) << 32) | a2) : (((uint64_t)a1 << 32) | a0);
            const uint32_t below = (chunk & 1) ? (a1 >> 31) : 0u;
            v = (bits << 1) | below;
            vtop = (uint32_t)(bits >> 63);
        };
        auto take = [&]() {  // signed digit of the low 17 bits, then shift by 16
            const uint32_t x = (uint32_t)v & 0x1ffffu;
            v = (v >> 16) | ((uint64_t)vtop << 48);
            vtop = 0;
            const int t = (int)((x + 1) >> 1);
            return (x >> 16) ? t - 65536 : t;
        };
        fetch(0);
        int i = 0, w = 0;
        int d = take();
        uint32_t dneg = sneg;
        PackLine cur = load_pack(tb + (d ? (d < 0 ? -d : d) - 1 : 0));
        const int total = 4 * nb;
#pragma unroll 1
        for (int e = 0; e < total; e++) {
            int w2 = w + 1, i2 = i;
            const uint32_t dneg_cur = dneg;
            if (w2 == 4) {
                w2 = 0;
                i2 = i + 1;
                fetch(i2 < nb ? i2 : 0);
            }
            const int d2 = i2 < nb ? take() : 0;
            dneg = sneg;
            const int a2 = d2 ? (d2 < 0 ? -d2 : d2) - 1 : 0;
            const PackLine nxt = load_pack(tb + ((((size_t)w2 * nb + (i2 < nb ? i2 : 0)) << (C - 1)) + a2));
            if (d != 0) acc = add_mixed(acc, pack_to_affs(cur), (d < 0) != (dneg_cur != 0));
            cur = nxt;
            d = d2;
            w = w2;
            i = i2;
        }
    }
    JacS sum = to_jacs(acc);
    red[tid] = sum;
    __syncthreads();
    if ((chunk & 1) == 0) sum = add(sum, red[tid + 64]);
    if (chunk == 2) sum = apply_phi(sum, beta);
    __syncthreads();
    if (chunk == 2) red[tid] = sum;
    __syncthreads();
    if (chunk == 0) {
        sum = add(sum, red[tid + 128]);
        if (active) store_sum(out, (size_t)out_pos(group, brp_bits) * out_stride + slice, sum, out_fmt);
    }
}
#endif

#if GLV_WIDTH != 16
// four chunks per MSM at any width: block = 64 MSMs x 4 waves, wave = (half, lower / upper part of the W windows); the half
// scalar sits in the 127-bit shift register of the lane kernel, the upper part first skips the lower part's windows; fold
// (c0 + c1) + phi(c2 + c3) through LDS.  Short waves that the hardware deals out as slots free up balance better than the
// long waves of the lane kernels (measured at width 16: -1.5 % against a lane per MSM), so this is the large-batch schedule.
__global__ __launch_bounds__(256, 2) void k_msm_glv_chunked(const GlvScalar* __restrict__ scalars, launch::TabBlocks table,
                                                            JacQ* __restrict__ out, int n_groups, int n_slices, int nb,
                                                            int out_stride, int brp_bits, Fs<1, DC> beta, int out_fmt) {
    __shared__ JacS red[256];  // (WL windows in the lower part, W - WL in the upper: the two blocks of a group)
    const int tid = threadIdx.x, chunk = tid >> 6, lane = tid & 63;
    const int half = chunk >> 1, w0 = (chunk & 1) ? WL : 0, nw = (chunk & 1) ? W - WL : WL;
#if GLV_GROUP_MAJOR
    // a wave's 64 lanes are 64 slices (blobs) of ONE group: they gather from the same 3 MB table row per (window, base) instead of
    // from 64 table regions 1.6 GB apart, and consecutive blocks stay in the group (16 groups' tables in use at a time, not all 128)
    const int slice_blocks = (n_slices + 63) / 64;
    const int group_of_block = table.g0 + (int)(blockIdx.x / slice_blocks), slice_of_lane = (int)(blockIdx.x % slice_blocks) * 64 + lane;
    const long m = (long)slice_of_lane * n_groups + group_of_block;  // MSM index = slice * n_groups + group
    const bool active = slice_of_lane < n_slices;
#else
#error "the slice-major block order has no group range"
#endif
    int slice = 0, group = 0;
    MsmAcc acc = xyzz30_inf();
    if (active) {
        slice = (int)(m / n_groups);
        group = (int)(m % n_groups);
        const GlvScalar* sc = scalars + (size_t)m * nb;
        const TabS* tb = tab_block(table, group, chunk & 1);  // entry (w, i, a): tb[(((w - w0) * nb + i) << (C-1)) + a]
        uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, below = 0, sneg = 0;
        auto take = [&](int cw) {  // signed Booth digit of the low cw bits + the bit below, then shift by cw
            const uint32_t x = ((r0 & ((1u << cw) - 1)) << 1) | below;
            below = (r0 >> (cw - 1)) & 1u;
            r0 = __funnelshift_r(r0, r1, cw);
            r1 = __funnelshift_r(r1, r2, cw);
            r2 = __funnelshift_r(r2, r3, cw);
            r3 >>= cw;
            const int t = (int)((x + 1) >> 1);
            return (x >> cw) ? t - (1 << cw) : t;
        };
        auto fetch = [&](int i) {
            const uint4 h = *reinterpret_cast<const uint4*>(sc[i].h[half]);
            r0 = h.x; r1 = h.y; r2 = h.z;
            sneg = h.w >> 31;
            r3 = h.w & 0x7fffffffu;
            below = 0;
            if (chunk & 1)
                for (int k = 0; k < WL; k++) (void)take(win_bits(k));  // the lower part's windows belong to the neighbouring wave
        };
        fetch(0);
        int i = 0, w = 0;  // w: window inside this chunk's part (table window w0 + w)
        int d = take(win_bits(w0));
        uint32_t dneg = sneg;
        PackLine cur = load_pack(tb + (d ? (d < 0 ? -d : d) - 1 : 0));
        const int total = nw * nb;
#pragma unroll 1
        for (int e = 0; e < total; e++) {
            int w2 = w + 1, i2 = i;
            const uint32_t dneg_cur = dneg;
            if (w2 == nw) {
                w2 = 0;
                i2 = i + 1;
                fetch(i2 < nb ? i2 : 0);
            }
            const int cw2 = win_bits(w0 + w2);
            const int d2 = i2 < nb ? take(cw2) : 0;
            dneg = sneg;
            const int a2 = d2 ? (d2 < 0 ? -d2 : d2) - 1 : 0;
            // entry (w, i, a) of this part's block: [window][base][digit] with the window's own digit count
            const PackLine nxt = load_pack(tb + (win_entries(w0, w0 + w2) * (size_t)nb + ((size_t)(i2 < nb ? i2 : 0) << (cw2 - 1)) + a2));
            if (d != 0) acc = add_mixed(acc, pack_to_affs(cur), (d < 0) != (dneg_cur != 0));
            cur = nxt;
            d = d2;
            w = w2;
            i = i2;
        }
    }
    JacS sum = to_jacs(acc);
    red[tid] = sum;
    __syncthreads();
    if ((chunk & 1) == 0) sum = add(sum, red[tid + 64]);
    if (chunk == 2) sum = apply_phi(sum, beta);
    __syncthreads();
    if (chunk == 2) red[tid] = sum;
    __syncthreads();
    if (chunk == 0) {
        sum = add(sum, red[tid + 128]);
        if (active) store_sum(out, (size_t)out_pos(group, brp_bits) * out_stride + slice, sum, out_fmt);
    }
}
#endif

// ---- medium batches: thread = (MSM, joint window u < 2 W): u < W is window u of k1, u >= W window u - W of k2 (both read
// the SAME table rows); 256 / (2 W) MSMs per block; phi per lane, then a tree over the 2 W lanes of an MSM through LDS ----
// SPLIT = 2 (round 6; batches of <= 32 blobs, where a lane per window leaves half the wave slots empty and the launch lasts as long as
// one lane's 64 dependent additions): two lanes per joint window, each over half of the bases -- the chain is 32 additions and the tree
// one level deeper.
template <int SPLIT>
__global__ __launch_bounds__(256, 2) void k_msm_glv_windowed(const GlvScalar* __restrict__ scalars, launch::TabBlocks table,
                                                             JacQ* __restrict__ out, int n_groups, int n_slices, int nb,
                                                             int out_stride, int brp_bits, Fs<1, DC> beta, int out_fmt) {
    static_assert(SPLIT == 1 || SPLIT == 2, "lanes per joint window");
    constexpr int U = 2 * W * SPLIT, PB = 256 / U;
    __shared__ JacS red[256];
    const int tid = threadIdx.x, local = tid / U, u = tid % U, part = u / (2 * W), uw = u % (2 * W), half = uw >= W ? 1 : 0, w = half ? uw - W : uw;
    const long q_lin = (long)blockIdx.x * PB + local;  // linear index, GROUP-major: consecutive lanes / blocks are slices (blobs) of one group -- the same table rows
    const long m = (q_lin % n_slices) * (long)n_groups + table.g0 + q_lin / n_slices;  // MSM index = slice * n_groups + group (the scalars' layout)
    const bool active = local < PB && q_lin < (long)table.gcnt * n_slices;
    MsmAcc acc = xyzz30_inf();
    int group = 0, slice = 0;
    if (active) {
        slice = (int)(m / n_groups);
        group = (int)(m % n_groups);
        const GlvScalar* sc = scalars + (size_t)m * nb;
        const TabS* tb = tab_window(table, group, w, nb);
        // the next base's digit and table entry are requested before the current addition (as in the chunked kernel): without
        // it every addition waited for two dependent reads, the scalar and then the entry it selects
        const int i0 = part * (nb / SPLIT), i1 = SPLIT == 1 ? nb : (part + 1 == SPLIT ? nb : i0 + nb / SPLIT);  // this lane's bases
        const uint32_t* h0 = sc[i0].h[half];
        int d = booth_mem(h0, w);
        bool neg = (d < 0) != ((h0[3] >> 31) != 0);
        PackLine cur = load_pack(tb + (((size_t)i0 << (win_bits(w) - 1)) + (d ? (d < 0 ? -d : d) - 1 : 0)));
#pragma unroll 1
        for (int i = i0; i < i1; i++) {
            const int i2 = i + 1 < i1 ? i + 1 : i0;
            const uint32_t* h = sc[i2].h[half];
            const int d2 = i + 1 < i1 ? booth_mem(h, w) : 0;
            const bool neg2 = (d2 < 0) != ((h[3] >> 31) != 0);
            const PackLine nxt = load_pack(tb + (((size_t)i2 << (win_bits(w) - 1)) + (d2 ? (d2 < 0 ? -d2 : d2) - 1 : 0)));
            if (d != 0) acc = add_mixed(acc, pack_to_affs(cur), neg);
            cur = nxt;
            d = d2;
            neg = neg2;
        }
    }
    JacS sum = to_jacs(acc);
    if (half) sum = apply_phi(sum, beta);
    red[tid] = sum;
    __syncthreads();
    // The tree over the U partial sums of each of the block's PB MSMs, four lanes per addition (g1_coop30.hpp: 5 reductions deep instead
    // of 10) and whole waves only: a level's additions are dealt to the block's 64 quads as jobs (MSM, pair); a wave without a job
    // skips, the quads behind the last job -- or on a sum without a partner (U need not be a power of two) -- repeat another job and
    // store nothing (a wave with few lanes in use is the slow one: k_g1slp.hip).  Round 6; before: one lane per addition, and from
    // the second level on 16, 8, 4 lanes of a wave in use.
    {
        const int quad = tid & 3, qd = tid >> 2, wave_qd = (tid & ~63) >> 2;
#pragma unroll 1
        for (int span = 1; span < U; span <<= 1) {
            const int jpm = (U + 2 * span - 1) / (2 * span), jobs = PB * jpm;  // jobs per MSM (its last sum may have no partner)
#pragma unroll 1
            for (int j0 = 0; j0 < jobs; j0 += 64) {
                if (j0 + wave_qd < jobs) {
                    int j = j0 + qd;
                    const bool mine = j < jobs;
                    if (!mine) j = jobs - 1;
                    const int lc = j / jpm, uu = (j % jpm) * 2 * span;
                    const bool has = uu + span < U;
                    const int a = lc * U + (has ? uu : 0);
                    const JacS r = coop4_add(red[a], red[a + span], false, quad);
                    if (mine && has && quad == 0) red[a] = r;
                }
            }
            __syncthreads();
        }
    }
    if (active && u == 0) store_sum(out, (size_t)out_pos(group, brp_bits) * out_stride + slice, red[tid], out_fmt);
}

// ---- a handful of blobs: one block of NT threads per MSM; the lower half of the block takes the k1 terms, the upper half the k2 terms;
// tree fold with four lanes per addition ----
template <int NT>
__global__ __launch_bounds__(NT) void k_msm_glv_flat(const GlvScalar* __restrict__ scalars, launch::TabBlocks table,
                                                     JacQ* __restrict__ out, int n_groups, int nb, int out_stride, int brp_bits,
                                                     Fs<1, DC> beta, int out_fmt) {
    __shared__ JacS red[NT];
    constexpr int HL = NT / 2;
    const int tid = threadIdx.x, half = tid / HL, l = tid % HL;
    const int slice = (int)(blockIdx.x / table.gcnt), group = table.g0 + (int)(blockIdx.x % table.gcnt);
    const long m = (long)slice * n_groups + group;
    const GlvScalar* sc = scalars + (size_t)m * nb;
    MsmAcc xacc = xyzz30_inf();
    for (int e = l; e < W * nb; e += HL) {
        const int w = e / nb, i = e - w * nb;
        const uint32_t* h = sc[i].h[half];
        const int d = booth_mem(h, w);
        if (d != 0) {
            const bool neg = (d < 0) != ((h[3] >> 31) != 0);
            const AffS p = pack_to_affs(load_pack(tab_window(table, group, w, nb) + (((size_t)i << (win_bits(w) - 1)) + ((d < 0 ? -d : d) - 1))));
            xacc = add_mixed(xacc, p, neg);
        }
    }
    JacS acc = to_jacs(xacc);
    if (half) acc = apply_phi(acc, beta);
    red[tid] = acc;
    coop4_tree_fold<NT>(red, HL, tid);  // the idle lanes of each level share its additions (g1_coop30.hpp): four lanes per addition, 5 reductions deep
    if (tid == 0) store_sum(out, (size_t)out_pos(group, brp_bits) * out_stride + slice, red[0], out_fmt);
}

}  // namespace glv<width>

namespace launch {
using namespace GLV_CAT(glv, GLV_WIDTH);
// (launch.hpp: preload_code_objects) this width's code object is loaded before the table builder starts allocating
void GLV_CAT(preload_k_msm_glv, GLV_WIDTH)() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_msm_glv_flat<256>));
}
// mode: 0 flat (one block per MSM), 1 windowed (a lane per joint window), 3 windowed with two lanes per window, anything else: four chunks per MSM.  The scalars must have been split (launch::glv_split).
void GLV_CAT(msm_glv_w, GLV_WIDTH)(int mode, const void* scalars, const TabBlocks& tb, void* out, int n_groups, int n_slices, int nb,
                                   int out_stride, int brp_bits, const Fp12w& beta, hipStream_t st, int out_fmt) {
    Fp b384;
    for (int i = 0; i < 12; i++) b384.v[i] = beta.v[i];
    const Fs<1, DC> bq = fs_from_fp(b384);
    const long msms = (long)tb.gcnt * n_slices;  // of this launch: groups [g0, g0 + gcnt) of every slice
    if (msms <= 0) return;
    const GlvScalar* sc = (const GlvScalar*)scalars;
    if (mode == 0) {
        // 256 threads per MSM while every block is resident at once (two per CU: 512 MSMs on the 256 CUs of an MI355X = one blob in four
        // segments, or four blobs); beyond that 128 threads -- half the waves, a block's lanes take twice the terms, the fold is a level
        // shorter: 2 blobs 1.22 -> 1.13 ms per step, 5 blobs 1.54 -> 1.49, 8 blobs 1.65 -> 1.57 (tools/ab_flat_msm_block.sh; 64 threads: no better)
        if (msms > 512) k_msm_glv_flat<128><<<(unsigned)msms, 128, 0, st>>>(sc, tb, (JacQ*)out, n_groups, nb, out_stride, brp_bits, bq, out_fmt);
        else k_msm_glv_flat<256><<<(unsigned)msms, 256, 0, st>>>(sc, tb, (JacQ*)out, n_groups, nb, out_stride, brp_bits, bq, out_fmt);
    }
    else if (mode == 1) {
        constexpr int PB = 256 / (2 * W);
        k_msm_glv_windowed<1><<<(unsigned)((msms + PB - 1) / PB), 256, 0, st>>>(sc, tb, (JacQ*)out, n_groups, n_slices, nb, out_stride, brp_bits, bq, out_fmt);
    } else if (mode == 3) {  // two lanes per joint window (the engine: when even that leaves the chip within one round of wave slots)
        constexpr int PB = 256 / (4 * W);
        if (nb % 2) throw std::logic_error("msm_glv: two lanes per window need an even number of bases");
        k_msm_glv_windowed<2><<<(unsigned)((msms + PB - 1) / PB), 256, 0, st>>>(sc, tb, (JacQ*)out, n_groups, n_slices, nb, out_stride, brp_bits, bq, out_fmt);
    } else
        k_msm_glv_chunked<<<(unsigned)tb.gcnt * (unsigned)((n_slices + 63) / 64), 256, 0, st>>>(sc, tb, (JacQ*)out, n_groups, n_slices, nb, out_stride, brp_bits, bq, out_fmt);
}
}  // namespace launch
}  // namespace kzg
