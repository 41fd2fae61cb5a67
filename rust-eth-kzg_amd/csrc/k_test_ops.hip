// Per-operation test kernels (libc_eth_kzg_hooks.so only; tests/test_device_ops.py): every field and point operation the product
// kernels call, at the types and template arguments of their call sites, run one element per operation on raw words -- the device
// compilation under test (fp30_mac.hpp's v_mad_i64_i32 chains, fp29_mac.hpp's v_mad_u64_u32 chains under -DFQ_ASM_MAC, the slow paths
// as real calls through their word buffers) and, for the HD operations, the host pass of the same source.
//
// Operands and results are the device structs as words, fields in declaration order: Fs 13 x int32, Fq 14 x uint32, Fr29 9 words,
// JacS (x, y, z), XyzzS (x, y, zz, zzz), AffS / AffT (x, y), JacQ (x, y, z), AffQ (x, y); a flag (negq, a result bit) is one word.
// The word counts live in OPS[] below; Python reads them through eth_kzg_amd_test_op_info.
//
// The pair and quad forms map operation i onto lanes the way their callers do: COOP consecutive lanes per operation, whole
// 64-lane waves; in the signed field the padding lanes of the last wave repeat the last operation and store nothing
// (k_slp_mulc_coop_s, k_slp_add_coop_s), in the 14 x 29-bit field whole groups beyond the last operation leave
// (k_verify_many.hip).  Every lane of a group writes its own copy of the result, so a lane that ends with a different value shows.
// The tree folds take one block per fold with the callers' block size and first span.
#include "g1_coop.hpp"
#include "g1_coop30.hpp"
#include "fr29.hpp"
#include "launch.hpp"

namespace kzg {
namespace testops {

// ---- words <-> structs ----------------------------------------------------------------------------------------------------
template <int B, int F>
HD Fs<B, F> lds(const int32_t* w) {
    Fs<B, F> r;
    for (int i = 0; i < SL; i++) r.v[i] = w[i];
    return r;
}
template <int B, int F>
HD void sts(int32_t* w, const Fs<B, F>& a) {
    for (int i = 0; i < SL; i++) w[i] = a.v[i];
}
template <int B>
HD Fq<B> ldq(const int32_t* w) {
    Fq<B> r;
    for (int i = 0; i < QL; i++) r.v[i] = (uint32_t)w[i];
    return r;
}
template <int B>
HD void stq(int32_t* w, const Fq<B>& a) {
    for (int i = 0; i < QL; i++) w[i] = (int32_t)a.v[i];
}
HD Fr29 ldr(const int32_t* w) {
    Fr29 r;
    for (int i = 0; i < RL; i++) r.v[i] = (uint32_t)w[i];
    return r;
}
HD void str(int32_t* w, const Fr29& a) {
    for (int i = 0; i < RL; i++) w[i] = (int32_t)a.v[i];
}
HD JacS ld_jacs(const int32_t* w) {
    JacS p;
    p.x = lds<4, DC>(w);
    p.y = lds<1, DC>(w + SL);
    p.z = lds<1, DC>(w + 2 * SL);
    return p;
}
HD void st_jacs(int32_t* w, const JacS& p) {
    sts(w, p.x);
    sts(w + SL, p.y);
    sts(w + 2 * SL, p.z);
}
HD XyzzS ld_xyzz(const int32_t* w) {
    XyzzS p;
    p.x = lds<4, DU>(w);
    p.y = lds<1, DU>(w + SL);
    p.zz = lds<1, DU>(w + 2 * SL);
    p.zzz = lds<1, DU>(w + 3 * SL);
    return p;
}
HD void st_xyzz(int32_t* w, const XyzzS& p) {
    sts(w, p.x);
    sts(w + SL, p.y);
    sts(w + 2 * SL, p.zz);
    sts(w + 3 * SL, p.zzz);
}
HD AffS ld_affs(const int32_t* w) {
    AffS a;
    a.x = lds<1, DC>(w);
    a.y = lds<1, DC>(w + SL);
    return a;
}
HD AffT ld_afft(const int32_t* w) {
    AffT a;
    a.x = lds<1, DC>(w);
    a.y = lds<1, DC>(w + SL);
    return a;
}
HD JacQ ld_jacq(const int32_t* w) {
    JacQ p;
    p.x = ldq<XB>(w);
    p.y = ldq<XB>(w + QL);
    p.z = ldq<ZB>(w + 2 * QL);
    return p;
}
HD void st_jacq(int32_t* w, const JacQ& p) {
    stq(w, p.x);
    stq(w + QL, p.y);
    stq(w + 2 * QL, p.z);
}
HD AffQ ld_affq(const int32_t* w) {
    AffQ a;
    a.x = ldq<1>(w);
    a.y = ldq<1>(w + QL);
    return a;
}

constexpr int JS = 3 * SL, XS = 4 * SL, AS = 2 * SL, JQ = 3 * QL, AQ = 2 * QL;

// ---- the operations -------------------------------------------------------------------------------------------------------
// HD operations: run(in, out), one element.  COOP operations: dev(in, out, sub) on every lane of the group, out = this lane's copy.
#define OP_HD(NAME, IN_W, OUT_W, ...)                                       \
    struct op_##NAME {                                                            \
        static constexpr int IN = IN_W, OUT = OUT_W, COOP = 0, FOLD = 0;     \
        static HD void run(const int32_t* in, int32_t* out) { __VA_ARGS__; }        \
    };

// fp30.hpp: products at the operand classes the kernels combine (C x C, C x U, C x W) and the largest bounds each instantiation allows
OP_HD(fs_mul_cc, 2 * SL, SL, sts(out, mul(lds<16, DC>(in), lds<16, DC>(in + SL))))
OP_HD(fs_mul_cc_du, 2 * SL, SL, sts(out, mul<DU>(lds<16, DC>(in), lds<16, DC>(in + SL))))
OP_HD(fs_mul_cu, 2 * SL, SL, sts(out, mul(lds<4, DC>(in), lds<64, DU>(in + SL))))
OP_HD(fs_mul_cu_du, 2 * SL, SL, sts(out, mul<DU>(lds<4, DC>(in), lds<64, DU>(in + SL))))
OP_HD(fs_mul_cw, 2 * SL, SL, sts(out, mul(lds<4, DC>(in), lds<64, DW>(in + SL))))
OP_HD(fs_mul_cw_du, 2 * SL, SL, sts(out, mul<DU>(lds<4, DC>(in), lds<64, DW>(in + SL))))
OP_HD(fs_sqr, SL, SL, sts(out, sqr(lds<16, DC>(in))))
OP_HD(fs_sqr_du, SL, SL, sts(out, sqr<DU>(lds<16, DC>(in))))
// the MSM step's U2 - X1 (C x U, U injected) and the widest operands of the same instantiation family
OP_HD(fs_mul_inj_m1, 3 * SL, SL, sts(out, mul_inj<-1, DC>(lds<1, DC>(in), lds<1, DU>(in + SL), lds<4, DU>(in + 2 * SL))))
OP_HD(fs_mul_inj_m1_wide, 3 * SL, SL, sts(out, mul_inj<-1, DC>(lds<4, DC>(in), lds<64, DW>(in + SL), lds<32, DW>(in + 2 * SL))))
OP_HD(fs_sqr_inj_m2, 2 * SL, SL, sts(out, sqr_inj<-2, DC>(lds<2, DC>(in), lds<1, DC>(in + SL))))
OP_HD(fs_sqr_inj_m2_wide, 2 * SL, SL, sts(out, sqr_inj<-2, DC>(lds<16, DC>(in), lds<32, DW>(in + SL))))
OP_HD(fs_sqr_inj2, 3 * SL, SL, sts(out, sqr_inj2<-1, -2, DU>(lds<5, DC>(in), lds<1, DC>(in + SL), lds<1, DU>(in + 2 * SL))))
OP_HD(fs_sqr_inj2_wide, 3 * SL, SL, sts(out, sqr_inj2<-1, -2, DC>(lds<16, DC>(in), lds<32, DW>(in + SL), lds<32, DU>(in + 2 * SL))))
OP_HD(fs_mul_add_cccc, 4 * SL, SL,
      sts(out, mul_add<DC>(lds<11, DC>(in), lds<11, DC>(in + SL), lds<11, DC>(in + 2 * SL), lds<11, DC>(in + 3 * SL))))
OP_HD(fs_mul_add_split, 4 * SL, SL,
      sts(out, mul_add<DU>(lds<4, DC>(in), lds<32, DW>(in + SL), lds<32, DW>(in + 2 * SL), lds<4, DC>(in + 3 * SL))))
OP_HD(fs_half_of_triple, SL, SL, sts(out, half_of_triple(lds<1, DC>(in))))
OP_HD(fs_normalise, SL, SL, sts(out, normalise(lds<64, DW>(in))))
OP_HD(fs_canonical, SL, SL, sts(out, canonical(lds<64, DW>(in))))
OP_HD(fs_canonical_of_product, SL, SL, sts(out, canonical_of_product(lds<1, DU>(in))))
OP_HD(fs_product_is_zero, SL, 1, out[0] = product_is_zero(lds<1, DC>(in)) ? 1 : 0)
OP_HD(fs_is_zero_slow, SL, 1, out[0] = is_zero_slow(lds<64, DW>(in)) ? 1 : 0)
OP_HD(fs_neg_du, SL, SL, sts(out, neg(lds<64, DU>(in))))
OP_HD(fs_neg_dw, SL, SL, sts(out, neg(lds<64, DW>(in))))
OP_HD(fs_sub_lazy_du, 2 * SL, SL, sts(out, sub_lazy(lds<32, DU>(in), lds<32, DU>(in + SL))))
OP_HD(fs_regroup_32_to_30, 12, SL, regroup_32_to_30<12>(out, reinterpret_cast<const uint32_t*>(in)))
OP_HD(fs_regroup_30_to_32, SL, 12, regroup_30_to_32(reinterpret_cast<uint32_t*>(out), in))
// packed table entry: two canonical floor-digit coordinates -> 24 words -> the unpacked entry
OP_HD(fs_tabs_pack_unpack, 2 * SL, 24 + 2 * SL, {
    uint32_t* w = reinterpret_cast<uint32_t*>(out);
    tabs_pack_coord(w, lds<1, DU>(in));
    tabs_pack_coord(w + 12, lds<1, DU>(in + SL));
    const AffS a = tabs_unpack(w);
    sts(out + 24, a.x);
    sts(out + 24 + SL, a.y);
})

// fp29.hpp / curve29.hpp
OP_HD(fq_mul, 2 * QL, QL, stq(out, mul(ldq<XB>(in), ldq<XB>(in + QL))))
OP_HD(fq_mul_wide, 2 * QL, QL, stq(out, mul(ldq<4096>(in), ldq<4096>(in + QL))))
OP_HD(fq_sqr, QL, QL, stq(out, sqr(ldq<4096>(in))))
OP_HD(fq_mul_add, 4 * QL, QL, stq(out, mul_add(ldq<2048>(in), ldq<4096>(in + QL), ldq<2048>(in + 2 * QL), ldq<4096>(in + 3 * QL))))
OP_HD(fq_is_zero, QL, 1, out[0] = is_zero(ldq<8>(in)) ? 1 : 0)
OP_HD(fq_product_is_zero, QL, 1, out[0] = product_is_zero(ldq<2>(in)) ? 1 : 0)

// fr29.hpp at the NTT's bounds: 32 r at entry (times a product < 2 r), 56 r after 12 layers (times a canonical twiddle)
OP_HD(fr_mul, 2 * RL, RL, str(out, fr29_mul(ldr(in), ldr(in + RL))))
OP_HD(fr_reduce_once, RL, RL, str(out, fr29_reduce_once(ldr(in))))
OP_HD(fr_partial_reduce, RL, RL, str(out, fr29_partial_reduce(ldr(in))))
OP_HD(fr_add, 2 * RL, RL, str(out, fr29_add(ldr(in), ldr(in + RL))))
OP_HD(fr_sub2r, 2 * RL, RL, str(out, fr29_sub2r(ldr(in), ldr(in + RL))))

// curve30.hpp: the MSM step, the constant multiplication's chain, the folds' general forms, the conversions
OP_HD(xyzz_add_mixed, XS + AS + 1, XS, st_xyzz(out, add_mixed(ld_xyzz(in), ld_affs(in + XS), in[XS + AS] != 0)))
OP_HD(xyzz_to_jacs, XS, JS, st_jacs(out, to_jacs(ld_xyzz(in))))
OP_HD(jacs_dbl_half, JS, JS, st_jacs(out, dbl_half(ld_jacs(in))))
OP_HD(jacs_add_mixed, JS + AS + 1, JS, st_jacs(out, add_mixed(ld_jacs(in), ld_afft(in + JS), in[JS + AS] != 0)))
OP_HD(jacs_add, 2 * JS + 1, JS, st_jacs(out, add(ld_jacs(in), ld_jacs(in + JS), in[2 * JS] != 0)))
OP_HD(jacs_add_sub, 2 * JS, 2 * JS, {
    JacS s, d;
    add_sub(ld_jacs(in), ld_jacs(in + JS), s, d);
    st_jacs(out, s);
    st_jacs(out + JS, d);
})
OP_HD(jacs_dbl, JS, JS, st_jacs(out, dbl(ld_jacs(in))))
OP_HD(jacs_apply_phi, JS + SL, JS, st_jacs(out, apply_phi(ld_jacs(in), lds<1, DC>(in + JS))))
OP_HD(jacs_from_jacq, JQ, JS, st_jacs(out, jacs_from_jacq(ld_jacq(in))))
OP_HD(jacq_from_jacs, JS, JQ, st_jacq(out, jacq_from_jacs(ld_jacs(in))))

// curve29.hpp (verification, the table build)
OP_HD(jacq_add, 2 * JQ + 1, JQ, st_jacq(out, add(ld_jacq(in), ld_jacq(in + JQ), in[2 * JQ] != 0)))
OP_HD(jacq_add_mixed, JQ + AQ + 1, JQ, st_jacq(out, add_mixed(ld_jacq(in), ld_affq(in + JQ), in[JQ + AQ] != 0)))
OP_HD(jacq_dbl, JQ, JQ, st_jacq(out, dbl(ld_jacq(in))))
#undef OP_HD

// ---- device-only forms: COOP lanes per operation ---------------------------------------------------------------------------
#define OP_COOP(NAME, CO, IN_W, OUT_W, ...)                                           \
    struct op_##NAME {                                                                      \
        static constexpr int IN = IN_W, OUT = (CO) * (OUT_W), COOP = CO, FOLD = 0;     \
        static constexpr bool SIGNED = true;                                           \
        static __device__ void dev(const int32_t* in, int32_t* out, int sub) { __VA_ARGS__; } \
    };
#define OP_COOPQ(NAME, CO, IN_W, OUT_W, ...)                                          \
    struct op_##NAME {                                                                      \
        static constexpr int IN = IN_W, OUT = (CO) * (OUT_W), COOP = CO, FOLD = 0;     \
        static constexpr bool SIGNED = false;                                          \
        static __device__ void dev(const int32_t* in, int32_t* out, int sub) { __VA_ARGS__; } \
    };
OP_COOP(coop2_dbl_half, 2, JS, JS, st_jacs(out, coop2_dbl_half(ld_jacs(in), sub == 0)))
OP_COOP(coop2_add_mixed, 2, JS + AS + 1, JS, st_jacs(out, coop2_add_mixed(ld_jacs(in), ld_afft(in + JS), in[JS + AS] != 0, sub == 0)))
OP_COOP(coop4_dbl_half, 4, JS, JS, st_jacs(out, coop4_dbl_half(ld_jacs(in), sub)))
OP_COOP(coop4_dbl_half_phi, 4, JS + SL, JS + SL, {
    Fs<1, DC> bx;
    st_jacs(out, coop4_dbl_half_phi(ld_jacs(in), sub, lds<1, DC>(in + JS), bx));
    sts(out + JS, bx);
})
OP_COOP(coop4_add_mixed, 4, JS + AS + 1, JS, st_jacs(out, coop4_add_mixed(ld_jacs(in), ld_afft(in + JS), in[JS + AS] != 0, sub)))
OP_COOP(coop4_add, 4, 2 * JS + 1, JS, st_jacs(out, coop4_add(ld_jacs(in), ld_jacs(in + JS), in[2 * JS] != 0, sub)))
OP_COOP(coop4_add_sub, 4, 2 * JS, 2 * JS, {
    JacS s, d;
    coop4_add_sub(ld_jacs(in), ld_jacs(in + JS), sub, s, d);
    st_jacs(out, s);
    st_jacs(out + JS, d);
})
OP_COOPQ(q_coop_dbl, 4, JQ, JQ, st_jacq(out, coop_dbl(ld_jacq(in), sub)))
OP_COOPQ(q_coop_add_mixed, 4, JQ + AQ + 1, JQ, st_jacq(out, coop_add_mixed(ld_jacq(in), ld_affq(in + JQ), in[JQ + AQ] != 0, sub)))
OP_COOPQ(q_coop_add, 4, 2 * JQ + 1, JQ, st_jacq(out, coop_add(ld_jacq(in), ld_jacq(in + JQ), in[2 * JQ] != 0, sub)))
#undef OP_COOP
#undef OP_COOPQ

// ---- the tree folds: one block of NT threads per fold over 2 * SPAN partial sums (NT == 2 * SPAN at every call site) ----------
template <class Pt, int NT, int SPAN>
struct FoldOp {
    static_assert(NT == 2 * SPAN, "one partial sum per thread");
    static constexpr bool SIGNED = sizeof(Pt) == sizeof(JacS);
    static constexpr int PW = SIGNED ? JS : JQ;
    static constexpr int IN = 2 * SPAN * PW, OUT = PW, COOP = 0, FOLD = NT;
};
using op_fold30_64 = FoldOp<JacS, 64, 32>;     // k_g1_sum_positions (k_g1misc.hip)
using op_fold30_256 = FoldOp<JacS, 256, 128>;  // the circulant form's sums (k_g1circ.hip: CIRC_LANES / 2)
using op_fold29_64 = FoldOp<JacQ, 64, 32>;     // one wave: the two-round first level never runs
using op_fold29_128 = FoldOp<JacQ, 128, 64>;   // k_ps_buckets (PS_LANES / 2)
using op_fold29_256 = FoldOp<JacQ, 256, 128>;  // the bucket sums of verification (PIP_B / 2)

// ---- kernels ------------------------------------------------------------------------------------------------------------
template <class O>
__global__ __launch_bounds__(64) void k_test_op(const int32_t* __restrict__ in, int32_t* __restrict__ out, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    O::run(in + (size_t)i * O::IN, out + (size_t)i * O::OUT);
}
template <class O>
__global__ __launch_bounds__(64) void k_test_op_coop(const int32_t* __restrict__ in, int32_t* __restrict__ out, int n) {
    constexpr int C = O::COOP;
    const int op_of_thread = blockIdx.x * (64 / C) + (int)threadIdx.x / C, sub = (int)threadIdx.x % C;
    if (!O::SIGNED && op_of_thread >= n) return;  // whole groups leave (k_verify_many.hip)
    const bool keep = op_of_thread < n;           // padding lanes repeat the last operation and store nothing (k_slp_add_coop_s)
    const int op = keep ? op_of_thread : n - 1;
    int32_t r[O::OUT / C];
    O::dev(in + (size_t)op * O::IN, r, sub);
    if (keep) {
        int32_t* o = out + (size_t)op * O::OUT + (size_t)sub * (O::OUT / C);
        for (int k = 0; k < O::OUT / C; k++) o[k] = r[k];
    }
}
__device__ __forceinline__ JacS ld_pt(const int32_t* w, JacS*) { return ld_jacs(w); }
__device__ __forceinline__ JacQ ld_pt(const int32_t* w, JacQ*) { return ld_jacq(w); }
__device__ __forceinline__ void st_pt(int32_t* w, const JacS& p) { st_jacs(w, p); }
__device__ __forceinline__ void st_pt(int32_t* w, const JacQ& p) { st_jacq(w, p); }
__device__ __forceinline__ void fold(JacS* red, int first_span, int t, JacS*, std::integral_constant<int, 64>) { coop4_tree_fold<64>(red, first_span, t); }
__device__ __forceinline__ void fold(JacS* red, int first_span, int t, JacS*, std::integral_constant<int, 256>) { coop4_tree_fold<256>(red, first_span, t); }
template <int NT>
__device__ __forceinline__ void fold(JacQ* red, int first_span, int t, JacQ*, std::integral_constant<int, NT>) { coop_tree_fold<NT>(red, first_span, t); }
template <class Pt, int NT, int SPAN>
__global__ __launch_bounds__(NT) void k_test_fold(const int32_t* __restrict__ in, int32_t* __restrict__ out) {
    using O = FoldOp<Pt, NT, SPAN>;
    __shared__ Pt red[2 * SPAN];
    const int t = threadIdx.x;
    red[t] = ld_pt(in + ((size_t)blockIdx.x * 2 * SPAN + t) * O::PW, (Pt*)nullptr);
    fold(red, SPAN, t, (Pt*)nullptr, std::integral_constant<int, NT>{});
    if (t == 0) st_pt(out + (size_t)blockIdx.x * O::PW, red[0]);
}

// ---- the table ----------------------------------------------------------------------------------------------------------
#define TEST_OPS(X)                                                                                                           \
    X(fs_mul_cc) X(fs_mul_cc_du) X(fs_mul_cu) X(fs_mul_cu_du) X(fs_mul_cw) X(fs_mul_cw_du) X(fs_sqr) X(fs_sqr_du)              \
    X(fs_mul_inj_m1) X(fs_mul_inj_m1_wide) X(fs_sqr_inj_m2) X(fs_sqr_inj_m2_wide) X(fs_sqr_inj2) X(fs_sqr_inj2_wide)          \
    X(fs_mul_add_cccc) X(fs_mul_add_split) X(fs_half_of_triple) X(fs_normalise) X(fs_canonical) X(fs_canonical_of_product)    \
    X(fs_product_is_zero) X(fs_is_zero_slow) X(fs_neg_du) X(fs_neg_dw) X(fs_sub_lazy_du) X(fs_regroup_32_to_30)               \
    X(fs_regroup_30_to_32) X(fs_tabs_pack_unpack)                                                                             \
    X(fq_mul) X(fq_mul_wide) X(fq_sqr) X(fq_mul_add) X(fq_is_zero) X(fq_product_is_zero)                                      \
    X(fr_mul) X(fr_reduce_once) X(fr_partial_reduce) X(fr_add) X(fr_sub2r)                                                    \
    X(xyzz_add_mixed) X(xyzz_to_jacs) X(jacs_dbl_half) X(jacs_add_mixed) X(jacs_add) X(jacs_add_sub) X(jacs_dbl)              \
    X(jacs_apply_phi) X(jacs_from_jacq) X(jacq_from_jacs) X(jacq_add) X(jacq_add_mixed) X(jacq_dbl)                            \
    X(coop2_dbl_half) X(coop2_add_mixed) X(coop4_dbl_half) X(coop4_dbl_half_phi) X(coop4_add_mixed) X(coop4_add)              \
    X(coop4_add_sub) X(q_coop_dbl) X(q_coop_add_mixed) X(q_coop_add)                                                            \
    X(fold30_64) X(fold30_256) X(fold29_64) X(fold29_128) X(fold29_256)

struct OpInfo {
    const char* name;
    int in, out, coop, fold;
};
#define X_INFO(N) {#N, op_##N::IN, op_##N::OUT, op_##N::COOP, op_##N::FOLD},
static const OpInfo OPS[] = {TEST_OPS(X_INFO)};
#undef X_INFO
constexpr int N_OPS = sizeof(OPS) / sizeof(OPS[0]);

template <class O>
void launch_op(const int32_t* in, int32_t* out, int n, hipStream_t st) {
    if constexpr (O::FOLD != 0) {
        hipLaunchKernelGGL((k_test_fold<std::conditional_t<O::SIGNED, JacS, JacQ>, O::FOLD, O::FOLD / 2>), dim3(n), dim3(O::FOLD), 0, st,
                           in, out);
    } else if constexpr (O::COOP != 0) {
        const int per_wave = 64 / O::COOP;
        hipLaunchKernelGGL(k_test_op_coop<O>, dim3((n + per_wave - 1) / per_wave), dim3(64), 0, st, in, out, n);
    } else {
        hipLaunchKernelGGL(k_test_op<O>, dim3((n + 63) / 64), dim3(64), 0, st, in, out, n);
    }
}
template <class O>
int host_op(const int32_t* in, int32_t* out, int n) {
    if constexpr (O::FOLD != 0 || O::COOP != 0) {
        return -1;  // device-only form
    } else {
        for (int i = 0; i < n; i++) O::run(in + (size_t)i * O::IN, out + (size_t)i * O::OUT);
        return 0;
    }
}

}  // namespace testops

namespace launch {
int test_op_info(int op, int* in_words, int* out_words, int* device_only, const char** name) {
    if (op < 0 || op >= testops::N_OPS) return -1;
    const testops::OpInfo& o = testops::OPS[op];
    *in_words = o.in;
    *out_words = o.out;
    *device_only = (o.coop != 0 || o.fold != 0) ? 1 : 0;
    *name = o.name;
    return 0;
}
int test_op_host(int op, int n, const int32_t* in, int32_t* out) {
    int k = 0;
#define X_HOST(N) if (op == k++) return testops::host_op<testops::op_##N>(in, out, n);
    TEST_OPS(X_HOST)
#undef X_HOST
    return -1;
}
int test_op_device(int op, int n, const int32_t* d_in, int32_t* d_out, hipStream_t st) {
    int k = 0;
#define X_DEV(N) if (op == k++) { testops::launch_op<testops::op_##N>(d_in, d_out, n, st); return 0; }
    TEST_OPS(X_DEV)
#undef X_DEV
    return -1;
}
}  // namespace launch
}  // namespace kzg
