// Exact audit of a GLV window table (libc_eth_kzg_hooks.so only; tests/test_table_audit.py): ONE routine, compiled for the device and
// for the host, that decides for an entry (group, window, base, d) of a table in the layout of launch.hpp / k_table.hip / k_msm_glv.inc
// whether it is what the row's induction needs:
//   encoding   the 24 words are the unique packing of a canonical coordinate pair (unpack, canonicalise, repack == stored words);
//   on curve   y^2 = x^3 + 4;
//   step       T[d] = T[d-1] + T[1], decided WITHOUT an adder: T[d-1], T[1] and -T[d] are collinear and have three different x
//              (d = 2: -T[2] lies on the tangent in T[1], x differs, y(T[1]) != 0).  A line meets the curve in three points that sum
//              to the identity, so with the three on the curve the relation holds exactly -- and cannot hold by a degenerate accident;
//   link       the first entry of window w > 0 is 2^bits(w-1) times the first entry of window w - 1 (dbl of curve30.hpp, pinned to exact
//              integers by tests/test_device_ops.py; compared by cross-multiplication);
//   anchor     the first entry of window 0 is the base itself;
//   identity   a row of an identity base is all zero words; a zero entry anywhere else is a finding.
// By induction a row without findings is exactly d 2^lo(w) B for every d.  Every entry is visited by exactly one call, which counts
// itself; findings (group, window, base, d, reasons) go to a small buffer, first come first kept, the total is counted.
//
// A step that fails BECAUSE the row's head is broken (T[1] zero, or T[2] != 2 T[1]: the entries d = 1, 2 report that themselves) is
// not reported again at every d >= 3 of the row: a wrong first entry shows at d = 1, 2 and at the link of the window after it, not
// as 32768 findings.  Zero findings still mean that every relation holds: a silent d >= 3 implies the head relation was evaluated and
// held, or that d = 2 has reported it.
#pragma once
#include "curve30.hpp"
#include "launch.hpp"

namespace kzg {
namespace audit {

constexpr int R_ENCODING = 1, R_OFF_CURVE = 2, R_STEP = 4, R_LINK = 8, R_ZERO = 16, R_NONZERO_IDENTITY = 32, R_ANCHOR = 64;
constexpr int FINDING_WORDS = 5;  // group, window, base, d, reasons

struct Out {
    unsigned long long visited;
    unsigned int n_findings, max_findings;
    int32_t* findings;  // [max_findings][FINDING_WORDS]
};
HD void count_visit(Out* o) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicAdd(&o->visited, 1ull);
#else
    o->visited++;
#endif
}
HD void report(Out* o, int group, int w, int base, int d, int reasons) {
#ifdef __HIP_DEVICE_COMPILE__
    const unsigned int k = atomicAdd(&o->n_findings, 1u);
#else
    const unsigned int k = o->n_findings++;
#endif
    if (k >= o->max_findings) return;
    int32_t* f = o->findings + (size_t)k * FINDING_WORDS;
    f[0] = group; f[1] = w; f[2] = base; f[3] = d; f[4] = reasons;
}

// an entry as stored, and its coordinates as the representatives in [0, p) (floor digits: equal residues <=> equal digits)
struct Entry {
    uint32_t w[24];
    Fs<1, DU> x, y;
    bool zero;
};
// what 12 words unpack to, whatever they hold: twelve sign-extended 30-bit digits and a 24-bit top digit: |value| < 2^384 < 16 p
HD Fs<16, DC> raw_coord(const uint32_t* w) {
    const Fs<1, DC> u = tabs_unpack_coord(w);
    Fs<16, DC> r;
    for (int i = 0; i < SL; i++) r.v[i] = u.v[i];
    return r;
}
HD Entry load_entry(const TabS* p) {
    Entry e;
    uint32_t any = 0;
    for (int i = 0; i < 24; i++) { e.w[i] = p->w[i]; any |= e.w[i]; }
    e.zero = any == 0;
    e.x = canonical(raw_coord(e.w));
    e.y = canonical(raw_coord(e.w + 12));
    return e;
}
HD bool same(const Fs<1, DU>& a, const Fs<1, DU>& b) {
    int32_t d = 0;
    for (int i = 0; i < SL; i++) d |= a.v[i] ^ b.v[i];
    return d == 0;
}
HD bool encoding_ok(const Entry& e) {
    uint32_t w[24];
    tabs_pack_coord(w, e.x);
    tabs_pack_coord(w + 12, e.y);
    uint32_t d = 0;
    for (int i = 0; i < 24; i++) d |= w[i] ^ e.w[i];
    return d == 0;
}
HD bool on_curve(const Entry& e) {
    const Fs<1, DC> x = normalise(e.x), y = normalise(e.y);
    const Fs<1, DC> x3 = mul(sqr(x), x), y2 = sqr(y);
    const Fs<4, DC> four = mul_small<2>(mul_small<2>(fs_one()));
    return is_zero_slow(sub(add(x3, four), y2));
}
// c == a + b for entries a != b of one row (chord), by collinearity of a, b, -c:  (yb - ya)(xc - xa) + (yc + ya)(xb - xa) == 0
HD bool chord_ok(const Entry& a, const Entry& b, const Entry& c) {
    if (a.zero || b.zero || c.zero) return false;
    if (same(a.x, b.x) || same(a.x, c.x) || same(b.x, c.x)) return false;
    const Fs<1, DC> ya = normalise(a.y);
    const auto dy_ba = sub(b.y, a.y), dx_ca = sub(c.x, a.x), dx_ba = sub(b.x, a.x);
    const auto sy_ca = add(ya, c.y);
    return product_is_zero(mul_add(dy_ba, dx_ca, sy_ca, dx_ba));
}
// c == 2 a (tangent in a through -c):  (yc + ya) 2 ya + 3 xa^2 (xc - xa) == 0
HD bool tangent_ok(const Entry& a, const Entry& c) {
    if (a.zero || c.zero) return false;
    if (same(a.x, c.x) || product_is_zero(a.y)) return false;
    const Fs<1, DC> xa = normalise(a.x), ya = normalise(a.y);
    const auto slope_n = mul_small<3>(sqr(xa));
    const auto slope_d = mul_small<2>(ya);
    return product_is_zero(mul_add(add(ya, c.y), slope_d, slope_n, sub(c.x, a.x)));
}
// e == 2^k a, by k doublings and cross-multiplication
HD bool link_ok(const Entry& a, int k, const Entry& e) {
    if (a.zero || e.zero) return false;
    AffS s;
    s.x = mul(fs_one(), a.x);
    s.y = mul(fs_one(), a.y);
    JacS j = to_jacs(s);
    for (int i = 0; i < k; i++) j = dbl(j);
    if (is_zero_slow(j.z)) return false;
    const Fs<1, DC> zz = sqr(j.z), zzz = mul(zz, j.z);
    return is_zero_slow(sub(j.x, mul(zz, e.x))) && is_zero_slow(sub(j.y, mul(zzz, e.y)));
}
HD bool anchor_ok(const G1Affine& b, const Entry& e) {
    return same(canonical_of_product(fs_from_fp<DU>(b.x)), e.x) && same(canonical_of_product(fs_from_fp<DU>(b.y)), e.y);
}

// where an entry lives: blocks[2 group + upper], inside a block [window][base][digit] (k_table.hip)
HD const TabS* entry_ptr(const void* const* blocks, int c, int nb, int group, int w, int i, int d) {
    const int WL = launch::glv_lower_windows(c), upper = w >= WL ? 1 : 0;
    const size_t T = (size_t)1 << (launch::glv_window_bits(c, w) - 1);
    const size_t in_block = launch::glv_entries_per_base(c, upper ? WL : 0, w) * (size_t)nb + (size_t)i * T + (size_t)(d - 1);
    return reinterpret_cast<const TabS*>(blocks[2 * group + upper]) + in_block;
}

// Entry number e of the table, in the table's own order [group][window][base][digit].  blocks: the pointer array of the groups
// [0, n_groups) audited; bases: their n_groups x nb bases.
HD void audit_entry(const void* const* blocks, const G1Affine* bases, int c, int nb, unsigned long long e, Out* out) {
    const int W = launch::glv_windows(c);
    const unsigned long long per_group = (unsigned long long)launch::glv_entries_per_base(c, 0, W) * nb;
    const int group = (int)(e / per_group);
    unsigned long long rem = e % per_group;
    int w = 0;
    for (; w < W; w++) {
        const unsigned long long in_w = ((unsigned long long)nb) << (launch::glv_window_bits(c, w) - 1);
        if (rem < in_w) break;
        rem -= in_w;
    }
    const int bits = launch::glv_window_bits(c, w);
    const int i = (int)(rem >> (bits - 1)), d = (int)(rem & (((unsigned long long)1 << (bits - 1)) - 1)) + 1;
    const Entry me = load_entry(entry_ptr(blocks, c, nb, group, w, i, d));
    count_visit(out);
    int reasons = 0;
    if (is_inf(bases[(size_t)group * nb + i])) {
        if (!me.zero) reasons |= R_NONZERO_IDENTITY;
    } else if (me.zero) {
        reasons |= R_ZERO;
    } else {
        if (!encoding_ok(me)) reasons |= R_ENCODING;
        if (!on_curve(me)) reasons |= R_OFF_CURVE;
        if (d == 1) {
            if (w == 0) {
                if (!anchor_ok(bases[(size_t)group * nb + i], me)) reasons |= R_ANCHOR;
            } else if (!link_ok(load_entry(entry_ptr(blocks, c, nb, group, w - 1, i, 1)), launch::glv_window_bits(c, w - 1), me)) {
                reasons |= R_LINK;
            }
        } else {
            const Entry first = load_entry(entry_ptr(blocks, c, nb, group, w, i, 1));
            if (d == 2) {
                if (!tangent_ok(first, me)) reasons |= R_STEP;
            } else if (!chord_ok(load_entry(entry_ptr(blocks, c, nb, group, w, i, d - 1)), first, me)) {
                // the head of the row (see the top of the file): d = 1, 2 report a broken one themselves
                if (tangent_ok(first, load_entry(entry_ptr(blocks, c, nb, group, w, i, 2)))) reasons |= R_STEP;
            }
        }
    }
    if (reasons) report(out, group, w, i, d, reasons);
}

}  // namespace audit
}  // namespace kzg
