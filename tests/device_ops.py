"""Exact references and cases for the per-operation test kernels of csrc/k_test_ops.hip (tests/test_device_ops.py).

Operands travel as the raw words of the device structs, so a case can hold any digit pattern its type admits: canonical digits,
every digit at its class bound with aligned signs, values at +-B p, zero written as a multiple of p where the type allows it.
Results are decoded with Python integers and checked two ways: the VALUE (a field element's residue; a point projectively equal to
the plain affine group law below, or the identity) and the BOUND its type declares (later operations rely on it, and a correct
value can still violate it).  The word counts per operation come from the library (eth_kzg_amd_test_op_info), not from here.
"""
import ctypes as C
import random

import numpy as np

import synth

P = synth.P  # BLS12-381 base field
R_ORDER = synth.R  # scalar field
RS, RQ, RR = 1 << 390, 1 << 406, 1 << 261  # Montgomery radices: fp30.hpp, fp29.hpp, fr29.hpp
SHALF = 1 << 29
DC, DU, DW = 1, 2, 3
DC_MAX, DW_MAX = SHALF + 4, (1 << 30) + 8
GX = 0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB
GY = 0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1
G = (GX, GY)
INV_RS, INV_RQ = pow(RS, -1, P), pow(RQ, -1, P)
INV_RR = pow(RR, -1, R_ORDER)


# ---- reference group law: affine points over Python integers, None = identity ------------------------------------------------
def on_curve(a):
    return a is None or (a[1] * a[1] - a[0] ** 3 - 4) % P == 0


def g_neg(a):
    return None if a is None else (a[0], (-a[1]) % P)


def g_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def g_mul(a, k):
    r = None
    for bit in bin(k % R_ORDER)[2:] if k % R_ORDER else "":
        r = g_add(r, r)
        if bit == "1":
            r = g_add(r, a)
    return r


def compress(a):
    """48-byte ZCash encoding (the oracle's and the ABI's)."""
    if a is None:
        return b"\xc0" + bytes(47)
    b = bytearray(a[0].to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if a[1] > (P - 1) // 2 else 0)
    return bytes(b)


# ---- digit forms --------------------------------------------------------------------------------------------------------------
def fs_value(d):
    return sum(int(x) << (30 * i) for i, x in enumerate(d))


def fs_digits(v, cls):
    """exact digits of v: floor digits (DU) or centred digits in [-2^29, 2^29) (DC, DW); the top digit takes the rest"""
    d = []
    for _ in range(12):
        lo = v & ((1 << 30) - 1)
        if cls != DU and lo >= SHALF:
            lo -= 1 << 30
        d.append(lo)
        v = (v - lo) >> 30
    d.append(v)
    assert -(1 << 31) <= v < (1 << 31)
    return d


def fs_extreme(B, cls, pattern, top_sign):
    """digits 0..11 at their class bound with the signs of `pattern` (+1 / -1 per digit), the top digit the largest of sign
    top_sign that keeps |value| <= B p"""
    mag = {DC: DC_MAX, DW: DW_MAX, DU: (1 << 30) - 1}[cls]
    d = [(mag if s > 0 else (0 if cls == DU else -mag)) for s in pattern]
    low = fs_value(d + [0])
    if top_sign > 0:
        t = (B * P - low) >> 360
    else:
        t = -((B * P + low) >> 360)
    v = low + (t << 360)
    assert abs(v) <= B * P
    return d + [t]


def fq_limbs(v):
    """normalised 29-bit limbs (limbs 0..12 < 2^29, limb 13 the rest) of 0 <= v"""
    d = [(v >> (29 * i)) & ((1 << 29) - 1) for i in range(13)]
    d.append(v >> (29 * 13))
    assert d[13] < (1 << 32)
    return d


def fq_value(d):
    return sum((int(x) & 0xFFFFFFFF) << (29 * i) for i, x in enumerate(d))


def fr_limbs(v):
    d = [(v >> (29 * i)) & ((1 << 29) - 1) for i in range(8)]
    d.append(v >> (29 * 8))
    assert d[8] < (1 << 32)
    return d


fr_value = fq_value


# ---- types: words <-> values, bounds --------------------------------------------------------------------------------------------
class Fs:
    """Fs<B, F> of fp30.hpp; exact = the digits a fresh product leaves (centred in [-2^29, 2^29) or floor)"""
    words = 13

    def __init__(self, B, cls, exact=False):
        self.B, self.cls, self.exact = B, cls, exact

    def value(self, w):
        return fs_value(w)

    def residue(self, w):
        return fs_value(w) * INV_RS % P

    def bound_error(self, w):
        v = fs_value(w)
        if abs(v) > self.B * P:
            return f"|value| = {abs(v) / P:.3f} p > {self.B} p"
        for i in range(12):
            d = w[i]
            if self.cls == DU:
                ok = 0 <= d < (1 << 30)
            elif self.exact:
                ok = -SHALF <= d < SHALF
            elif self.cls == DC:
                ok = -DC_MAX <= d <= DC_MAX
            else:
                ok = -DW_MAX <= d <= DW_MAX
            if not ok:
                return f"digit {i} = {d} outside class {self.cls}{' (exact)' if self.exact else ''}"
        return None


class Fq:
    """Fq<B> of fp29.hpp: normalised limbs, 0 <= value < B p"""
    words = 14

    def __init__(self, B):
        self.B = B

    def value(self, w):
        return fq_value(w)

    def residue(self, w):
        return fq_value(w) * INV_RQ % P

    def bound_error(self, w):
        if any((x & 0xFFFFFFFF) >= (1 << 29) for x in w[:13]):
            return "limb not normalised"
        if fq_value(w) >= self.B * P:
            return f"value >= {self.B} p"
        return None


class Fr:
    """Fr29 of fr29.hpp: value < B r; normalised limbs unless lazy"""
    words = 9

    def __init__(self, B, lazy=False):
        self.B, self.lazy = B, lazy

    def value(self, w):
        return fr_value(w)

    def residue(self, w):
        return fr_value(w) * INV_RR % R_ORDER

    def bound_error(self, w):
        if not self.lazy and any((x & 0xFFFFFFFF) >= (1 << 29) for x in w[:8]):
            return "limb not normalised"
        if fr_value(w) >= self.B * R_ORDER:
            return f"value >= {self.B} r"
        return None


class Flag:
    words = 1

    def bound_error(self, w):
        return None if w[0] in (0, 1) else f"flag {w[0]}"


class Raw:
    """plain words (the 32-bit side of a regrouping): an integer"""

    def __init__(self, n):
        self.words = n

    def value(self, w):
        return sum((int(x) & 0xFFFFFFFF) << (32 * i) for i, x in enumerate(w))

    def bound_error(self, w):
        return None


class Point:
    """a point struct: its coordinates' types, how to read the affine point, how the identity is told"""

    def __init__(self, kind, coords):
        self.kind, self.coords = kind, coords
        self.words = sum(c.words for c in coords)

    def split(self, w):
        out, k = [], 0
        for c in self.coords:
            out.append(w[k:k + c.words])
            k += c.words
        return out

    def affine(self, w):
        parts = self.split(w)
        r = [c.residue(x) for c, x in zip(self.coords, parts)]
        if self.kind in ("affs", "affq"):
            return None if all(v == 0 for x in parts for v in x) else (r[0], r[1])
        if self.kind == "afft":
            return (r[0], r[1])
        if self.kind == "xyzz":
            x, y, zz, zzz = r
            if zz == 0:
                return None
            return x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P
        x, y, z = r  # Jacobian
        if z == 0:
            return None
        zi = pow(z, -1, P)
        return x * zi * zi % P, y * zi * zi * zi % P

    def bound_error(self, w):
        parts = self.split(w)
        for name, c, x in zip("xyzw", self.coords, parts):
            e = c.bound_error(x)
            if e:
                return f"{name}: {e}"
        if self.kind == "xyzz":  # the identity must be recognisable by product_is_zero(zz) (thirteen ORs)
            zz = parts[2]
            if self.coords[2].residue(zz) == 0 and any(zz):
                return "zz == 0 mod p but not written as 0"
            if self.coords[2].residue(zz) != 0:
                r = [c.residue(x) for c, x in zip(self.coords, parts)]
                if r[2] ** 3 % P != r[3] ** 2 % P:
                    return "zz^3 != zzz^2"
        return None


JACS = Point("jacs", [Fs(4, DC), Fs(1, DC), Fs(1, DC)])
JACS_OUT = Point("jacs", [Fs(4, DC), Fs(1, DC), Fs(1, DC)])
XYZZ = Point("xyzz", [Fs(4, DU), Fs(1, DU), Fs(1, DU), Fs(1, DU)])
AFFS = Point("affs", [Fs(1, DC, exact=True), Fs(1, DC, exact=True)])
AFFT = Point("afft", [Fs(1, DC, exact=True), Fs(1, DC, exact=True)])
JACQ = Point("jacq", [Fq(64), Fq(64), Fq(4)])
AFFQ = Point("affq", [Fq(1), Fq(1)])
FLAG = Flag()


# ---- encoders of points ------------------------------------------------------------------------------------------------------
def _rep(res, R, B, rng, extreme=False, signed=True):
    """a representative of the Montgomery form of residue `res` with |v| <= B p (v >= 0 when not signed)"""
    m = res * R % P
    lo = -((B * P + m) // P) if signed else 0
    hi = (B * P - m) // P
    if signed and B == 1:  # |v| < p: the value a fresh product holds
        lo, hi = (-1 if m else 0), 0
    if extreme:
        k = rng.choice([lo, hi])
    else:
        k = rng.randint(lo, hi)
    v = m + k * P
    if signed and B == 1 and abs(v) >= P:
        v = m
    return v


def enc_jacs(a, rng, extreme=False, ident="one"):
    if a is None:
        x = fs_digits(_rep(1, RS, 1, rng), DC) if ident == "one" else fs_digits(_rep(rng.randrange(P), RS, 4, rng), DC)
        y = fs_digits(_rep(1, RS, 1, rng), DC) if ident == "one" else fs_digits(_rep(rng.randrange(P), RS, 1, rng), DC)
        zv = {"one": 0, "junk": 0, "p": P, "-p": -P}[ident]
        return x + y + fs_digits(zv, DC)
    z = rng.randrange(1, P)
    X, Y = a[0] * z * z % P, a[1] * z * z * z % P
    return (fs_digits(_rep(X, RS, 4, rng, extreme), DC) + fs_digits(_rep(Y, RS, 1, rng, extreme), DC)
            + fs_digits(_rep(z, RS, 1, rng, extreme), DC))


def enc_xyzz(a, rng, extreme=False):
    if a is None:
        return [0] * 52
    z = rng.randrange(1, P)
    zz, zzz = z * z % P, z * z * z % P
    X, Y = a[0] * zz % P, a[1] * zzz % P
    return (fs_digits(_rep(X, RS, 4, rng, extreme), DU) + fs_digits(_rep(Y, RS, 1, rng, extreme), DU)
            + fs_digits(_rep(zz, RS, 1, rng, extreme), DU) + fs_digits(_rep(zzz, RS, 1, rng, extreme), DU))


def enc_affs(a):
    if a is None:
        return [0] * 26
    return fs_digits(a[0] * RS % P, DC) + fs_digits(a[1] * RS % P, DC)


def enc_afft(a, rng):  # fresh products: |v| < p, exact centred digits
    return fs_digits(_rep(a[0], RS, 1, rng), DC) + fs_digits(_rep(a[1], RS, 1, rng), DC)


def enc_jacq(a, rng, extreme=False, zmul=0):
    if a is None:
        one = fq_limbs(RQ % P)
        return one + one + fq_limbs(zmul * P)
    z = rng.randrange(1, P)
    X, Y = a[0] * z * z % P, a[1] * z * z * z % P
    return (fq_limbs(_rep(X, RQ, 64, rng, extreme, signed=False)) + fq_limbs(_rep(Y, RQ, 64, rng, extreme, signed=False))
            + fq_limbs(_rep(z, RQ, 4, rng, extreme, signed=False)))


def enc_affq(a):
    if a is None:
        return [0] * 28
    return fq_limbs(a[0] * RQ % P) + fq_limbs(a[1] * RQ % P)


# ---- operations: operand types, result types, reference ---------------------------------------------------------------------
def _f(fn):
    return lambda *r: [fn(*r) % P]


SPEC = {
    # name: (operand types, result types, reference on residues -> expected residues / points / integers)
    "fs_mul_cc": ([Fs(16, DC), Fs(16, DC)], [Fs(1, DC, True)], _f(lambda a, b: a * b)),
    "fs_mul_cc_du": ([Fs(16, DC), Fs(16, DC)], [Fs(1, DU, True)], _f(lambda a, b: a * b)),
    "fs_mul_cu": ([Fs(4, DC), Fs(64, DU)], [Fs(1, DC, True)], _f(lambda a, b: a * b)),
    "fs_mul_cu_du": ([Fs(4, DC), Fs(64, DU)], [Fs(1, DU, True)], _f(lambda a, b: a * b)),
    "fs_mul_cw": ([Fs(4, DC), Fs(64, DW)], [Fs(1, DC, True)], _f(lambda a, b: a * b)),
    "fs_mul_cw_du": ([Fs(4, DC), Fs(64, DW)], [Fs(1, DU, True)], _f(lambda a, b: a * b)),
    "fs_sqr": ([Fs(16, DC)], [Fs(1, DC, True)], _f(lambda a: a * a)),
    "fs_sqr_du": ([Fs(16, DC)], [Fs(1, DU, True)], _f(lambda a: a * a)),
    "fs_mul_inj_m1": ([Fs(1, DC), Fs(1, DU), Fs(4, DU)], [Fs(5, DC)], _f(lambda a, b, x: a * b - x)),
    "fs_mul_inj_m1_wide": ([Fs(4, DC), Fs(64, DW), Fs(32, DW)], [Fs(33, DC)], _f(lambda a, b, x: a * b - x)),
    "fs_sqr_inj_m2": ([Fs(2, DC), Fs(1, DC)], [Fs(3, DC)], _f(lambda a, x: a * a - 2 * x)),
    "fs_sqr_inj_m2_wide": ([Fs(16, DC), Fs(32, DW)], [Fs(65, DC)], _f(lambda a, x: a * a - 2 * x)),
    "fs_sqr_inj2": ([Fs(5, DC), Fs(1, DC), Fs(1, DU)], [Fs(4, DU)], _f(lambda a, x, y: a * a - x - 2 * y)),
    "fs_sqr_inj2_wide": ([Fs(16, DC), Fs(32, DW), Fs(32, DU)], [Fs(97, DC)], _f(lambda a, x, y: a * a - x - 2 * y)),
    "fs_mul_add_cccc": ([Fs(11, DC)] * 4, [Fs(1, DC, True)], _f(lambda a, b, c, d: a * b + c * d)),
    "fs_mul_add_split": ([Fs(4, DC), Fs(32, DW), Fs(32, DW), Fs(4, DC)], [Fs(1, DU, True)], _f(lambda a, b, c, d: a * b + c * d)),
    "fs_half_of_triple": ([Fs(1, DC, True)], [Fs(2, DC)], _f(lambda a: 3 * a * pow(2, -1, P))),
    "fs_normalise": ([Fs(64, DW)], [Fs(64, DC)], _f(lambda a: a)),
    "fs_canonical": ([Fs(64, DW)], [Fs(1, DU, True)], _f(lambda a: a)),
    "fs_canonical_of_product": ([Fs(1, DU, True)], [Fs(1, DU, True)], _f(lambda a: a)),
    "fs_product_is_zero": ([Fs(1, DC, True)], [FLAG], lambda a: [int(a == 0)]),
    "fs_is_zero_slow": ([Fs(64, DW)], [FLAG], lambda a: [int(a == 0)]),
    "fs_neg_du": ([Fs(64, DU)], [Fs(64, DW)], _f(lambda a: -a)),
    "fs_neg_dw": ([Fs(64, DW)], [Fs(64, DW)], _f(lambda a: -a)),
    "fs_sub_lazy_du": ([Fs(32, DU), Fs(32, DU)], [Fs(64, DW)], _f(lambda a, b: a - b)),
    "fs_regroup_32_to_30": ([Raw(12)], [Fs(1 << 8, DU)], None),
    "fs_regroup_30_to_32": ([Fs(1 << 8, DU)], [Raw(12)], None),
    "fs_tabs_pack_unpack": ([Fs(1, DU, True), Fs(1, DU, True)], [Raw(24), Fs(1, DC, True), Fs(1, DC, True)], None),
    "fq_mul": ([Fq(64), Fq(64)], [Fq(2)], _f(lambda a, b: a * b)),
    "fq_mul_wide": ([Fq(4096), Fq(4096)], [Fq(2)], _f(lambda a, b: a * b)),
    "fq_sqr": ([Fq(4096)], [Fq(2)], _f(lambda a: a * a)),
    "fq_mul_add": ([Fq(2048), Fq(4096), Fq(2048), Fq(4096)], [Fq(2)], _f(lambda a, b, c, d: a * b + c * d)),
    "fq_is_zero": ([Fq(8)], [FLAG], lambda a: [int(a == 0)]),
    "fq_product_is_zero": ([Fq(2)], [FLAG], lambda a: [int(a == 0)]),
    "fr_mul": ([Fr(56, lazy=True), Fr(2)], [Fr(2)], lambda a, b: [a * b % R_ORDER]),
    "fr_reduce_once": ([Fr(2)], [Fr(1)], None),
    "fr_partial_reduce": ([Fr(56, lazy=True)], [Fr(2)], None),
    "fr_add": ([Fr(28), Fr(28)], [Fr(56, lazy=False)], None),
    "fr_sub2r": ([Fr(54), Fr(2)], [Fr(56)], None),
    "xyzz_add_mixed": ([XYZZ, AFFS, FLAG], [XYZZ], lambda p, q, n: [g_add(p, g_neg(q) if n else q)]),
    "xyzz_to_jacs": ([XYZZ], [JACS_OUT], lambda p: [p]),
    "jacs_dbl_half": ([JACS], [JACS_OUT], lambda p: [g_add(p, p)]),
    "jacs_add_mixed": ([JACS, AFFT, FLAG], [JACS_OUT], lambda p, q, n: [g_add(p, g_neg(q) if n else q)]),
    "jacs_add": ([JACS, JACS, FLAG], [JACS_OUT], lambda p, q, n: [g_add(p, g_neg(q) if n else q)]),
    "jacs_add_sub": ([JACS, JACS], [JACS_OUT, JACS_OUT], lambda p, q: [g_add(p, q), g_add(p, g_neg(q))]),
    "jacs_dbl": ([JACS], [JACS_OUT], lambda p: [g_add(p, p)]),
    "jacs_apply_phi": ([JACS, Fs(1, DC, True)], [JACS_OUT], None),
    "jacs_from_jacq": ([JACQ], [JACS_OUT], lambda p: [p]),
    "jacq_from_jacs": ([JACS], [JACQ], lambda p: [p]),
    "jacq_add": ([JACQ, JACQ, FLAG], [JACQ], lambda p, q, n: [g_add(p, g_neg(q) if n else q)]),
    "jacq_add_mixed": ([JACQ, AFFQ, FLAG], [JACQ], lambda p, q, n: [g_add(p, g_neg(q) if n else q)]),
    "jacq_dbl": ([JACQ], [JACQ], lambda p: [g_add(p, p)]),
}
# the device-only forms: the same operation as their one-lane counterpart, COOP copies of the result
COOP = {
    "coop2_dbl_half": ("jacs_dbl_half", 2), "coop2_add_mixed": ("jacs_add_mixed", 2), "coop4_dbl_half": ("jacs_dbl_half", 4),
    "coop4_dbl_half_phi": (None, 4), "coop4_add_mixed": ("jacs_add_mixed", 4), "coop4_add": ("jacs_add", 4),
    "coop4_add_sub": ("jacs_add_sub", 4), "q_coop_dbl": ("jacq_dbl", 4), "q_coop_add_mixed": ("jacq_add_mixed", 4),
    "q_coop_add": ("jacq_add", 4),
}
FOLDS = {"fold30_64": (JACS, 64), "fold30_256": (JACS, 256), "fold29_64": (JACQ, 64), "fold29_128": (JACQ, 128),
         "fold29_256": (JACQ, 256)}
# the signed-field pair / quad forms take negq wave-uniform (k_slp_mulc_coop_s, k_slp_add_coop_s: one recoded digit / flag word per wave)
SIGNED_COOP = {"coop2_dbl_half", "coop2_add_mixed", "coop4_dbl_half", "coop4_dbl_half_phi", "coop4_add_mixed", "coop4_add", "coop4_add_sub"}
BETA = pow(2, (P - 1) // 3, P)  # a primitive cube root of unity in Fp
assert BETA != 1 and pow(BETA, 3, P) == 1


# ---- the library's table ----------------------------------------------------------------------------------------------------
def op_table(lib):
    """name -> (op index, input words, output words, device only), as the library states it"""
    t, op = {}, 0
    i, o, d, nm = C.c_int32(), C.c_int32(), C.c_int32(), C.c_char_p()
    while lib.eth_kzg_amd_test_op_info(op, C.byref(i), C.byref(o), C.byref(d), C.byref(nm)) == 0:
        t[nm.value.decode()] = (op, i.value, o.value, bool(d.value))
        op += 1
    return t


def run(lib, table, name, cases, handle=None, on_device=False):
    """cases: list of input word lists -> array [n, out_words] of int32"""
    op, iw, ow, _ = table[name]
    a = np.array(cases, dtype=np.int64)
    assert a.shape == (len(cases), iw), (name, a.shape, iw)
    a = np.ascontiguousarray((a & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
    out = np.zeros((len(cases), ow), dtype=np.int32)
    rc = lib.eth_kzg_amd_test_op(handle, op, len(cases), a.ctypes.data, out.ctypes.data, int(on_device))
    assert rc == 0, (name, rc)
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------
def _field_pool(t, rng):
    """encodings of one operand of type t: random, 0, 1, p - 1, zero as a multiple of p, values near +-B p, worst digits"""
    out = []
    if isinstance(t, Fs):
        exact_only = t.exact
        B = 1 if exact_only else t.B
        enc_cls = t.cls
        for res in [0, 1, P - 1, 2, (P - 1) // 2]:
            out.append(fs_digits(_rep(res, RS, B, rng, extreme=False), enc_cls))
            if not exact_only:
                out.append(fs_digits(_rep(res, RS, B, rng, extreme=True), enc_cls))
        if not exact_only:
            for k in sorted({1, B // 2, B}):  # zero written as +-k p
                if k >= 1:
                    out += [fs_digits(k * P, enc_cls), fs_digits(-k * P, enc_cls)]
            out += [fs_digits(B * P, enc_cls), fs_digits(-B * P, enc_cls)]
            for pat in range(8):  # worst-case digit patterns, signs aligned / alternating
                sgn = [(-1 if pat & 1 else 1) * ((-1) ** i if pat & 4 else 1) for i in range(12)]
                out.append(fs_extreme(B, enc_cls, sgn, -1 if pat & 2 else 1))
        else:
            out += [fs_digits(-1, enc_cls), fs_digits(1, enc_cls), fs_digits(P - 1, enc_cls), fs_digits(-(P - 1), enc_cls)]
        for _ in range(6):
            out.append(fs_digits(_rep(rng.randrange(P), RS, B, rng), enc_cls))
        return [d for d in out if t.bound_error(d) is None]
    if isinstance(t, Fq):
        for res in [0, 1, P - 1, 2]:
            out.append(fq_limbs(_rep(res, RQ, t.B, rng, signed=False)))
            out.append(fq_limbs(_rep(res, RQ, t.B, rng, extreme=True, signed=False)))
        out += [fq_limbs(k * P) for k in sorted({0, 1, t.B - 1})]
        top = (t.B * P - 1) >> (29 * 13)
        out.append([(1 << 29) - 1] * 13 + [top if fq_value([(1 << 29) - 1] * 13 + [top]) < t.B * P else top - 1])
        out.append(fq_limbs(t.B * P - 1))
        for _ in range(6):
            out.append(fq_limbs(_rep(rng.randrange(P), RQ, t.B, rng, signed=False)))
        return [d for d in out if t.bound_error(d) is None]
    if isinstance(t, Fr):
        vals = [0, 1, R_ORDER - 1, R_ORDER, t.B * R_ORDER - 1, (t.B - 1) * R_ORDER, rng.randrange(t.B * R_ORDER)]
        vals += [rng.randrange(R_ORDER) for _ in range(4)]
        out = [fr_limbs(v) for v in vals]
        if t.lazy:  # carries left where they are (LAZY LIMBS, fr29.hpp): limbs up to 2^31 with the same value
            for v in vals[2:]:
                d = fr_limbs(v)
                for i in range(7, -1, -1):
                    if d[i + 1] >= 2 and d[i] + (1 << 29) < (1 << 31):
                        d[i + 1] -= 1
                        d[i] += 1 << 29
                out.append(d)
        return [d for d in out if t.bound_error(d) is None and fr_value(d) < RR]
    if isinstance(t, Raw):
        return [[0] * t.words, [0xFFFFFFFF] * t.words, [rng.getrandbits(32) for _ in range(t.words)]]
    raise TypeError(t)


def field_cases(name, rng, n_random=48):
    ins = SPEC[name][0]
    if name == "fs_regroup_32_to_30":
        return [[rng.getrandbits(32) for _ in range(12)] for _ in range(n_random)] + [[0] * 12, [0xFFFFFFFF] * 12]
    if name == "fs_regroup_30_to_32":  # non-negative floor digits, value < 2^384
        c = [fs_digits(rng.randrange(1 << 384), DU) for _ in range(n_random)]
        return c + [fs_digits(0, DU), fs_digits((1 << 384) - 1, DU), fs_digits(P - 1, DU)]
    if name == "fs_tabs_pack_unpack":
        vals = [0, 1, P - 1, (1 << 380) - 1] + [rng.randrange(P) for _ in range(n_random)]
        return [fs_digits(a, DU) + fs_digits(b, DU) for a, b in zip(vals, reversed(vals))]
    if name == "fs_canonical_of_product":
        vals = [0, 1, -1, P - 1, -(P - 1), (P - 1) // 2, -(P - 1) // 2] + [rng.randrange(-P + 1, P) for _ in range(n_random)]
        return [fs_digits(v, DU) for v in vals]
    if name == "fr_reduce_once":
        vals = [0, 1, R_ORDER - 1, R_ORDER, R_ORDER + 1, 2 * R_ORDER - 1] + [rng.randrange(2 * R_ORDER) for _ in range(n_random)]
        return [fr_limbs(v) for v in vals]
    if name == "fr_sub2r":  # a - b + 2 r: b < 2 r normalised (a fresh product)
        a = [0, 1, 54 * R_ORDER - 1] + [rng.randrange(54 * R_ORDER) for _ in range(n_random)]
        b = [0, 2 * R_ORDER - 1, R_ORDER] + [rng.randrange(2 * R_ORDER) for _ in range(n_random)]
        return [fr_limbs(x) + fr_limbs(y) for x in a[:3] for y in b[:3]] + [fr_limbs(x) + fr_limbs(y) for x, y in zip(a, b)]
    if name == "fr_mul":  # entry: a < 32 r times a product < 2 r; after 12 layers: a < 56 r times a canonical twiddle
        pa32 = [d for d in _field_pool(Fr(32, lazy=True), rng)]
        pa56 = [d for d in _field_pool(Fr(56, lazy=True), rng)]
        pb2 = _field_pool(Fr(2), rng)
        pb1 = _field_pool(Fr(1), rng)
        cases = [x + y for x in pa32 for y in pb2[:6]] + [x + y for x in pa56 for y in pb1[:6]]
        return cases
    pools = [_field_pool(t, rng) for t in ins]
    cases = []
    # every special operand against random partners, then random combinations
    for k, pool in enumerate(pools):
        for d in pool:
            cases.append([w for j, p in enumerate(pools) for w in (d if j == k else rng.choice(pools[j][-6:]))])
    # worst patterns together (all operands at their extremes)
    for _ in range(n_random):
        cases.append([w for p in pools for w in rng.choice(p)])
    if name in ("fr_add",):
        cases = [c for c in cases if fr_value(c[:9]) + fr_value(c[9:]) < RR]
    return cases


def _points(rng, n):
    pts = []
    for _ in range(n):
        pts.append(g_mul(G, rng.randrange(1, R_ORDER)))
    return pts


POINT_POOL_SEED = 4242


def point_cases(name, rng, pts):
    """(cases, references) for a point operation: generic, P + P and P - P under different Z, identities in every encoding,
    negq both ways, coordinates at the extremes of their bounds"""
    ins = SPEC[name][0]
    cases = []
    kinds = [t.kind if isinstance(t, Point) else ("flag" if t is FLAG else "fs") for t in ins]

    def enc(kind, a, extreme, ident):
        if kind == "jacs":
            return enc_jacs(a, rng, extreme, ident)
        if kind == "xyzz":
            return enc_xyzz(a, rng, extreme)
        if kind == "affs":
            return enc_affs(a)
        if kind == "afft":
            return enc_afft(a, rng)
        if kind == "jacq":
            return enc_jacq(a, rng, extreme, {"one": 0, "junk": 1, "p": 2, "-p": 3}[ident])
        if kind == "affq":
            return enc_affq(a)
        raise TypeError(kind)

    idents = ["one", "junk", "p", "-p"]
    n_pts = [k for k in kinds if k != "flag" and k != "fs"]
    combos = []  # (points, negq)
    P0, Q0 = pts[0], pts[1]
    if len(n_pts) == 1:
        for a in pts[:8]:
            combos.append(([a], 0))
        combos.append(([None], 0))
    else:
        for i in range(6):
            combos += [([pts[i], pts[i + 1]], 0), ([pts[i], pts[i + 1]], 1)]
        combos += [([P0, P0], 0), ([P0, P0], 1), ([P0, g_neg(P0)], 0), ([P0, g_neg(P0)], 1), ([Q0, Q0], 0), ([Q0, g_neg(Q0)], 1)]
        if n_pts[0] != "afft" and n_pts[1] != "afft":
            combos += [([None, Q0], 0), ([None, Q0], 1), ([None, None], 0), ([None, None], 1)]
        else:
            combos += [([None, Q0], 0), ([None, Q0], 1)]
        if n_pts[1] != "afft":  # a table point of the constant multiplication is never the identity
            combos += [([P0, None], 0), ([P0, None], 1)]
    refs = []
    for pts_, negq in combos:
        for extreme in (False, True):
            for ident in (idents if any(p is None for p in pts_) else ["one"]):
                if "xyzz" in kinds and ident != "one":
                    continue  # the MSM's accumulator has one identity: all zero (xyzz30_inf, the slow path)
                words, it = [], iter(pts_)
                vals = []
                for k, t in zip(kinds, ins):
                    if k == "flag":
                        words.append(negq)
                        vals.append(negq)
                    elif k == "fs":
                        words += fs_digits(BETA * RS % P, DC)
                        vals.append(BETA)
                    else:
                        a = next(it)
                        if k == "afft" and a is None:
                            a = Q0
                        words += enc(k, a, extreme, ident)
                        vals.append(a)
                cases.append(words)
                refs.append(vals)
    return cases, refs


# ---- checks -----------------------------------------------------------------------------------------------------------------
def _split(types, w):
    out, k = [], 0
    for t in types:
        out.append(list(int(x) for x in w[k:k + t.words]))
        k += t.words
    return out


def _decode_in(t, w):
    if isinstance(t, Point):
        return t.affine(w)
    if t is FLAG:
        return w[0]
    if isinstance(t, Raw):
        return t.value(w)
    return t.residue(w)


def check(name, case, result, ref_vals=None):
    """None, or what is wrong with `result` (the output words of op `name` on input words `case`)"""
    ins, outs, ref = SPEC[name]
    iw = _split(ins, case)
    ow = _split(outs, result)
    for k, (t, w) in enumerate(zip(outs, ow)):
        e = t.bound_error(w)
        if e:
            return f"result {k}: bound: {e}"
    if name == "fs_regroup_32_to_30":
        return None if fs_value(ow[0]) == Raw(12).value(iw[0]) else "value"
    if name == "fs_regroup_30_to_32":
        return None if Raw(12).value(ow[0]) == fs_value(iw[0]) else "value"
    if name == "fs_tabs_pack_unpack":
        for k in range(2):
            if fs_value(ow[1 + k]) != fs_value(iw[k]):
                return f"coordinate {k}: unpacked {fs_value(ow[1 + k])} != packed {fs_value(iw[k])}"
            d = fs_digits(fs_value(iw[k]), DC)  # word i: centred digit i's low 30 bits | two bits of the top digit
            want = [(d[i] & ((1 << 30) - 1)) | (((d[12] >> (2 * i)) & 3) << 30) for i in range(12)]
            if [x & 0xFFFFFFFF for x in ow[0][12 * k:12 * k + 12]] != want:
                return f"coordinate {k}: packed words"
        return None
    if name in ("fs_canonical", "fs_canonical_of_product"):
        v = fs_value(ow[0])
        return None if 0 <= v < P and (v - fs_value(iw[0])) % P == 0 else f"not the canonical representative: {v}"
    if name == "fr_reduce_once":
        v, a = fr_value(ow[0]), fr_value(iw[0])
        return None if v == a % R_ORDER else f"{v} != {a} mod r"
    if name == "fr_partial_reduce":
        v, a = fr_value(ow[0]), fr_value(iw[0])
        return None if (v - a) % R_ORDER == 0 and v < 2 * R_ORDER else f"{v} vs {a}"
    if name == "fr_add":
        return None if fr_value(ow[0]) == fr_value(iw[0]) + fr_value(iw[1]) else "sum"
    if name == "fr_sub2r":
        return None if fr_value(ow[0]) == fr_value(iw[0]) - fr_value(iw[1]) + 2 * R_ORDER else "difference"
    if name == "jacs_apply_phi":
        a = JACS.affine(iw[0])
        want = None if a is None else (a[0] * BETA % P, a[1])
        got = JACS_OUT.affine(ow[0])
        return None if got == want else f"phi: {got} != {want}"
    vals = ref_vals if ref_vals is not None else [_decode_in(t, w) for t, w in zip(ins, iw)]
    want = ref(*vals)
    for k, (t, w, e) in enumerate(zip(outs, ow, want)):
        got = _decode_in(t, w)
        if isinstance(t, Point):
            if got is not None and not on_curve(got):
                return f"result {k}: not on the curve"
        if got != e:
            return f"result {k}: {got} != {e}"
    return None


# ---- the device-only forms ----------------------------------------------------------------------------------------------------
def coop_cases(name, rng, pts):
    """cases in wave layouts: every wave mixes regular operations with exceptional ones at its first, a middle and its last
    position; n is not a multiple of the operations per wave; negq wave-uniform for the signed-field forms"""
    base, co = COOP[name]
    per_wave = 64 // co
    if name == "coop4_dbl_half_phi":
        regular = [enc_jacs(a, rng) for a in pts[:8]]
        special = [enc_jacs(None, rng, ident=i) for i in ("one", "junk", "p", "-p")] + [enc_jacs(pts[0], rng, True)]
        beta = fs_digits(BETA * RS % P, DC)
        regular = [c + beta for c in regular]
        special = [c + beta for c in special]
    else:
        bc, _ = point_cases(base, rng, pts)
        ins = SPEC[base][0]
        regular, special = [], []
        for c in bc:
            vals = [_decode_in(t, w) for t, w in zip(ins, _split(ins, c))]
            pv = [v for v, t in zip(vals, ins) if isinstance(t, Point)]
            exceptional = any(v is None for v in pv) or (len(pv) == 2 and pv[1] is not None and pv[0] is not None and pv[0][0] == pv[1][0])
            (special if exceptional else regular).append(c)
    flag_at = None
    ins = SPEC[base][0] if base else []
    if ins and ins[-1] is FLAG:
        flag_at = sum(t.words for t in ins) - 1
    n_waves = 3
    n = n_waves * per_wave - (per_wave // 2 + 1)  # the last wave is partly padding
    cases = []
    for wv in range(n_waves):
        negq = wv & 1
        for pos in range(per_wave):
            i = wv * per_wave + pos
            if i >= n:
                break
            at_edge = pos in (0, per_wave // 2, per_wave - 1) or i == n - 1
            src = special if (at_edge or rng.random() < 0.2) and special else regular
            c = list(rng.choice(src))
            if flag_at is not None and name in SIGNED_COOP:
                c[flag_at] = negq
            cases.append(c)
    return cases


def fold_cases(name, rng, pts):
    """folds of 2 * span partial sums: random points, identities and equal partial sums at each level of the tree"""
    pt, nt = FOLDS[name]
    enc = (lambda a, ident="one": enc_jacs(a, rng, ident=ident)) if pt is JACS else \
        (lambda a, ident="one": enc_jacq(a, rng, zmul={"one": 0, "junk": 1, "p": 2, "-p": 3}[ident]))
    folds = []
    folds.append([rng.choice(pts) for _ in range(nt)])                     # random
    folds.append([None] * nt)                                              # all identities
    folds.append([pts[0]] * nt)                                            # equal partial sums at every level
    f = [rng.choice(pts) for _ in range(nt // 2)]
    folds.append(f + [g_neg(a) for a in f])                                # opposite points at the first level: all identities after it
    folds.append([pts[1] if (i % 4) < 2 else None for i in range(nt)])     # identities next to equal sums
    f = [rng.choice(pts + [None]) for _ in range(nt // 4)]
    folds.append(f + f + [g_neg(a) for a in f] + f)                        # equal sums at the second level, opposite at the first
    cases, refs = [], []
    for pts_ in folds:
        words = []
        for a in pts_:
            words += enc(a, rng.choice(["one", "junk", "p", "-p"]) if a is None else "one")
        cases.append(words)
        tot = None
        for a in pts_:
            tot = g_add(tot, a)
        refs.append(tot)
    return cases, refs


# ---- GLV window tables: layout (csrc/launch.hpp), packed entries (curve30.hpp: TabS), the audit predicate -----------------------
# A table of nominal width c: W = ceil(128 / c) windows of mixed widths covering the 128-bit half exactly; two blocks per group (the
# lower ceil(W / 2) windows, the upper rest); inside a block [window][base][digit]; entry (base i, digit d) of a window of `bits`
# bits at (i << (bits - 1)) + d - 1, 1 <= d <= 2^(bits - 1); 24 words per entry.  The entry is d 2^lo(w) B.
def glv_windows(c):
    return (128 + c - 1) // c


def glv_lower_windows(c):
    return (glv_windows(c) + 1) // 2


def glv_window_bits(c, w):
    W = glv_windows(c)
    b = 128 // W
    return b + (1 if w < 128 - W * b else 0)


def glv_window_lo(c, w):
    return sum(glv_window_bits(c, k) for k in range(w))


def glv_entries_per_base(c, w0=0, w1=None):
    return sum(1 << (glv_window_bits(c, w) - 1) for w in range(w0, glv_windows(c) if w1 is None else w1))


def glv_table_entries(c, n_groups, nb):
    return n_groups * nb * glv_entries_per_base(c)


def glv_entry_index(c, nb, group, w, i, d):
    """position (in entries) of entry (group, w, i, d) in a table whose blocks lie one after the other"""
    WL = glv_lower_windows(c)
    per_group = glv_entries_per_base(c) * nb
    lower = glv_entries_per_base(c, 0, WL) * nb
    upper = w >= WL
    in_block = glv_entries_per_base(c, WL if upper else 0, w) * nb + (i << (glv_window_bits(c, w) - 1)) + d - 1
    return group * per_group + (lower if upper else 0) + in_block


def tabs_pack_value(v):
    """12 words of an integer 0 <= v < 2^384 (the coordinate's Montgomery-390 value when it is canonical): word i = centred digit i's
    low 30 bits | bits 2 i, 2 i + 1 of the top digit"""
    d = fs_digits(v, DC)
    assert 0 <= d[12] < (1 << 24), "not packable"
    return [(d[i] & ((1 << 30) - 1)) | (((d[12] >> (2 * i)) & 3) << 30) for i in range(12)]


def tabs_unpack_value(w):
    """the integer 12 stored words stand for, whatever they hold"""
    top, v = 0, 0
    for i in range(12):
        x = int(w[i]) & 0xFFFFFFFF
        lo = x & 0x3FFFFFFF
        if lo >= SHALF:
            lo -= 1 << 30
        v += lo << (30 * i)
        top |= (x >> 30) << (2 * i)
    return v + (top << 360)


def tabs_pack(a):
    """the 24 words tabs_pack_from_fq stores for the affine point a (None: the all-zero entry of an identity row)"""
    if a is None:
        return [0] * 24
    return tabs_pack_value(a[0] * RS % P) + tabs_pack_value(a[1] * RS % P)


def tabs_point(w):
    """the affine point an entry holds (None: all zero), read without any check"""
    if not any(int(x) for x in w):
        return None
    return tabs_unpack_value(w[:12]) * INV_RS % P, tabs_unpack_value(w[12:24]) * INV_RS % P


def g1affine_words(a):
    """G1Affine of curve.hpp: x, y as 12 little-endian words each of the Montgomery form x 2^384 mod p; the identity is all zero"""
    if a is None:
        return [0] * 24
    out = []
    for v in a:
        m = v * (1 << 384) % P
        out += [(m >> (32 * i)) & 0xFFFFFFFF for i in range(12)]
    return out


A_ENCODING, A_OFF_CURVE, A_STEP, A_LINK, A_ZERO, A_NONZERO_IDENTITY, A_ANCHOR = 1, 2, 4, 8, 16, 32, 64


def _collinear(a, b, c):
    """a + b == c for three affine points with a != +-b, by the line through a, b and -c and three different x"""
    if a is None or b is None or c is None or len({a[0], b[0], c[0]}) != 3:
        return False
    return ((b[1] - a[1]) * (c[0] - a[0]) + (c[1] + a[1]) * (b[0] - a[0])) % P == 0


def _tangent(a, c):
    """2 a == c by the tangent in a through -c"""
    if a is None or c is None or a[0] == c[0] or a[1] == 0:
        return False
    return ((c[1] + a[1]) * 2 * a[1] + 3 * a[0] * a[0] * (c[0] - a[0])) % P == 0


def audit_row(row, bits_prev, prev_first, base, identity_row=False):
    """The audit predicate (csrc/table_audit.hpp) over one row in plain integers: row = the 24 words of d = 1 .. T; prev_first = the
    stored words of the first entry of the window below (None for window 0, where `base` -- the affine base -- anchors the row);
    bits_prev = that window's width.  Returns {d: reasons}.  The words of a coordinate and the integer they stand for determine
    each other (twelve 30-bit digits and a 24-bit top digit), so the encoding is the canonical one exactly when 0 <= value < p."""
    out = {}
    vals = [(tabs_unpack_value(w[:12]), tabs_unpack_value(w[12:24])) if any(int(x) for x in w) else None for w in row]
    pts = [None if v is None else (v[0] * INV_RS % P, v[1] * INV_RS % P) for v in vals]
    head_ok = None
    for k in range(len(row)):
        d, r, me = k + 1, 0, pts[k]
        if identity_row:
            if me is not None:
                out[d] = A_NONZERO_IDENTITY
            continue
        if me is None:
            out[d] = A_ZERO
            continue
        if not (0 <= vals[k][0] < P and 0 <= vals[k][1] < P):
            r |= A_ENCODING
        if (me[1] * me[1] - me[0] * me[0] * me[0] - 4) % P:
            r |= A_OFF_CURVE
        if d == 1:
            if prev_first is None:
                if me != base:
                    r |= A_ANCHOR
            else:
                q = tabs_point(prev_first)
                for _ in range(bits_prev):
                    q = g_add(q, q)
                if q is None or q != me:
                    r |= A_LINK
        elif d == 2:
            if not _tangent(pts[0], me):
                r |= A_STEP
        elif not _collinear(pts[k - 1], pts[0], me):
            if head_ok is None:
                head_ok = _tangent(pts[0], pts[1])
            if head_ok:  # a broken head is reported by d = 1, 2 themselves
                r |= A_STEP
        if r:
            out[d] = r
    return out


def row_multiples_error(row, q):
    """None, or the first d whose entry is not d q (q = 2^lo B, affine): the direct statement, by d - 1 additions (Jacobian, compared
    by cross-multiplication: no inversion per entry; d = 2 is the doubling)"""
    X, Y, Z = q[0], q[1], 1
    qx, qy = q
    for k, w in enumerate(row):
        if k == 1:
            X, Y = g_add(q, q)
        elif k:
            # (X, Y, Z) + q, mixed addition in plain integers (madd-2007-bl); d q != +-q for d < r, so H != 0
            zz = Z * Z % P
            h = (qx * zz - X) % P
            rr = 2 * (qy * Z * zz - Y) % P
            if h == 0:
                return k + 1
            i = 4 * h * h % P
            j = h * i % P
            v = X * i % P
            X3 = (rr * rr - j - 2 * v) % P
            Y = (rr * (v - X3) - 2 * Y * j) % P
            Z = 2 * Z * h % P
            X = X3
        me = tabs_point(w)
        zz = Z * Z % P
        if me is None or (me[0] * zz - X) % P or (me[1] * zz * Z - Y) % P:
            return k + 1
    return None
