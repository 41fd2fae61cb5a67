"""The fixed-base MSM kernels (csrc/k_msm_glv.inc) on a setup whose bases collide: the setup, the planned scalars, a model of the
kernels' schedules that says which additions of a case are degenerate, and the closed-form reference.  No GPU is used here;
tests/test_fixed_msm_cases.py asserts the model's statements, tests/test_gpu_fixed_msm.py runs the cases.

THE SETUP.  All 4096 G1 points are the generator G (the G2 points are mainnet's: the verifier's set-up looks at nothing else).  FK20
vector i is then [G] * 63 + [identity] * 65 for every i, so all 64 bases of FK20 group j are ONE point B_j = c_j G with
c_j = sum_{k < 63} omega^(j k) (never zero), and every base of the commitment table is G.  Table entry (window w, base i, digit d) of a
group is d 2^lo(w) B whatever i is: which gathered additions meet equal or opposite operands is integer arithmetic on window digits.

THE MODEL works on discrete logarithms in units of the group's base B: integers mod r, a k2 sum multiplied by lambda where the kernel
applies phi.  For a case (64 pairs of signed halves), a nominal table width and a kernel it replays the additions in the order the
kernel source states them and names each one: `plain`, `acc identity`, `operand identity`, `both identity`, `equal` (the doubling
path), `opposite` (the sum is the identity).  It describes the test's INPUTS -- that a case reaches the path it was built for -- and is
no reference: the expected sum of a group is (sum_i k1_i + lambda k2_i mod r) c_j G, one multiplication by plain double-and-add."""
import functools
import json
import os
import random

import device_ops as D
import oracle_lib
import setup_material as sm

R = D.R_ORDER
LAMBDA = 0xAC45A4010001A40200000000FFFFFFFF  # phi(x, y) = (beta x, y) = [LAMBDA](x, y) on G1 (csrc/glv.hpp); LAMBDA^2 + LAMBDA + 1 = r
assert (LAMBDA * LAMBDA + LAMBDA + 1) % R == 0
G_BYTES = D.compress(D.G)
IDENTITY = D.compress(None)
WIDTHS = (16, 15, 8)
KERNELS = ("chunked", "windowed1", "windowed2", "flat256", "flat128")
MODE_OF = {"flat": 0, "windowed1": 1, "windowed2": 3, "chunked": 2}  # what launch::msm_glv calls them
EVENT_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fixed_msm_events.json")
NB = 64


# ---- the colliding setup ------------------------------------------------------------------------------------------------------
def colliding_setup():
    return G_BYTES * sm.N_G1, sm.mainnet_points()[1]


OMEGA_128 = pow(sm.OMEGA_4096, 32, R)


@functools.lru_cache(maxsize=None)
def c_fk20(j):
    """B_j = c_j G: output j of the 128-point transform of [G] * 63 + [identity] * 65."""
    return sum(pow(OMEGA_128, j * k, R) for k in range(63)) % R


def base_factor(kind, group):
    return c_fk20(group) if kind == 0 else 1


def groups_of(kind):
    return 128 if kind == 0 else 64


_MUL = {}


def times_g(k):
    k %= R
    if k not in _MUL:
        _MUL[k] = oracle_lib.g1_mul(G_BYTES, k.to_bytes(32, "big")) if k else IDENTITY
    return _MUL[k]


def commitment_layout(k):
    """(group, base) of coefficient k in the commitment's launch: launch_msm(d_canon_, TAB_SRS, ..., 64 groups, ...) reads
    scalars[slice][group][base] = coefficient 64 group + base, and the table's bases are the setup's points in that order."""
    return k // NB, k % NB


# ---- scalars: the balanced split, halves as the kernels read them ----------------------------------------------------------
def split_balanced(k):
    """glv_split_balanced of csrc/glv.hpp on a canonical scalar: signed (k1, k2) with k = k1 + k2 lambda mod r."""
    k2, k1 = divmod(k, LAMBDA)
    if k1 > (LAMBDA - 1) // 2:
        k1, k2 = k1 - LAMBDA, k2 + 1
    if k2 > (LAMBDA + 1) // 2:
        k1, k2 = k1 - 1, k2 - (LAMBDA + 1)
    return k1, k2


def join(k1, k2):
    return (k1 + k2 * LAMBDA) % R


def half_bytes(v, minus_zero=False):
    """16 bytes = 4 little-endian words: the magnitude (< 2^127) with the sign in bit 127."""
    assert abs(v) < 1 << 127
    return (abs(v) | ((1 << 127) if v < 0 or (v == 0 and minus_zero) else 0)).to_bytes(16, "little")


def windows(c):
    """(lowest bit, bits) of the W = ceil(128 / c) windows of a table of nominal width c (csrc/launch.hpp)."""
    return [(D.glv_window_lo(c, w), D.glv_window_bits(c, w)) for w in range(D.glv_windows(c))]


def booth(mag, c):
    """The signed digit of every window of a magnitude: the window's bits and the bit below it (booth_mem, and the shift registers
    of the chunked kernels)."""
    out = []
    for lo, bits in windows(c):
        x = (((mag >> lo) & ((1 << bits) - 1)) << 1) | ((mag >> (lo - 1)) & 1 if lo else 0)
        out.append(((x + 1) >> 1) - ((1 << bits) if x >> bits else 0))
    assert sum(d << lo for d, (lo, _) in zip(out, windows(c))) == mag
    return out


class Case:
    def __init__(self, name, halves, minus_zero=False, why=""):
        self.name, self.why, self.minus_zero = name, why, minus_zero
        self.halves = list(halves) + [(0, 0)] * (NB - len(halves))
        assert len(self.halves) == NB

    def total(self):
        return sum(k1 + LAMBDA * k2 for k1, k2 in self.halves) % R

    def presplit(self):
        return b"".join(half_bytes(k1, self.minus_zero) + half_bytes(k2, self.minus_zero) for k1, k2 in self.halves)

    def canonical(self):
        assert not self.minus_zero, "minus zero exists in the split form only"
        return b"".join(join(k1, k2).to_bytes(32, "big") for k1, k2 in self.halves)

    def round_trips(self):
        return all(split_balanced(join(k1, k2)) == (k1, k2) for k1, k2 in self.halves)


def at(pairs):
    """{base: (k1, k2)} -> 64 pairs"""
    return [pairs.get(i, (0, 0)) for i in range(NB)]


def _trunc(v, bits):
    return (abs(v) >> bits << bits) * (-1 if v < 0 else 1)


def _rand_halves(rng, n=NB):
    return [split_balanced(rng.randrange(R)) for _ in range(n)]


def cases(c, seed=20):
    """The planned cases on a table of nominal width c, as halves.  A case is the same idea at every width; where a window boundary
    enters, the values follow the width's windows."""
    rng = random.Random(seed)
    win = windows(c)
    W, WL = len(win), (len(win) + 1) // 2
    lo = [l for l, _ in win]
    b0 = win[0][1]
    top = 3 << lo[WL - 1]  # digit 3 in the last window of the lower part
    X = 1 << lo[WL]        # digit 1 in the first window of the upper part
    third = LAMBDA // 3
    thirds = (third, third + 1, LAMBDA - 2 * third - 1)  # three different values below (lambda - 1) / 2 with sum lambda
    a, b = split_balanced(rng.randrange(R))
    out = [
        # chains
        Case("chain equal", at({0: (5, 0), 1: (5, 0)}), why="two consecutive bases with the same digit"),
        Case("chain equal after prefix", at({0: (1, 0), 1: (2, 0), 2: (3, 0)}), why="a projective accumulator meets an equal entry"),
        Case("chain opposite then restart", at({0: (7, 0), 1: (-7, 0), 2: (9, 0)}), why="the accumulator restarts from the identity mid-chain"),
        Case("chain equal last", at({62: (top, 0), 63: (top, 0)}), why="equal at the lane's last step: the prefetch has wrapped to base 0"),
        Case("chain opposite last", at({62: (top, 0), 63: (-top, 0)}), why="opposite at the lane's last step"),
        Case("all scalars equal", [(a, b)] * NB, why="a collision candidate at every step"),
        Case("booth carry", at({0: (1 << (b0 - 1), 0), 1: (1 << (b0 - 1), 0)}),
             why="the second negative top digit meets the positive partial sum the carry left (chunked), or the first one (windowed)"),
        Case("second half of the bases", at({40: (5, 0), 41: (5, 0), 45: (0, 6), 46: (0, -6)}), why="part 1 of the two-lane kernel"),
        Case("bases 31 and 32", at({31: (5, 0), 32: (5, 0)}), why="a chain collision a lane per window sees and two lanes per window do not"),
        # folds
        Case("k1 parts equal", at({0: (X, 0), 1: (X // 4 + 1, 0), 2: (X // 4 - 1, 0), 3: (X // 4 + 2, 0), 4: (X // 4 - 2, 0)}), why="c0 = c1"),
        Case("k1 parts opposite", at({0: (-X, 0), 1: (X // 4 + 1, 0), 2: (X // 4 - 1, 0), 3: (X // 4 + 2, 0), 4: (X // 4 - 2, 0)}), why="c0 = -c1"),
        Case("k2 parts equal", at({0: (0, X), 1: (0, X // 4 + 1), 2: (0, X // 4 - 1), 3: (0, X // 4 + 2), 4: (0, X // 4 - 2)}), why="c2 = c3, before phi"),
        Case("k2 parts opposite", at({0: (0, -X), 1: (0, X // 4 + 1), 2: (0, X // 4 - 1), 3: (0, X // 4 + 2), 4: (0, X // 4 - 2)}), why="c2 = -c3"),
    ]
    for wa in (0, 1, 3):  # the sums of windows wa and wa + 1 are the same point: spans 1, 2 and 4 of the windowed tree
        q = 1 << (win[wa][1] - 2)
        vals = {0: q + 1, 1: q - 1, 2: q + 2, 3: q - 2}
        for sign, word in ((1, "equal"), (-1, "opposite")):
            pairs = {i: (v << lo[wa], 0) for i, v in vals.items()}
            pairs[4] = (sign << lo[wa + 1], 0)
            out.append(Case("windows %d and %d %s" % (wa, wa + 1, word), at(pairs), why="neighbouring window sums, across the %d -> %d-bit boundary" % (win[wa][1], win[wa + 1][1])))
    out += [
        Case("bases 3 and 35 equal", at({3: (a, b), 35: (a, b)}), why="the flat fold below its first level"),
        Case("bases 3 and 35 opposite", at({3: (a, b), 35: (-a, -b)}), why="the flat fold below its first level"),
        Case("k1 sum is lambda times k2 sum", at({0: (thirds[0], 1), 1: (thirds[1], 0), 2: (thirds[2], 0)}), why="the addition of the k1 sum and phi(k2 sum) doubles"),
        Case("k1 sum is minus lambda times k2 sum", at({0: (thirds[0], -1), 1: (thirds[1], 0), 2: (thirds[2], 0)}), why="... gives the identity"),
    ]
    if W & (W - 1):  # the tree's last addition takes the sums behind the largest power of two: k2's top windows (nine windows: 7 and 8)
        cut = 1
        while cut * 2 < 2 * W:
            cut *= 2
        hi = 1 << lo[cut - W]
        for sign, word in ((1, "equal"), (-1, "opposite")):
            out.append(Case("last tree addition %s" % word,
                            at({0: (sign * thirds[0], hi), 1: (sign * thirds[1], sign * (hi // 2 - 1)), 2: (sign * thirds[2], sign * (hi // 4)), 3: (0, sign * (hi // 4))}),
                            why="k1 sum + lambda (k2 below window %d) = +-lambda (k2 from window %d)" % (cut - W, cut - W)))
    out += [
        # identities where real data has none
        Case("one base only", at({17: (a, b)}), why="every other term is skipped"),
        Case("k2 only", [(0, k2) for _, k2 in _rand_halves(rng)], why="the k1 lanes fold identities"),
        Case("upper windows only", [(_trunc(k1, lo[WL]), _trunc(k2, lo[WL])) for k1, k2 in _rand_halves(rng)], why="the lower parts fold identities"),
        Case("minus zero", at({17: (a, b)}), minus_zero=True, why="a set sign bit on a zero half is skipped like zero (split form only)"),
    ]
    assert len({x.name for x in out}) == len(out)
    return out


# ---- the schedules ------------------------------------------------------------------------------------------------------------
def _chain_event(acc, entry, step):
    assert entry % R
    if acc % R == 0:
        return "acc identity"
    if (acc - entry) % R == 0:
        return "equal"
    if (acc + entry) % R == 0:
        return "opposite"
    return "plain"


def _fold_event(x, y):
    x, y = x % R, y % R
    if x == 0 and y == 0:
        return "both identity"
    if x == 0:
        return "acc identity"
    if y == 0:
        return "operand identity"
    if x == y:
        return "equal"
    if (x + y) % R == 0:
        return "opposite"
    return "plain"


def _chain(terms, events, lane):
    """terms: the lane's loop, one entry value (0: the digit is zero, no addition) per iteration.  Place: `chain first` = the second
    addition made (step 1), `chain last` = the loop's last iteration, `chain` between; an accumulator that is the identity again
    after the first addition is `chain restart`."""
    acc, made = 0, 0
    for e, t in enumerate(terms):
        if t == 0:
            continue
        ev = _chain_event(acc, t, made)
        if made:
            place = "chain restart" if ev == "acc identity" else "chain last" if e == len(terms) - 1 else "chain first" if made == 1 else "chain"
            events.append((ev, place, lane))
        acc += t
        made += 1
    return acc


def model(case, c, kernel):
    """[(event, place, where)] of every addition behind a lane's first one, and the sum (in units of the base)."""
    win = windows(c)
    W, WL = len(win), (len(win) + 1) // 2
    dig = [[booth(abs(h), c) for h in pair] for pair in case.halves]  # dig[i][half][w]
    sgn = [[-1 if h < 0 else 1 for h in pair] for pair in case.halves]
    term = lambda i, half, w: sgn[i][half] * dig[i][half][w] * (1 << win[w][0])  # the entry's value, sign applied
    events = []
    if kernel == "chunked":  # wave = (half, part): per lane base-major, the windows of its part inside
        csum = []
        for chunk in range(4):
            half, ws = chunk >> 1, range(WL, W) if chunk & 1 else range(WL)
            csum.append(_chain([term(i, half, w) for i in range(NB) for w in ws], events, "chunk %d" % chunk))
        events.append((_fold_event(csum[0], csum[1]), "fold k1", ""))
        events.append((_fold_event(csum[2], csum[3]), "fold k2", ""))
        s, t = csum[0] + csum[1], (csum[2] + csum[3]) * LAMBDA
        events.append((_fold_event(s, t), "fold phi", ""))
        total = s + t
    elif kernel in ("windowed1", "windowed2"):  # lane = (part, joint window): its bases in order, phi per lane, then the span tree
        split = int(kernel[-1])
        U = 2 * W * split
        red = []
        for u in range(U):
            part, uw = divmod(u, 2 * W)
            half, w = (1, uw - W) if uw >= W else (0, uw)
            i0 = part * (NB // split)
            s = _chain([term(i, half, w) for i in range(i0, i0 + NB // split)], events, "lane %d" % u)
            red.append(s * LAMBDA if half else s)
        span = 1
        while span < U:
            for uu in range(0, U, 2 * span):
                if uu + span < U:
                    events.append((_fold_event(red[uu], red[uu + span]), "tree span %d" % span, "%d" % uu))
                    red[uu] += red[uu + span]
            span *= 2
        total = red[0]
    else:  # flat: lane l of a half takes e = l, l + HL, ... (e = 64 window + base), phi per lane, fold from span HL down
        HL = int(kernel[4:]) // 2
        red = [0] * (2 * HL)
        for half in range(2):
            for l in range(HL):
                mine = []
                s = _chain([term(e % NB, half, e // NB) for e in range(l, W * NB, HL)], mine, "lane %d" % (half * HL + l))
                # a lane adds windows of ONE base in rising order: what it holds is below half the next entry, never plus or minus it
                assert all(ev == "plain" for ev, _, _ in mine), (case.name, c, kernel, mine)
                red[half * HL + l] = s * LAMBDA if half else s
        span = HL
        while span >= 1:
            for x in range(span):
                ev = _fold_event(red[x], red[x + span])
                events.append((ev, "fold phi" if span == HL else "fold span %d" % span, "%d" % x))
                red[x] += red[x + span]
            span //= 2
        total = red[0]
    assert total % R == case.total(), (case.name, c, kernel)
    return events, total % R


def reached(c, kernel, case_list=None):
    """{(event, place): [case names]} of the degenerate additions the cases reach in a kernel."""
    out = {}
    for case in case_list or cases(c):
        for ev, place, _ in model(case, c, kernel)[0]:
            if ev != "plain":
                out.setdefault((ev, place), [])
                if case.name not in out[(ev, place)]:
                    out[(ev, place)].append(case.name)
    return out


def required_events():
    """The committed table: [width, kernel, event, place, a case that reaches it]."""
    return [tuple(row) for row in json.load(open(EVENT_TABLE))["events"]]


def unreachable():
    return json.load(open(EVENT_TABLE))["not_reachable"]


# ---- inputs of a launch and their expected bytes -----------------------------------------------------------------------------
def slice_bytes(case, form, n_groups):
    """the case in every group of one slice"""
    return (case.presplit() if form == 1 else case.canonical()) * n_groups


class RandomSlices:
    """A small pool of seeded random slices (every group with scalars of its own), in both forms, and their sums."""

    def __init__(self, n_groups, seed, n=3):
        rng = random.Random(seed)
        self.n_groups = n_groups
        self.halves = [[_rand_halves(rng) for _ in range(n_groups)] for _ in range(n)]
        self.bytes = {1: [b"".join(half_bytes(k1) + half_bytes(k2) for g in s for k1, k2 in g) for s in self.halves],
                      0: [b"".join(join(k1, k2).to_bytes(32, "big") for g in s for k1, k2 in g) for s in self.halves]}

    def total(self, k, group):
        return sum(k1 + LAMBDA * k2 for k1, k2 in self.halves[k][group]) % R


def expected(kind, group, total):
    return times_g(total * base_factor(kind, group))


def group_law_sum(kind, group, halves):
    """The same sum by the exact affine law of tests/device_ops.py, term by term (for a sample)."""
    base = D.g_mul(D.G, base_factor(kind, group))
    acc = None
    for k1, k2 in halves:
        acc = D.g_add(acc, D.g_mul(base, join(k1, k2)))
    return D.compress(acc)


# ---- closed forms through the public ABI: the setup [tau^i G], stated for any tau by exact polynomial arithmetic ------------------
def blob_coefficients(blob):
    """The 4096 coefficients of the polynomial whose values on the bit-reversed 4096th roots of unity are the blob's elements."""
    ev = sm.blob_evals(blob)
    nat = [ev[sm.brp(i, 12)] for i in range(4096)]
    return _transform(nat, pow(sm.OMEGA_4096, R - 2, R), pow(4096, R - 2, R))


def blob_of_coefficients(coeffs):
    nat = _transform(list(coeffs) + [0] * (4096 - len(coeffs)), sm.OMEGA_4096, 1)
    return b"".join(nat[sm.brp(i, 12)].to_bytes(32, "big") for i in range(4096))


def _transform(a, w, scale):
    """radix-2 transform over Python integers: out[i] = scale * sum_k a[k] w^(i k)"""
    n = len(a)
    if n == 1:
        return [a[0] * scale % R]
    even, odd = _transform(a[0::2], w * w % R, scale), _transform(a[1::2], w * w % R, scale)
    out, t = [0] * n, 1
    for i in range(n // 2):
        x = odd[i] * t % R
        out[i], out[i + n // 2] = (even[i] + x) % R, (even[i] - x) % R
        t = t * w % R
    return out


def poly_eval(p, z):
    s = 0
    for a in reversed(p):
        s = (s * z + a) % R
    return s


def commitment_scalar(coeffs, tau):
    return poly_eval(coeffs, tau)


def proof_scalar(coeffs, k, tau):
    """q_k(tau) with q_k = (p - I_k) / (X^64 - h_k^64) by exact division: the quotient of p by X^64 - a, a = h_k^64 (the remainder is
    I_k, of degree < 64).  No division by tau^64 - a, which vanishes at tau = 1 for cell 0."""
    a = pow(pow(sm.OMEGA_8192, sm.brp(k, 7), R), 64, R)
    q = [0] * (len(coeffs) - 64)
    rem = list(coeffs)
    for i in range(len(coeffs) - 1, 63, -1):
        q[i - 64] = rem[i]
        rem[i - 64] = (rem[i - 64] + a * rem[i]) % R
        rem[i] = 0
    return poly_eval(q, tau)
