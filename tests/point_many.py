"""The statement of eth_kzg_amd_verify_kzg_proof_many (csrc/verify_host.hpp: PointProofTranscript), in hashlib, Python integers and the
oracle's G1 operations -- never the library.

Item i = (commitment C_i, z_i, y_i, proof pi_i).  A call is cut into passes of at most P items in the caller's order; within a pass of n_p:
    LEAF_i = SHA-256("RCKZGPROOFLEAF_1" | C_i | z_i | y_i | pi_i)
    SEED   = SHA-256("RCKZGPROOFFOLD_1" | be64(n_p) | LEAF_0 | .. | LEAF_{n_p - 1})
    rho_i  = the first 16 bytes of SHA-256(SEED | be64(i)) as a little-endian integer mod 2^127, 0 -> 1; i = position in the pass
    pair(R) = ( sum_{i in R, status 0} rho_i pi_i ,  sum_{i in R, status 0} rho_i (C_i + z_i pi_i - y_i G) )
The status of an item: 2 if the commitment or the proof is not a canonical point of the subgroup, else 1 if z or y is >= r, else 0.
An item whose status is not 0 is hashed like any other and takes no part in any sum."""
import hashlib

import oracle_lib
import synth
from verify_transcript import INF, be64, fr_be, off_subgroup_point, setup_g1_first64  # noqa: F401

R = synth.R
LEAF_DOMAIN = b"RCKZGPROOFLEAF_1"
SEED_DOMAIN = b"RCKZGPROOFFOLD_1"
PASS = 16384  # the product's P (csrc/verify_host.hpp: POINT_MANY_PASS); the tests that depend on it say so


def generator():
    return setup_g1_first64()[0]


def leaf(item):
    c, z, y, p = item
    assert (len(c), len(z), len(y), len(p)) == (48, 32, 32, 48)
    return hashlib.sha256(LEAF_DOMAIN + c + z + y + p).digest()


def seed(leaves):
    return hashlib.sha256(SEED_DOMAIN + be64(len(leaves)) + b"".join(leaves)).digest()


def weight(seed32, i):
    v = int.from_bytes(hashlib.sha256(seed32 + be64(i)).digest()[:16], "little") % (1 << 127)
    return v or 1


def pass_bounds(n, pass_size=PASS):
    """the first item of every pass, then n"""
    return list(range(0, n, pass_size)) + [n]


def item_status(item):
    c, z, y, p = item
    if oracle_lib.g1_validate(c, True) != 0 or oracle_lib.g1_validate(p, True) != 0:
        return 2
    if int.from_bytes(z, "big") >= R or int.from_bytes(y, "big") >= R:
        return 1
    return 0


class PassStatement:
    """leaves, seed and weights of one pass (items in the caller's order) and the pair of any range of it"""

    def __init__(self, items, statuses):
        self.items, self.statuses = items, statuses
        self.leaves = [leaf(it) for it in items]
        self.seed = seed(self.leaves)
        self.rho = [weight(self.seed, i) for i in range(len(items))]
        self._pairs = {}

    def pair(self, lo, hi):
        """compress(first sum) | compress(second sum) over the items lo <= i < hi whose status is 0"""
        if (lo, hi) not in self._pairs:
            part = [i for i in range(lo, hi) if self.statuses[i] == 0]
            if not part:
                self._pairs[(lo, hi)] = INF + INF
            else:
                G = generator()
                pts, sc, pts2, sc2 = [], [], [], []
                ysum = 0
                for i in part:
                    c, z, y, p = self.items[i]
                    rho = self.rho[i]
                    pts.append(p)
                    sc.append(fr_be(rho))
                    pts2 += [c, p]
                    sc2 += [fr_be(rho), fr_be(rho * int.from_bytes(z, "big"))]
                    ysum += rho * int.from_bytes(y, "big")
                pts2.append(G)
                sc2.append(fr_be(-ysum))
                self._pairs[(lo, hi)] = oracle_lib.g1_msm(b"".join(pts), b"".join(sc)) + oracle_lib.g1_msm(b"".join(pts2), b"".join(sc2))
        return self._pairs[(lo, hi)]


def call_statement(items, statuses, pass_size=PASS):
    """-> (bounds, [PassStatement per pass])"""
    bounds = pass_bounds(len(items), pass_size)
    return bounds, [PassStatement(items[lo:hi], statuses[lo:hi]) for lo, hi in zip(bounds, bounds[1:])]


# ---- items -----------------------------------------------------------------------------------------------------------------------------
def g1_mul_int(point, k):
    return oracle_lib.g1_mul(point, fr_be(k))


def degenerate_items():
    """{name: item} -- operands the equation degenerates on.  The oracle gives each verdict (the tests ask it); what each is meant to be:
    valid: zero-polynomial, constant-polynomial, (z = 0, an opening with y = 0 and z inside the domain come from blobs: the GPU test
    makes them with compute_kzg_proof); invalid: doubling, cancels, equals-yG."""
    G = generator()
    c = int.from_bytes(hashlib.sha256(b"point-many:constant").digest(), "big") % R
    z = int.from_bytes(hashlib.sha256(b"point-many:z").digest(), "big") % R
    return {
        "zero-polynomial": (INF, fr_be(z), fr_be(0), INF),
        "constant-polynomial": (g1_mul_int(G, c), fr_be(z), fr_be(c), INF),           # C - y G cancels
        "doubling": (g1_mul_int(G, 5), fr_be(5), fr_be(0), G),                        # C + z pi = 5 G + 5 G
        "cancels": (g1_mul_int(G, R - 5), fr_be(5), fr_be(0), G),                     # C + z pi = the identity
        "equals-yG": (g1_mul_int(G, 7), fr_be(5), fr_be(12), G),                      # C + z pi = 12 G = y G, pi != identity
    }


def error_order_items(good):
    """good = a valid item -> {name: (item, status)}: one item of each shape of the issue's "order of errors" """
    c, z, y, p = good
    off = off_subgroup_point()
    r_be, top = R.to_bytes(32, "big"), b"\xff" * 32
    return {
        "bad-commitment-and-z=r": ((off, r_be, y, p), 2),
        "bad-proof-and-y=2^256-1": ((c, z, top, off), 2),
        "z=r": ((c, r_be, y, p), 1),
        "y=r": ((c, z, r_be, p), 1),
        "z=y=r-1": ((c, fr_be(R - 1), fr_be(R - 1), p), 0),
    }

