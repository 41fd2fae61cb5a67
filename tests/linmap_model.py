"""The prover's G1 stage in exact integers: the map it computes stated by its definition, an interpreter of the compiled
programs that run it (csrc/g1_linmap.hpp: Schedule; executed by csrc/k_g1slp.hip), and the plan of degenerate inputs that sends
every kind of addition of every program through each of its exceptional classes.

Points are replaced by their discrete logarithms: a value x stands for x G, the identity is 0, phi is multiplication by lambda.
The programs come from tests/c/dump_linmap.cpp, which takes them from the header the engine compiles them with
(csrc/g1_linmap_programs.hpp); tests/test_gpu_g1_stage.py compares that dump with what a context uploaded.

The definition follows the reference's two transforms (Domain::ifft_g1_take_n, then Domain::fft_g1 on the zero-padded result,
crates/cryptography/polynomial/src/domain.rs; compute_multi_opening_proofs hands the proofs out in bit-reversed order):
    h_m   = (1 / 128) sum_j y_j omega^(-j m),  m < 64        (inverse transform, first 64 kept)
    out_k = sum_{m < 64} h_m omega^(k m),      k < 128       (forward transform of h || 0)
    proof of cell p = out_(bit-reverse_7 p)
The linear map is given x_j = y_j / 2 (so h_m = (1 / 64) sum_j x_j omega^(-j m)), the circulant form u_j = y_j / 128.
"""
import json
import os
import random
import shutil
import subprocess
import tempfile

import numpy as np

import synth

R = synth.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")
OMEGA128 = pow(7, (R - 1) // 128, R)
KIND_MULC = 3  # linmap::OpKind of a launch of constant multiplications; anything else: additions, subtractions, doubling runs
CLASSES = ("a=O", "b=O", "a=b", "a=-b", "a=b=O")  # of the two operands of an addition, after rotation and doubling
MAX_CONDITIONS = 8  # linear conditions one lane carries


def brp7(p):
    return int(format(p, "07b")[::-1], 2)


# ---- the map by its definition ------------------------------------------------------------------------------------------------
_W = [pow(OMEGA128, e, R) for e in range(128)]


def _transforms(v, scale):
    h = [scale * sum(v[j] * _W[(-j * m) % 128] for j in range(128)) % R for m in range(64)]
    out = [sum(h[m] * _W[(k * m) % 128] for m in range(64)) % R for k in range(128)]
    return [out[brp7(p)] for p in range(128)]


def proofs_of_linmap_inputs(x):
    """x_j = y_j / 2, natural Fourier order -> the 128 proofs (as scalars of G) in the order the product writes them"""
    return _transforms(x, pow(64, -1, R))


def proofs_of_circulant_inputs(u):
    """u_j = y_j / 128 -> the same"""
    return _transforms(u, 1)


# ---- the compiled programs -------------------------------------------------------------------------------------------------------
class Program:
    def __init__(self, doc, lam):
        self.id, self.n_slots, self.lam = doc["id"], doc["n_slots"], lam
        self.launches = [tuple(l) for l in doc["launches"]]
        w = doc["words"]
        self.ops = [tuple(w[4 * i:4 * i + 4]) for i in range(len(w) // 4)]
        self.consts = [int(c, 16) for c in doc["consts"]]
        self.launch_of = [None] * len(self.ops)
        for li, (_, first, count) in enumerate(self.launches):
            for i in range(first, first + count):
                self.launch_of[i] = li
        assert None not in self.launch_of
        self.mulc_launches = [li for li, l in enumerate(self.launches) if l[0] == KIND_MULC]

    def is_mulc(self, i):
        return self.launches[self.launch_of[i]][0] == KIND_MULC

    def signature(self, i):
        """the low 16 bits of the flag word (subtract, doubling run, fused pair, doublings of operand a first, rot_a, rot_b), and the
        run length of a doubling run; None for a constant multiplication"""
        if self.is_mulc(i):
            return None
        _, _, b, fl = self.ops[i]
        return (fl & 0xFFFF, b if fl & 2 else 0)

    def signatures(self):
        return sorted({self.signature(i) for i in range(len(self.ops))} - {None})


_DUMP = None


def dump():
    """tests/c/dump_linmap.cpp built with hipcc's host pass and run, once per process -> its JSON document"""
    global _DUMP
    if _DUMP is None:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        with tempfile.TemporaryDirectory() as d:
            exe = os.path.join(d, "dump_linmap")
            subprocess.check_call([hipcc, "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                                   os.path.join(ROOT, "tests", "c", "dump_linmap.cpp"), "-o", exe])
            out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        _DUMP = json.loads(out.stdout)
    return _DUMP


_PROGRAMS = None


def programs():
    global _PROGRAMS
    if _PROGRAMS is None:
        doc = dump()
        lam = int(doc["lambda"], 16)
        assert (lam * lam + lam + 1) % R == 0 and int(doc["omega128"], 16) == OMEGA128
        _PROGRAMS = [Program(p, lam) for p in doc["programs"]]
    return _PROGRAMS


def run(prog, inputs, zero=0, record=None):
    """The program over integers mod r (or over anything with +, -, *, %: the linear forms below): launches in order, within a launch
    every read before any write.  record: a list that receives, per operation (in the order of the words), the operand values as
    the group law meets them -- (a after rotation and doubling, b after rotation), (operand, None) for a doubling run or a
    constant multiplication."""
    arena = [zero] * prog.n_slots
    arena[:128] = inputs
    lp = [1, prog.lam, prog.lam * prog.lam % R]
    for kind, first, count in prog.launches:
        writes = []
        for i in range(first, first + count):
            dst, a, b, fl = prog.ops[i]
            va = arena[a]
            if kind == KIND_MULC:
                rec = (va, None)
                writes.append((dst, va * prog.consts[b] % R))
            elif fl & 2:
                rec = (va, None)
                writes.append((dst, va * (1 << b) % R))
            else:
                ra, rb = (fl >> 8) & 3, (fl >> 10) & 3
                assert ra < 3 and rb < 3
                x = va * (lp[ra] << ((fl >> 3) & 31)) % R
                y = arena[b] * lp[rb] % R
                rec = (x, y)
                if fl & 4:
                    writes.append((dst, (x + y) % R))
                    writes.append((fl >> 16, (x - y) % R))
                else:
                    writes.append((dst, (x - y) % R if fl & 1 else (x + y) % R))
            if record is not None:
                record.append(rec)
        read = {s for i in range(first, first + count) for s in prog.ops[i][1:(2 if kind == KIND_MULC or prog.ops[i][3] & 2 else 3)]}
        assert not read & {d for d, _ in writes}, "an operation writes a slot its launch reads"
        assert len({d for d, _ in writes}) == len(writes), "two results of a launch share a slot"
        for d, v in writes:
            arena[d] = v
    return arena[128:256]


def classify(a, b):
    """the class of an addition's operands, or None for a generic pair"""
    if a == 0 and b == 0:
        return "a=b=O"
    if a == 0:
        return "a=O"
    if b == 0:
        return "b=O"
    if a == b:
        return "a=b"
    if (a + b) % R == 0:
        return "a=-b"
    return None


# ---- the plan of degenerate lanes ---------------------------------------------------------------------------------------------------
_FORMS = {}


def operand_forms(prog):
    """per operation the operands of run() as linear forms in the 128 inputs (numpy object vectors)"""
    if prog.id not in _FORMS:
        eye = []
        for j in range(128):
            e = np.zeros(128, dtype=object)
            e[j] = 1
            eye.append(e)
        rec = []
        run(prog, eye, zero=np.zeros(128, dtype=object), record=rec)
        _FORMS[prog.id] = rec
    return _FORMS[prog.id]


def _rref(rows):
    """reduced row echelon form mod r of a list of 128-vectors -> (rows, pivot columns), or None if they are dependent"""
    rows = [[int(v) % R for v in r] for r in rows]
    piv = []
    for k in range(len(rows)):
        col = next((c for c in range(128) if rows[k][c] and c not in piv), None)
        if col is None:
            return None
        iv = pow(rows[k][col], -1, R)
        rows[k] = [v * iv % R for v in rows[k]]
        for o in range(len(rows)):
            if o != k and rows[o][col]:
                f = rows[o][col]
                rows[o] = [(v - f * w) % R for v, w in zip(rows[o], rows[k])]
        piv.append(col)
    return rows, piv


def _conditions(forms, i, cls):
    a, b = forms[i]
    if b is None or cls == "a=O":
        return [a]
    return {"b=O": [b], "a=b": [a - b], "a=-b": [a + b], "a=b=O": [a, b]}[cls]


def needs_of(prog):
    """what the plan of a program must reach: ("mulc", launch) for an identity operand in the first, a middle and the last
    multiplication launch; (signature, class) for every signature and class (a doubling run has the one class, operand = O)"""
    ml = prog.mulc_launches
    needs = [("mulc", li) for li in sorted({ml[0], ml[len(ml) // 2], ml[-1]})]  # (every program has ONE such launch today)
    for sig in prog.signatures():
        for cls in (("a=O",) if sig[0] & 2 else CLASSES):
            needs.append((sig, cls))
    return needs


def hits_of(prog, x):
    """what a lane with inputs x reaches, from the operand values the model records"""
    rec = []
    run(prog, x, record=rec)
    hits = set()
    for i, (a, b) in enumerate(rec):
        if prog.is_mulc(i):
            if a == 0:
                hits.add(("mulc", prog.launch_of[i]))
        elif b is None:
            if a == 0:
                hits.add((prog.signature(i), "a=O"))
        else:
            c = classify(a, b)
            if c:
                hits.add((prog.signature(i), c))
    return hits


def pool_scalars(n=300, seed=20260):
    rng = random.Random(seed)
    return [rng.randrange(1, R) for _ in range(n)]


def plan_lanes(prog, pool, seed=1):
    """Degenerate lanes of a program: each carries up to MAX_CONDITIONS linear conditions on its 128 inputs (Gaussian elimination
    gives the pivot inputs, the others come from the pool), chosen greedily until every need is hit by some lane -- as the model
    finds it in the operand values, not as intended.  -> list of input vectors; raises if a need cannot be reached."""
    forms = operand_forms(prog)
    rng = random.Random(1000 * prog.id + seed)
    ops_of = {}  # the first few operations of every kind: several classes of one signature share a lane on different operations
    for i in range(len(prog.ops)):
        key = ("mulc", prog.launch_of[i]) if prog.is_mulc(i) else prog.signature(i)
        if len(ops_of.setdefault(key, [])) < 8:
            ops_of[key].append(i)
    need = needs_of(prog)
    lanes = []

    def solve(conds):
        red = _rref(conds)
        if red is None:
            return None
        rows, piv = red
        x = [pool[rng.randrange(len(pool))] for _ in range(128)]
        for row, c in zip(rows, piv):
            x[c] = 0
        for row, c in zip(rows, piv):
            x[c] = -sum(v * xv for v, xv in zip(row, x) if v) % R
        return x

    alone = set()
    while need:
        conds, picked, ops_used = [], [], set()
        for nd in need:
            if nd in alone and picked:
                continue
            key, cls = (nd, "a=O") if nd[0] == "mulc" else nd
            for op in ops_of[key]:
                if op in ops_used:  # two classes of one operation in one lane would be a third class
                    continue
                add = _conditions(forms, op, cls)
                if len(conds) + len(add) > MAX_CONDITIONS:
                    break
                if _rref(conds + add) is None:
                    continue
                conds += add
                picked.append(nd)
                ops_used.add(op)
                break
            if len(conds) == MAX_CONDITIONS or nd in alone:
                break
        x = solve(conds)
        hits = hits_of(prog, x) & set(need)
        if not hits:
            raise AssertionError(f"program {prog.id}: {picked} cannot be reached")
        for nd in picked:  # a need its own lane did not reach (its neighbours' conditions changed its class) gets a lane to itself
            if nd not in hits:
                if nd in alone:
                    raise AssertionError(f"program {prog.id}: {nd} cannot be reached")
                alone.add(nd)
        lanes.append(x)
        need = [nd for nd in need if nd not in hits]
    return lanes


def generic_lanes(prog, pool, count=4):
    """lanes no operation of which meets a degenerate operand: every input a pool value"""
    rng = random.Random(77 + prog.id)
    out = []
    while len(out) < count:
        x = [pool[rng.randrange(len(pool))] for _ in range(128)]
        if not hits_of(prog, x):
            out.append(x)
    return out


# ---- where the lanes go in a batch of n --------------------------------------------------------------------------------------------
def edge_positions(n):
    """lane 0, a middle lane, the last lane of a 16-blob quad wave and of a 64-lane group, lane 64, lane n - 1 (the one the padding
    lanes repeat), as far as the batch has them"""
    out = []
    for p in (0, n - 1, n // 2, 15, 63, 64):
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


def layout(n, n_degenerate):
    """-> list of batches; a batch is a list of n entries ("d", k) (degenerate lane k), ("g", k) (generic lane k) or ("o", 0) (an
    all-identity lane).  Every degenerate lane appears once; they take the edge positions first, and a batch with fewer of them
    than edges repeats them there.  Lanes 1 and n - 2 are generic (a regular neighbour of both ends), lane 2 is all identity; the
    other positions alternate between generic and all-identity lanes."""
    edges = edge_positions(n)
    fixed = {1: ("g", 0), n - 2: ("g", 1), 2: ("o", 0)}
    fixed = {p: e for p, e in fixed.items() if p not in edges}
    free = [p for p in edges + [p for p in range(n) if p not in edges] if p not in fixed]
    per_batch = len(free) - (1 if n < 16 else 4)  # (room for the other two generic lanes)
    batches, k = [], 0
    while k < n_degenerate or not batches:
        take = min(per_batch, n_degenerate - k)
        lanes = [None] * n
        for p, e in fixed.items():
            lanes[p] = e
        for d in range(max(take, min(len(edges), len(free)) if take else 0)):
            lanes[free[d]] = ("d", k + d % take)
        g = 2
        for p in range(n):
            if lanes[p] is None:
                lanes[p] = ("o", 0) if g % 3 == 1 else ("g", g % 4)
                g += 1
        batches.append(lanes)
        k += take
    return batches


def lane_inputs(entry, degenerate, generic):
    kind, k = entry
    if kind == "d":
        return degenerate[k]
    if kind == "g":
        return generic[k % len(generic)]
    return [0] * 128
