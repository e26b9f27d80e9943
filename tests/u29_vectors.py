"""Shared test vectors of secp256r1's own radix-2^29 unit (ecamd_u29.h, ecamd_p256.h), in the manner of
tests/u29g_vectors.py: every generator yields one record (operation, operand limbs) at a time, receives what a
build of the headers computed for it and asserts on that.  tests/test_u29_host.py drives them with the g++ build,
tests/test_gpu_u29_unit.py with the device build as well (same seeds, same operands, same assertions)."""
import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import u29_consts as K  # noqa: E402

W, MASK, p, R = K.W, K.MASK, K.p, K.R
Rinv = pow(R, p - 2, p)
b = K.b
BUILD = os.path.join(ROOT, "tests", "_build")

# op: entry point; ins: operand word lists; arg: the `negate` switch of madd (None otherwise); edge: an operand at the edge of
# its class, a boundary value or an exceptional pair
Rec = collections.namedtuple("Rec", "op ins arg edge")
# words per item that an operation returns (is_zero returns its answer as the flag)
N_OUT = {"mul": 9, "sqr": 9, "mul_loose": 9, "fold": 9, "inv": 9, "canonical_words": 8, "from_words": 9, "is_zero": 0, "dbl": 27, "add": 27,
         "madd": 27}
FLAGGED = ("is_zero", "add", "madd")
_lib = []


def host_lib():
    """the g++ build of tests/u29_host_shim.cpp (built once per process)"""
    if not _lib:
        os.makedirs(BUILD, exist_ok=True)
        so = os.path.join(BUILD, "u29_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so,
                               os.path.join(ROOT, "tests", "u29_host_shim.cpp")])
        _lib.append(C.CDLL(so))
    return _lib[0]


def limbs(x, n=9):
    d = [(x >> (W * i)) & MASK for i in range(n - 1)]
    d.append(x >> (W * (n - 1)))
    return d


def val(l):
    return sum(int(v) << (W * i) for i, v in enumerate(l))


def arr(l):
    assert all(0 <= v < 2**32 for v in l)
    return (C.c_uint32 * len(l))(*l)


def call(fn, *ins, n_out=9):
    out = (C.c_uint32 * n_out)()
    r = fn(*[arr(x) for x in ins], out)
    return list(out), r


def run(lib, rec):
    """one record through the g++ build: (output words, return value)"""
    fn = getattr(lib, "t_" + rec.op)
    ins = [arr(x) for x in rec.ins]
    if rec.op == "is_zero":
        return [], fn(*ins)
    out = (C.c_uint32 * N_OUT[rec.op])()
    if rec.op == "madd":
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        r = fn(*ins, out, rec.arg)
    else:
        r = fn(*ins, out)
    return list(out), r


def drive(gen, lib):
    """run a generator against the g++ build: the generator asserts.  Returns [(rec, out, r)]"""
    done = []
    try:
        rec = next(gen)
        while True:
            out, r = run(lib, rec)
            done.append((rec, out, r))
            rec = gen.send((out, r))
    except StopIteration:
        pass
    return done


def replay(gen, done):
    """the same generator on recorded outputs of another build: its operands must come out the same"""
    it = iter(done)
    try:
        rec = next(gen)
        while True:
            want, out, r = next(it)
            assert rec[:3] == want[:3], "the replayed generator went another way"
            rec = gen.send((out, r))
    except StopIteration:
        pass
    assert next(it, None) is None, "records left over"


def loose(rng, v, lb, tb):
    """a representation of integer v with random 'looseness': limbs up to lb (top up to tb)"""
    l = limbs(v)
    for i in range(8):
        # move k units of 2^29 from limb i+1 down into limb i
        room = (lb - l[i]) >> W
        k = min(room, l[i + 1], int(rng.integers(0, 8)))
        l[i] += k << W
        l[i + 1] -= k
    assert val(l) == v and max(l[:8]) <= lb and l[8] <= tb
    return l


# ---- test_mul_sqr_random_and_extreme ----
def mul_sqr():
    rng = np.random.default_rng(21)
    cases = []
    for _ in range(300):
        cases.append((int(rng.integers(0, 2**62)) * int(rng.integers(0, 2**62)) ** 4 % (2 * p),
                      int.from_bytes(rng.bytes(40), "big") % (2 * p)))
    cases += [(0, 0), (2 * p - 1, 2 * p - 1), (p, p), (p - 1, 1), (2**256 - 1, 2**256 - 1)]
    for n, (x, y) in enumerate(cases):
        out, _ = yield Rec("mul", [limbs(x), limbs(y)], None, n >= 300)
        assert val(out) % p == x * y * Rinv % p
        assert val(out) < 2 * p and max(out[:8]) <= MASK
        out, _ = yield Rec("sqr", [limbs(x)], None, n >= 300)
        assert val(out) % p == x * x * Rinv % p and val(out) < 2 * p
    # loose class: every limb at 2^30, top limb at its bound -- worst case for the column accumulator
    worst = [1 << 30] * 8 + [6 << 24]
    out, _ = yield Rec("mul_loose", [worst, worst], None, True)
    assert val(out) % p == val(worst) ** 2 * Rinv % p
    for _ in range(200):
        v1 = int.from_bytes(rng.bytes(40), "big") % (5 * p)
        v2 = int.from_bytes(rng.bytes(40), "big") % (5 * p)
        l1, l2 = loose(rng, v1, 1 << 30, 6 << 24), loose(rng, v2, 1 << 30, 6 << 24)
        out, _ = yield Rec("mul_loose", [l1, l2], None, False)
        assert val(out) % p == v1 * v2 * Rinv % p and max(out[:8]) <= MASK


# ---- test_fold_and_canonical ----
def fold_canonical():
    rng = np.random.default_rng(22)
    for _ in range(300):
        v = int.from_bytes(rng.bytes(40), "big") % (6 * p - (1 << 240))
        l = loose(rng, v, 0xfffffffe, 6 << 24)
        out, _ = yield Rec("fold", [l], None, False)
        assert val(out) % p == v % p
        assert val(out) * 16 < 17 * p and max(out[:8]) <= MASK + 16
    for v in (0, 1, p - 1, p, p + 1, 2 * p - 1, int.from_bytes(rng.bytes(32), "big") % (2 * p)):
        words, _ = yield Rec("canonical_words", [limbs(v)], None, True)
        assert sum(int(w) << (32 * i) for i, w in enumerate(words)) == v % p
        back, _ = yield Rec("from_words", [[((v % p) >> (32 * i)) & 0xffffffff for i in range(8)]], None, True)
        assert back == limbs(v % p)
    for k in range(4):
        _, z = yield Rec("is_zero", [limbs(k * p)], None, True)
        assert z == 1
        _, z = yield Rec("is_zero", [limbs(k * p + 1)], None, True)
        assert z == 0
        if k:
            _, z = yield Rec("is_zero", [limbs(k * p - 1)], None, True)
            assert z == 0


# ---- test_inversion_chain ----
def inversion():
    rng = np.random.default_rng(23)
    for _ in range(5):
        x = int.from_bytes(rng.bytes(32), "big") % p or 1
        out, _ = yield Rec("inv", [limbs(x * R % p)], None, False)
        assert val(out) % p == pow(x, p - 2, p) * R % p


# ---- Jacobian formulas vs independent affine arithmetic ----
def aff_add(P, Q):
    if P is None:
        return Q
    if Q is None:
        return P
    if P[0] == Q[0]:
        if (P[1] + Q[1]) % p == 0:
            return None
        lam = (3 * P[0] * P[0] - 3) * pow(2 * P[1], p - 2, p) % p
    else:
        lam = (Q[1] - P[1]) * pow(Q[0] - P[0], p - 2, p) % p
    x = (lam * lam - P[0] - Q[0]) % p
    return (x, (lam * (P[0] - x) - P[1]) % p)


def aff_mul(k, P):
    Rr = None
    while k:
        if k & 1:
            Rr = aff_add(Rr, P)
        P = aff_add(P, P)
        k >>= 1
    return Rr


G = (0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296,
     0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5)


def jac_of(rng, P, xmul, ymul, zmul, classes):
    """Montgomery-domain Jacobian representation of affine P with random Z and non-canonical values
    (xmul etc. multiples of p added) and loose limbs within the (lb, tb) class bounds"""
    z = int.from_bytes(rng.bytes(32), "big") % p or 1
    X = (P[0] * z * z % p) * R % p + xmul * p
    Y = (P[1] * z * z * z % p) * R % p + ymul * p
    Z = z * R % p + zmul * p
    return [loose(rng, v, lb, tb) for v, (lb, tb) in zip((X, Y, Z), classes)]


def jac_to_aff(l27):
    X, Y, Z = (val(l27[0:9]) * Rinv % p, val(l27[9:18]) * Rinv % p, val(l27[18:27]) * Rinv % p)
    if Z == 0:
        return None
    zi = pow(Z, p - 2, p)
    return (X * zi * zi % p, Y * zi * zi * zi % p)


ACC = [(MASK + 16, (1 << 24) + 16), (MASK + 8, (6 << 24) + 8), (2 * MASK, 4 << 24)]
TBL = [(MASK + 16, (1 << 24) + 16), (MASK + 16, 4 << 24), (2 * MASK, 4 << 24)]


# ---- test_jacobian_dbl_add ----
def jacobian_dbl_add():
    rng = np.random.default_rng(24)
    for it in range(40):
        k1, k2 = int(rng.integers(1, 2**40)), int(rng.integers(1, 2**40))
        P, Q = aff_mul(k1, G), aff_mul(k2, G)
        # accumulator class: X < 17/16 p, Y < 6p, Z < 3.5p
        Pj = jac_of(rng, P, 0, int(rng.integers(0, 5)), int(rng.integers(0, 3)), ACC)
        flat = Pj[0] + Pj[1] + Pj[2]
        out, _ = yield Rec("dbl", [flat], None, False)
        assert jac_to_aff(out) == aff_add(P, P)
        assert max(out[0:8]) <= MASK + 16 and max(out[9:17]) <= MASK + 8 and max(out[18:26]) <= 2 * MASK
        assert val(out[0:9]) * 16 < 17 * p and val(out[9:18]) < 6 * p and val(out[18:27]) * 2 < 7 * p
        Qj = jac_of(rng, Q, 0, int(rng.integers(0, 3)), int(rng.integers(0, 3)), TBL)
        out, hz = yield Rec("add", [flat, Qj[0] + Qj[1] + Qj[2]], None, False)
        assert hz == 0 and jac_to_aff(out) == aff_add(P, Q)
        assert val(out[0:9]) * 16 < 17 * p and val(out[9:18]) < 6 * p and val(out[18:27]) * 2 < 7 * p
    # exceptional pairs are detected: P + P and P + (-P) give h_is_zero
    P = aff_mul(12345, G)
    Pj = jac_of(rng, P, 0, 2, 1, ACC)
    Qj = jac_of(rng, P, 0, 2, 2, TBL)
    _, hz = yield Rec("add", [Pj[0] + Pj[1] + Pj[2], Qj[0] + Qj[1] + Qj[2]], None, True)
    assert hz == 1
    Qn = jac_of(rng, (P[0], p - P[1]), 0, 2, 1, TBL)
    out, hz = yield Rec("add", [Pj[0] + Pj[1] + Pj[2], Qn[0] + Qn[1] + Qn[2]], None, True)
    assert hz == 1 and jac_to_aff(out) is None


# ---- test_mixed_addition ----
def mixed_addition():
    rng = np.random.default_rng(26)
    for it in range(40):
        P, Q = aff_mul(int(rng.integers(1, 2**40)), G), aff_mul(int(rng.integers(1, 2**40)), G)
        Pj = jac_of(rng, P, 0, int(rng.integers(0, 5)), int(rng.integers(0, 3)), ACC)
        flat = Pj[0] + Pj[1] + Pj[2]
        qa = limbs(Q[0] * R % p) + limbs(Q[1] * R % p)
        for negate in (0, 1):
            o, hz = yield Rec("madd", [flat, qa], negate, False)
            Qs = (Q[0], (p - Q[1]) % p) if negate else Q
            assert hz == 0 and jac_to_aff(o) == aff_add(P, Qs)
            assert val(o[0:9]) * 16 < 17 * p and val(o[9:18]) < 6 * p and val(o[18:27]) * 2 < 7 * p
    P = aff_mul(777, G)
    Pj = jac_of(rng, P, 0, 3, 2, ACC)
    qa = limbs(P[0] * R % p) + limbs(P[1] * R % p)
    _, hz = yield Rec("madd", [Pj[0] + Pj[1] + Pj[2], qa], 0, True)
    assert hz == 1
    out, hz = yield Rec("madd", [Pj[0] + Pj[1] + Pj[2], qa], 1, True)
    assert hz == 1 and jac_to_aff(out) is None


# ---- test_jacobian_chain_stays_in_bounds ----
def jacobian_chain():
    """200 consecutive doublings/additions through the loop-carried classes"""
    rng = np.random.default_rng(25)
    P = G
    cur = jac_of(rng, P, 0, 5, 2, ACC)
    flat = cur[0] + cur[1] + cur[2]
    aff = P
    for it in range(200):
        if it % 5 == 4:
            Q = aff_mul(int(rng.integers(1, 2**30)), G)
            Qj = jac_of(rng, Q, 0, 2, 2, TBL)
            flat, hz = yield Rec("add", [flat, Qj[0] + Qj[1] + Qj[2]], None, False)
            assert hz == 0
            aff = aff_add(aff, Q)
        else:
            flat, _ = yield Rec("dbl", [flat], None, False)
            aff = aff_add(aff, aff)
        assert jac_to_aff(flat) == aff
        assert val(flat[0:9]) * 16 < 17 * p and val(flat[9:18]) < 6 * p and val(flat[18:27]) * 2 < 7 * p


def check_consts(out):
    """the constants of the headers (t_consts / the device's view of them) against Python integers"""
    assert out[0:9] == limbs(p)
    assert out[9:18] == limbs((1 << 256) % p)
    assert out[18:27] == limbs(R * R % p)
    assert out[27:36] == limbs(R % p)
    assert out[36:45] == limbs(b * R % p)
    q = limbs(p + 1)
    assert q[:3] == [0, 0, 0] and q[4] == q[5] == 0 and out[45:49] == [q[3], q[6], q[7], q[8]]


GENERATORS = [("mul_sqr", mul_sqr), ("fold_canonical", fold_canonical), ("inversion", inversion), ("jacobian_dbl_add", jacobian_dbl_add),
              ("mixed_addition", mixed_addition), ("jacobian_chain", jacobian_chain)]
# records per operation that tests/test_u29_host.py runs (counted on the parent of the commit that introduced this module)
MIN_RECORDS = {"mul": 305, "sqr": 305, "mul_loose": 201, "fold": 300, "canonical_words": 7, "from_words": 7, "is_zero": 11, "inv": 5,
               "dbl": 40 + 160, "add": 42 + 40, "madd": 82}


def check_counts(done_by_name):
    counts = collections.Counter(rec.op for done in done_by_name.values() for rec, _, _ in done)
    assert set(counts) == set(MIN_RECORDS), (sorted(counts), sorted(MIN_RECORDS))
    for op, n in MIN_RECORDS.items():
        assert counts[op] >= n, (op, counts[op], n)
    return dict(counts)
