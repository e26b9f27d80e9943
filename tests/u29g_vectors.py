"""Shared test vectors of the generic radix-2^29 units (ecamd_u29g.h, ecamd_jacg.h, ecamd_rcbg.h).

Every generator below is a coroutine: it yields one record (operation, operand limbs) at a time, receives
what a build of the headers computed for it, and asserts on that -- the residue against Python integers,
the bound class of the output limbs.  tests/test_u29g_host.py drives the generators with the g++ build
(`drive`); tests/test_gpu_u29g_units.py drives them once with the g++ build to collect the records (some
operands are outputs of earlier records: the chains of `jacobian`), sends all records of an operation to
the device in one launch, and then replays the generators on the device's outputs (`replay`), so that
both builds pass through the very same assertions on the very same operands (same seeds)."""
import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import g29_consts as G  # noqa: E402
from oracles import CURVES  # noqa: E402

W, MASK = G.W, G.MASK
BUILD = os.path.join(ROOT, "tests", "_build")
HOST_SHIM = os.path.join(ROOT, "tests", "u29g_host_shim.cpp")

# f: the Field (curve image) the record runs on; op: entry point; ins: operand limb lists; arg: the `sq` switch of mul / the `dbl`
# switch of rcb (None otherwise); edge: an operand at the edge of its class, a boundary value or an exceptional pair
Rec = collections.namedtuple("Rec", "f op ins arg edge")
N_OUT = {"mul": 1, "mulword": 1, "canon": 1, "neg": 1, "inv": 1, "add": 3, "dbl": 3, "madd": 3, "dblt": 3, "rcb": 3, "liftx": 2}


# (name, object the unit's headers are compiled as, curve that selects the unit, layout of the curve image): the 18 generic units;
# the dense 256- and 384-bit units also on the secp curves the host test runs them on
UNITS = [("192", "dense", "BRAINPOOLP192R1", 0), ("224", "dense", "BRAINPOOLP224R1", 0), ("255", "dense", "WEI25519", 0),
         ("256", "dense", "BRAINPOOLP256R1", 0), ("256-secp256r1", "dense", "SECP256R1", 0), ("256-secp256k1", "dense", "SECP256K1", 0),
         ("320", "dense", "BRAINPOOLP320R1", 0), ("384", "dense", "BRAINPOOLP384R1", 0), ("384-secp384r1", "dense", "SECP384R1", 0),
         ("448", "dense", "WEI448", 0), ("511", "dense", "GOST512", 0), ("512", "dense", "BRAINPOOLP512R1", 0), ("521", "dense", "SECP521R1", 0),
         ("521m", "521m", "SECP521R1", 1), ("255c", "255c", "WEI25519", 2), ("256k", "256k", "SECP256K1", 4), ("448g", "448g", "WEI448", 5),
         ("384n", "384n", "SECP384R1", 0), ("224s", "224s", "SECP224R1", 0), ("192s", "192s", "SECP192R1", 0)]
HOST_FLAGS = {"dense": [], "521m": ["-DG29_M521P", "-DSHIM_ONLY_521"], "255c": ["-DG29_P25519", "-DSHIM_ONLY_255"],
              "256k": ["-DG29_K256", "-DSHIM_ONLY_256"], "448g": ["-DG29_P448", "-DSHIM_ONLY_448"], "384n": ["-DG29_P384S", "-DSHIM_ONLY_384"],
              "224s": ["-DG29_P224S", "-DSHIM_ONLY_224"], "192s": ["-DG29_P192S", "-DSHIM_ONLY_192"]}
HOST_NAME = {"dense": "", "521m": "_m521p", "255c": "_p25519", "256k": "_k256", "448g": "_p448", "384n": "_n384", "224s": "_s224", "192s": "_s192"}
_libs = {}


def host_lib(name, flags=()):
    """the g++ build of tests/u29g_host_shim.cpp with `flags`, as tests/_build/u29g_host<name>.so (built once per process)"""
    if name not in _libs:
        os.makedirs(BUILD, exist_ok=True)
        so = os.path.join(BUILD, f"u29g_host{name}.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + list(flags) + ["-o", so, HOST_SHIM])
        _libs[name] = (tuple(flags), C.CDLL(so))
    assert _libs[name][0] == tuple(flags), (name, flags)
    return _libs[name][1]


def val(l, w=W):
    return sum(int(v) << (w * i) for i, v in enumerate(l))


def arr(l):
    assert all(0 <= v < 2**32 for v in l), l
    return (C.c_uint32 * len(l))(*l)


class Field:
    def __init__(self, lib, curve, flavour=0, iso_u=None):
        c = CURVES[curve]
        self.curve, self.flavour = curve, flavour
        self.p, self.a, self.b = c["p"], c["a"], c["b"]
        self.pb = self.p.bit_length()
        img, self.nl = G.image(self.p, self.a, self.b, flavour, iso_u)
        self.W = G.width(flavour)          # 28 on the Goldilocks unit, 29 everywhere else
        self.MASK = (1 << self.W) - 1
        self.k = arr(img)
        self.lib = lib
        info = (C.c_uint32 * 8)()
        getattr(lib, f"g_info_{self.pb}")(info)
        assert info[0] == self.nl and info[5] == 4 * len(img), (list(info), len(img))
        self.head, self.va, self.fa_lb, self.fa_tb = info[1], info[4], info[6], info[7]
        self.R = 1 if flavour in (1, 2, 4, 5) else 1 << (self.W * self.nl)
        self.Rinv = pow(self.R, self.p - 2, self.p)

    def fn(self, name):
        return getattr(self.lib, f"g_{name}_{self.pb}")

    def val(self, l):
        return val(l, self.W)

    def digits(self, v):
        return G.digits(v, self.nl, self.W)

    def vmax(self, vb, tb):
        """largest multiple of p a class (value bound vb, top limb bound tb) can hold"""
        return min(vb, ((tb - 1) << (self.W * (self.nl - 1))) // self.p)

    def loose(self, rng, v, lb, tb):
        l = self.digits(v)
        for i in range(self.nl - 1):
            room = (lb - l[i]) >> self.W
            k = min(room, l[i + 1], int(rng.integers(0, 8)))
            l[i] += k << self.W
            l[i + 1] -= k
        assert self.val(l) == v and max(l[:-1]) <= lb and l[-1] <= tb, (l, lb, tb)
        return l

    def fa(self, rng, residue, mult=None):
        """an FA-class representation of `residue` mod p: value residue + mult*p, loose limbs"""
        vmax = self.vmax(self.va, self.fa_tb)
        mult = int(rng.integers(0, max(1, vmax - 1))) if mult is None else mult
        return self.loose(rng, residue % self.p + mult * self.p, self.fa_lb, self.fa_tb)

    def call(self, name, *ins, n_out=None):
        out = (C.c_uint32 * (n_out or self.nl))()
        r = self.fn(name)(self.k, *[arr(x) for x in ins], out)
        return list(out), r

    def infot(self):
        """(VT, FT::LB, FT::TB) of the tight accumulator class, (0, ..) where the unit has none"""
        it3 = (C.c_uint32 * 3)()
        getattr(self.lib, f"g_infot_{self.pb}")(it3)
        return list(it3)

    def run(self, rec):
        """one record through the g++ build: (output limbs, return value)"""
        out = (C.c_uint32 * (N_OUT[rec.op] * self.nl))()
        ins = [arr(x) for x in rec.ins]
        if rec.op == "mulword":
            r = self.fn(rec.op)(*ins, out)
        elif rec.arg is not None:
            r = self.fn(rec.op)(self.k, *ins, out, rec.arg)
        else:
            r = self.fn(rec.op)(self.k, *ins, out)
        return list(out), r


def drive(gen, run=None):
    """run a generator against a build: `run(rec)` computes, the generator asserts.  Returns [(rec, out, r)]"""
    done = []
    try:
        rec = next(gen)
        while True:
            out, r = (run or rec.f.run)(rec)
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
            assert (rec.op, rec.ins, rec.arg) == (want.op, want.ins, want.arg), "the replayed generator went another way"
            rec = gen.send((out, r))
    except StopIteration:
        pass
    assert next(it, None) is None, "records left over"


# ---- field operations (test_field_ops) ----
def field_ops(f, flavour=0):
    rng = np.random.default_rng(41)
    p = f.p
    for it in range(60):
        x = int.from_bytes(rng.bytes(80), "big") % p
        y = int.from_bytes(rng.bytes(80), "big") % p
        lx, ly = f.fa(rng, x), f.fa(rng, y)
        if it == 0:  # extreme: largest value the class allows, every low limb at its bound
            vmax = max(0, f.vmax(f.va, f.fa_tb) - 1)
            lx = f.fa(rng, x, vmax)
            ly = f.fa(rng, y, vmax)
        if it == 1 and flavour in (1, 2, 4, 5):   # every limb at the class bound (the value is then what it is: only the residue matters)
            lx = [f.fa_lb] * (f.nl - 1) + [f.fa_tb]
            ly = [f.fa_lb] * (f.nl - 1) + [f.fa_tb]
            x, y = f.val(lx) % p, f.val(ly) % p
        out, _ = yield Rec(f, "mul", [lx, ly], 0, it < 2)
        assert f.val(out) % p == f.val(lx) * f.val(ly) * f.Rinv % p
        # exact low digits -- on the Goldilocks unit limbs 1 and 9 keep the high parts of the two wrap-around carries (< 2^10)
        slack = [(1 << 10) if ((flavour == 5 and i in (1, 9)) or (flavour == 1 and i == 1)) else
                 ((1 << 17) if (flavour == 2 and i == 1) else ((1 << 15) if (flavour == 4 and i == 2) else 0)) for i in range(f.nl)]
        assert f.val(out) < 2 * p + (f.val(lx) * f.val(ly) >> (f.W * f.nl) if flavour not in (1, 5) else 0)
        assert all(v <= f.MASK + sl for v, sl in zip(list(out)[:-1], slack))
        out, _ = yield Rec(f, "mul", [lx, lx], 1, it < 2)
        assert f.val(out) % p == f.val(lx) ** 2 * f.Rinv % p
        assert all(v <= f.MASK + sl for v, sl in zip(list(out)[:-1], slack)) and (flavour not in (1, 5) or f.val(out) < 2 * p)
    # canonical digits, negation, inversion
    for v in (0, 1, p - 1, p, p + 1, 2 * p - 1, int.from_bytes(rng.bytes(80), "big") % (2 * p)):
        d, _ = yield Rec(f, "canon", [f.digits(v)], None, True)
        assert f.val(d) == v % p and max(d[:-1]) <= f.MASK
        n, _ = yield Rec(f, "neg", [f.digits(v)], None, True)
        assert (f.val(n) + v) % p == 0 and max(n[:-1]) <= f.fa_lb and n[-1] <= f.fa_tb
    if flavour in (1, 2, 4, 5):
        # lazy representatives of a multiplication result: limbs 1 (and 9; secp256k1: 2) over their width, values around 2^|p|
        top = 1 << f.pb
        lazy = {2: 1 << 17, 4: 1 << 15}.get(flavour, 1 << 10)     # P25519_MULX / K256_MULX / P448_MULX
        topbits = f.pb - f.W * (f.nl - 1)                     # 23 for 2^255 - 19, 24 for secp256k1, 28 for the no-headroom flavours
        # top limb of the class (MulOut of ecamd_u29g.h)
        fm_tb = {2: (1 << 23) + (1 << 12), 4: (1 << 24) + (1 << 17)}.get(flavour, (1 << 28) - 1)
        lazy_limbs = {5: (1, 9), 4: (2,)}.get(flavour, (1,))
        for v in (top - 1, top, top + 2**224, 2 * p - 1, p + 2**224 + 1, top + 5, top + 18, top + 19, top + 20, top + 2**32 + 976,
                  top + 2**32 + 977, top + 2**32 + 978):
            v = min(v, 2 * p - 1)
            l = f.digits(v)
            # every vector becomes a member of the class (none is dropped): a lazy limb borrows from its neighbour where it then
            # stays within mask + slack, and a top limb above the class bound is cut to the bound -- the value is then val(l)
            for i in lazy_limbs:
                if l[i] < lazy and l[i + 1] > 0:
                    l[i] += 1 << f.W
                    l[i + 1] -= 1
            l[-1] = min(l[-1], fm_tb)
            v = f.val(l)
            assert max(l[:-1]) <= f.MASK + lazy and l[-1] <= fm_tb and v < 2 * p
            d, _ = yield Rec(f, "canon", [l], None, True)
            assert f.val(d) == v % p and max(d) <= f.MASK, hex(v)
        # the largest member of the class: every limb at its mask, the lazy ones at mask + the slack (value above 2^|p|)
        for extra in (lazy, 1, 0):
            l = [f.MASK] * (f.nl - 1) + [(1 << topbits) - 1]
            for i in lazy_limbs:
                l[i] += extra
            d, _ = yield Rec(f, "canon", [l], None, True)
            assert f.val(d) == f.val(l) % p and max(d) <= f.MASK
    x = int.from_bytes(rng.bytes(80), "big") % p or 1
    iv, _ = yield Rec(f, "inv", [f.digits(x * f.R % p)], None, False)
    assert f.val(iv) % p == pow(x, p - 2, p) * f.R % p


def aff_add(P, Q, a, p):
    if P is None:
        return Q
    if Q is None:
        return P
    if P[0] == Q[0]:
        if (P[1] + Q[1]) % p == 0:
            return None
        lam = (3 * P[0] * P[0] + a) * pow(2 * P[1], p - 2, p) % p
    else:
        lam = (Q[1] - P[1]) * pow(Q[0] - P[0], p - 2, p) % p
    x = (lam * lam - P[0] - Q[0]) % p
    return (x, (lam * (P[0] - x) - P[1]) % p)


# ---- Jacobian formulas (test_jacobian) ----
def jacobian(f, flavour=0):
    rng = np.random.default_rng(42)
    c = CURVES[f.curve]
    p, a = f.p, f.a
    G0 = (c["gx"], c["gy"])

    def jac(P):
        z = int.from_bytes(rng.bytes(80), "big") % p or 1
        X, Y, Z = P[0] * z * z % p * f.R % p, P[1] * z * z * z % p * f.R % p, z * f.R % p
        return f.fa(rng, X) + f.fa(rng, Y) + f.fa(rng, Z)

    def aff(l):
        nl = f.nl
        X, Y, Z = (f.val(l[0:nl]) * f.Rinv % p, f.val(l[nl:2 * nl]) * f.Rinv % p, f.val(l[2 * nl:3 * nl]) * f.Rinv % p)
        if Z == 0:
            return None
        zi = pow(Z, p - 2, p)
        return (X * zi * zi % p, Y * zi * zi * zi % p)

    def in_class(l):
        nl = f.nl
        for k in range(3):
            part = l[k * nl:(k + 1) * nl]
            assert max(part[:-1]) <= f.fa_lb and part[-1] <= f.fa_tb and f.val(part) < f.va * p

    P = G0
    Q = aff_add(G0, G0, a, p)
    cur = jac(P)
    acc = P
    for it in range(24):
        if it % 4 == 3:
            Q = aff_add(Q, G0, a, p)
            cur, hz = yield Rec(f, "add", [cur, jac(Q)], None, False)
            assert hz == 0
            acc = aff_add(acc, Q, a, p)
        else:
            cur, _ = yield Rec(f, "dbl", [cur], None, False)
            acc = aff_add(acc, acc, a, p)
        assert aff(cur) == acc
        in_class(cur)
    # mixed addition and doubling on the tight accumulator class of the affine-table kernels (not for secp256k1's flavour,
    # which keeps the Jacobian table)
    it3 = f.infot()
    if it3[0]:
        vt, ft_lb, ft_tb = it3[0], it3[1], it3[2]

        def ft(residue):
            vmax = f.vmax(vt, ft_tb)
            mult = int(rng.integers(0, max(1, vmax - 1)))
            return f.loose(rng, residue % p + mult * p, ft_lb, ft_tb)

        def jac_t(P):
            z = int.from_bytes(rng.bytes(80), "big") % p or 1
            return ft(P[0] * z * z % p * f.R % p) + ft(P[1] * z * z * z % p * f.R % p) + ft(z * f.R % p)

        def in_class_t(l):
            for k in range(3):
                part = l[k * f.nl:(k + 1) * f.nl]
                assert max(part[:-1]) <= ft_lb and part[-1] <= ft_tb and f.val(part) < vt * p

        def affine_fa(P):
            return f.fa(rng, P[0] * f.R % p) + f.fa(rng, P[1] * f.R % p)
        cur, acc = jac_t(acc), acc
        for it in range(16):
            if it % 3 == 2:
                cur, _ = yield Rec(f, "dblt", [cur], None, False)
                acc = aff_add(acc, acc, a, p)
            else:
                Q = aff_add(Q, G0, a, p)
                T = Q if it % 2 else (Q[0], p - Q[1])
                cur, _ = yield Rec(f, "madd", [cur, affine_fa(T)], None, False)
                acc = aff_add(acc, T, a, p)
            assert aff(cur) == acc
            in_class_t(cur)
            if it % 5 == 4:
                cur = jac_t(acc)      # a fresh loose representative of the class
        # the same x: Z3 = 0, and it stays 0 through later doublings and additions (the kernels test the final Z once)
        for T in (P, (P[0], p - P[1])):
            out, _ = yield Rec(f, "madd", [jac_t(P), affine_fa(T)], None, True)
            assert aff(out) is None
            in_class_t(out)
            out, _ = yield Rec(f, "dblt", [out], None, True)
            assert aff(out) is None
            in_class_t(out)
            out, _ = yield Rec(f, "madd", [out, affine_fa(Q)], None, True)
            assert aff(out) is None
            in_class_t(out)
    # exceptional pairs are flagged
    _, hz = yield Rec(f, "add", [jac(P), jac(P)], None, True)
    assert hz == 1
    out, hz = yield Rec(f, "add", [jac(P), jac((P[0], p - P[1]))], None, True)
    assert hz == 1 and aff(out) is None


# ---- mul_word (_check_mul_word) ----
def mul_word(f, flavour, cst, lazy, lazy_limbs):
    """mul_word (a24 e of the x-only ladders as NL MADs): residue, limb class of a multiplication result, value < 2p,
    on random operands and on operands with every limb at the top of its range"""
    rng = np.random.default_rng(44)
    topmax = (1 << 29) - 1 if flavour == 5 else (1 << 32) - 1
    for it in range(40):
        if it == 0:
            l = [(1 << 32) - 1] * (f.nl - 1) + [topmax]
        elif it == 1:
            l = [0] * f.nl
        else:
            l = [int(rng.integers(0, 1 << 32)) for _ in range(f.nl - 1)] + [int(rng.integers(0, topmax + 1))]
            if it % 3 == 0:
                l = f.digits(int.from_bytes(rng.bytes(80), "big") % f.p)
        out, _ = yield Rec(f, "mulword", [l], None, it < 2)
        assert f.val(out) % f.p == f.val(l) * cst % f.p
        assert f.val(out) < 2 * f.p
        assert all(v <= f.MASK + (lazy if i in lazy_limbs else 0) for i, v in enumerate(list(out)[:-1]))
        assert out[f.nl - 1] < (1 << (f.pb - f.W * (f.nl - 1)))


# ---- the signed sparse flavours (_sparse_flavour_checks) ----
def sparse_small_products(f):
    """small products: the negative reduction terms outweigh a column's products, so column sums go negative and the carries must
    be arithmetic"""
    rng = np.random.default_rng(384)
    p = f.p
    for it in range(200):
        x = int.from_bytes(rng.bytes(48), "big") % p
        y = (0, 1, 2, 1 << 29, (1 << 29) - 1, 1 << 58, p - 1, int(rng.integers(0, 1 << 20)))[it % 8]
        lx, ly = f.digits(x), f.digits(y)
        if it % 3 == 0:
            lx, ly = ly, lx
        out, _ = yield Rec(f, "mul", [lx, ly], 0, it < 8)
        assert f.val(out) % p == x * y * f.Rinv % p and f.val(out) < 2 * p and max(list(out)[:-1]) <= f.MASK
        out, _ = yield Rec(f, "mul", [f.digits(y), f.digits(y)], 1, it < 8)
        assert f.val(out) % p == y * y * f.Rinv % p and f.val(out) < 2 * p and max(list(out)[:-1]) <= f.MASK


# ---- complete formulas (test_complete_formulas_on_the_radix29_types) ----
def rcb_add_py(P, Q, a, b, p):
    """RCB Algorithm 1 (generic a) over Python integers: the polynomials of ecamd_point.h:pt_add"""
    X1, Y1, Z1 = P
    X2, Y2, Z2 = Q
    b3 = 3 * b
    t0, t1, t2 = X1 * X2 % p, Y1 * Y2 % p, Z1 * Z2 % p
    t3 = ((X1 + Y1) * (X2 + Y2) - t0 - t1) % p
    t4 = ((X1 + Z1) * (X2 + Z2) - t0 - t2) % p
    t5 = ((Y1 + Z1) * (Y2 + Z2) - t1 - t2) % p
    z3 = (b3 * t2 + a * t4) % p
    x3, z3 = (t1 - z3) % p, (t1 + z3) % p
    y3 = x3 * z3 % p
    t1 = (3 * t0 + a * t2) % p
    t4 = (b3 * t4 + a * (t0 - a * t2)) % p
    return ((t3 * x3 - t5 * t4) % p, (y3 + t1 * t4) % p, (t5 * z3 + t3 * t1) % p)


def rcb_dbl_py(P, a, b, p):
    """RCB Algorithm 3 (generic a): the polynomials of ecamd_point.h:pt_dbl"""
    X, Y, Z = P
    b3 = 3 * b
    t0, t1, t2 = X * X % p, Y * Y % p, Z * Z % p
    t3, z3 = 2 * X * Y % p, 2 * X * Z % p
    y3 = (a * z3 + b3 * t2) % p
    x3, y3 = (t1 - y3) % p, (t1 + y3) % p
    y3 = x3 * y3 % p
    x3 = t3 * x3 % p
    t3 = (a * (t0 - a * t2) + b3 * z3) % p
    t0 = (3 * t0 + a * t2) % p
    t2 = 2 * Y * Z % p
    return ((x3 - t2 * t3) % p, (y3 + t0 * t3) % p, 4 * t2 * t1 % p)


def complete_formulas(f):
    """ecamd_rcbg.h (the tail of the EdDSA verifications on the 2^255 - 19 and Goldilocks units): the same FIELD ELEMENTS as the
    Renes-Costello-Batina polynomials over Python integers -- not just the same projective point -- for random pairs, P + P,
    P + (-P), infinity on either side, and the exceptional pairs of these even-order curves (P and P + T with T of order two:
    the result is (0 : 0 : 0), which the callers reject as libecc's prj_pt_add does)."""
    curve = f.curve
    rng = np.random.default_rng(99)
    c = CURVES[curve]
    p, a, b = f.p, f.a, f.b
    G0 = (c["gx"], c["gy"])

    def proj(P):
        if P is None:
            return (0, 1, 0)
        z = int.from_bytes(rng.bytes(80), "big") % p or 1
        return (P[0] * z % p, P[1] * z % p, z)

    def limbs(P):
        return f.fa(rng, P[0]) + f.fa(rng, P[1]) + f.fa(rng, P[2])

    def got(out):
        nl = f.nl
        return tuple(f.val(out[k * nl:(k + 1) * nl]) % p for k in range(3))

    def in_class(out):
        nl = f.nl
        for k in range(3):
            part = out[k * nl:(k + 1) * nl]
            assert max(part[:-1]) <= f.fa_lb and part[-1] <= f.fa_tb and f.val(part) < f.va * p

    # the point of order two: (x0, 0) with x0 a root of x^3 + a x + b (x0 = A / 3 on these two curves' Montgomery twins)
    A = {"WEI25519": 486662, "WEI448": 156326}[curve]
    x0 = next(x for x in (A * pow(3, p - 2, p) % p, (-A) * pow(3, p - 2, p) % p) if (x * x * x + a * x + b) % p == 0)
    T2 = (x0, 0)
    pts = [G0]
    for _ in range(6):
        pts.append(aff_add(pts[-1], G0, a, p))
    cases = []
    for i in range(1, 6):
        cases.append((pts[i], pts[i - 1]))                 # generic pairs
    cases += [(pts[2], pts[2]), (pts[3], (pts[3][0], p - pts[3][1])), (None, pts[1]), (pts[1], None), (None, None),
              (T2, T2), (pts[1], T2)]
    Q = aff_add(pts[4], T2, a, p)
    cases += [(pts[4], Q), (Q, pts[4])]                    # exceptional: the difference has order two
    for n, (P, Q) in enumerate(cases):
        PP, QQ = proj(P), proj(Q)
        out, flags = yield Rec(f, "rcb", [limbs(PP), limbs(QQ)], 0, n >= 5)
        exp = rcb_add_py(PP, QQ, a, b, p)
        assert got(list(out)) == exp, (curve, P, Q)
        assert flags == (1 if exp[1] == 0 else 0) | (2 if exp[2] == 0 else 0)
        in_class(list(out))
        if P is not None and Q is not None and P != Q and (P[0] != Q[0]) and aff_add(P, (Q[0], p - Q[1]), a, p) != T2:
            R = aff_add(P, Q, a, p)
            zi = pow(exp[2], p - 2, p)
            assert (exp[0] * zi % p, exp[1] * zi % p) == R
        out2, _ = yield Rec(f, "rcb", [limbs(PP), limbs(PP)], 1, n >= 5)
        assert got(list(out2)) == rcb_dbl_py(PP, a, b, p)
        in_class(list(out2))
    # the exceptional pairs do give (0 : 0 : 0)
    e = rcb_add_py(proj(pts[4]), proj(aff_add(pts[4], T2, a, p)), a, b, p)
    assert e == (0, 0, 0)


# ---- lift_x_even (test_lift_x_even) ----
def iso_u(p, a):
    """u with a u^4 = -3 mod p (p = 3 mod 4), or None: the isomorphism ecamd_host.cpp:upload_g29 looks for (the brainpool r1 curves have one)"""
    t = (p - 3) * pow(a, -1, p) % p                  # u^4
    for s2 in (1, -1):
        r = pow(t, (p + 1) // 4, p)                   # a square root of t, if any
        if r * r % p != t:
            return None
        r = r * s2 % p
        u = pow(r, (p + 1) // 4, p)
        if u * u % p == r:
            return u
    return None


def lift_x(f, u=None):
    """jacg::lift_x_even -- BIP0340's lift_x as the Schnorr multi-scalar multiplication runs it on the device (k_msm_table_g, r_fmt 1): for
    p = 3 mod 4, x < p, y = (x^3 + a x + b)^((p + 1) / 4) with the square test, and the root that is EVEN ON THE ORIGINAL CURVE also when the
    unit computes on the isomorphic a = -3 image (the parity goes through the export factor ey); every flavour's own multiplication.
    f: the Field of the (isomorphic, when u is given) image."""
    c = CURVES[f.curve]
    p, a, b = c["p"], c["a"], c["b"]
    assert p % 4 == 3
    rng = np.random.default_rng(31 + f.flavour)
    nw = (f.pb + 31) // 32
    xs = [c["gx"], 0, 1, 2, p - 1, p - 2] + [int.from_bytes(rng.bytes(80), "big") % p for _ in range(60)]
    n_ok = 0
    for n, x in enumerate(xs + [p, p + 1, (1 << (32 * nw)) - 1]):
        assert x < 1 << (32 * nw)
        xw = [(x >> (32 * k)) & 0xffffffff for k in range(nw)]
        out, ok = yield Rec(f, "liftx", [xw], None, n < 6 or n >= len(xs))
        rhs = (x * x * x + a * x + b) % p
        y = pow(rhs, (p + 1) // 4, p)
        want = x < p and y * y % p == rhs
        assert bool(ok) == want, (f.curve, f.flavour, hex(x))
        if not want:
            continue
        n_ok += 1
        y = y if y % 2 == 0 else p - y
        xo, yo = f.val(out[:f.nl]), f.val(out[f.nl:])
        assert xo < 2 * p and yo < 2 * p and max(out[:f.nl - 1]) <= f.MASK + (1 << 18)     # a multiplication result of the unit
        uu = u if u is not None else 1
        assert xo * f.Rinv % p == x * uu * uu % p, (f.curve, f.flavour, hex(x))               # the unit's (Montgomery / plain) form of u^2 x
        assert yo * f.Rinv % p == y * uu**3 % p, (f.curve, f.flavour, hex(x))                 # ... of u^3 y_even
    assert 20 <= n_ok <= len(xs)


# ---- what a unit runs: the generators of one (object, curve) pair, and how many records each operation must see ----
SPARSE_TAGS = ("384n", "224s", "192s")
PLAIN_FLAVOURS = (1, 2, 4, 5)
MUL_WORD = {"255c": (121665, 1 << 17, (1,)), "448g": (39081, 1 << 10, (1, 9))}


def generators(lib, tag, curve, flavour):
    """[(name, factory)]: every factory gives a fresh generator of the unit `tag` (the object the headers were compiled as) on
    `curve`; flavour: the layout of the curve image (tools/g29_consts.py)"""
    f = Field(lib, curve, flavour)
    gens = [("field", lambda: field_ops(f, flavour)), ("jacobian", lambda: jacobian(f, flavour))]
    if tag in SPARSE_TAGS:
        gens.append(("sparse", lambda: sparse_small_products(f)))
    if tag in MUL_WORD:
        gens.append(("mulword", lambda: mul_word(f, flavour, *MUL_WORD[tag])))
        gens.append(("rcb", lambda: complete_formulas(f)))
    if f.p % 4 == 3:
        gens.append(("liftx", lambda: lift_x(f)))
        u = iso_u(f.p, f.a) if flavour == 0 and f.a not in (0, f.p - 3) else None
        if u is not None:
            fu = Field(lib, curve, flavour, u)
            gens.append(("liftx_iso", lambda: lift_x(fu, u)))
    return f, gens


def min_records(f, tag, flavour, names):
    """records per operation the host test runs on such a unit (counted on the parent of the commit that introduced this module);
    a generator that drops records falls below it"""
    m = {"mul": 120 + (400 if tag in SPARSE_TAGS else 0), "canon": 7 + (15 if flavour in PLAIN_FLAVOURS else 0), "neg": 7, "inv": 1,
         "dbl": 18, "add": 8}
    if f.infot()[0]:
        m.update(madd=15, dblt=7)
    if tag in MUL_WORD:
        m.update(mulword=40, rcb=28)
    n_lift = sum(1 for n in names if n.startswith("liftx"))
    if n_lift:
        m["liftx"] = 69 * n_lift
    return m


def check_counts(f, tag, flavour, done_by_name):
    """done_by_name: {generator name: [(rec, out, r)]}.  Returns {op: count} after asserting the minimum per operation"""
    counts = collections.Counter(rec.op for done in done_by_name.values() for rec, _, _ in done)
    want = min_records(f, tag, flavour, list(done_by_name))
    assert set(counts) == set(want), (sorted(counts), sorted(want))
    for op, n in want.items():
        assert counts[op] >= n, (tag, f.curve, op, counts[op], n)
    return dict(counts)
