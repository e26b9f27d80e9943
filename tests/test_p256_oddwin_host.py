"""CPU tests of the odd-window secp256r1 pipeline (libecc_amd/csrc/ecamd_p256.h): the co-Z doubling / addition (dblu,
zaddu), the odd-multiple table chain with its back-substitution, the regular odd-digit recoding (recode_odd) and a host
run of the window ladder, all against Python integers through tests/p256_oddwin_host_shim.cpp (g++, no HIP), plus the
per-item MAD count of the pipeline (-DECAMD_COUNT_MADS)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import u29_consts as K  # noqa: E402

W, MASK, p, R = K.W, K.MASK, K.p, K.R
Rinv = pow(R, p - 2, p)
q = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
G = (0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296,
     0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5)
BUILD = os.path.join(ROOT, "tests", "_build")
SHIM = os.path.join(ROOT, "tests", "p256_oddwin_host_shim.cpp")
M_MADS, S_MADS = 117, 81


def _build(name, flags):
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so] + flags + [SHIM])
    lib = C.CDLL(so)
    lib.t_mads.restype = C.c_uint64
    lib.t_table_mads.restype = C.c_uint64
    return lib


# the header's recoding and chain are generic in the window width: 4 is what the kernels use (ecamd_p256_kernel.hip: ODD_WB), 5 the
# width profiles/r7_odd_windows.md measured
@pytest.fixture(scope="module", params=[4, 5])
def lib(request):
    return _build(f"p256_oddwin_host_w{request.param}.so", [f"-DSHIM_WB={request.param}"])


@pytest.fixture(scope="module", params=[4, 5])
def counting(request):
    return _build(f"p256_oddwin_host_count_w{request.param}.so", ["-DECAMD_COUNT_MADS", f"-DSHIM_WB={request.param}"])


def limbs(x, n=9):
    d = [(x >> (W * i)) & MASK for i in range(n - 1)]
    d.append(x >> (W * (n - 1)))
    return d


def val(l):
    return sum(int(v) << (W * i) for i, v in enumerate(l))


def arr(l, t=C.c_uint32):
    return (t * len(l))(*l)


def loose(rng, v, lb, tb):
    """a representation of v with limbs pushed up towards lb (top limb <= tb)"""
    l = limbs(v)
    for i in range(8):
        room = (lb - l[i]) >> W
        k = min(room, l[i + 1], int(rng.integers(0, 8)))
        l[i] += k << W
        l[i + 1] -= k
    assert val(l) == v and max(l[:8]) <= lb and l[8] <= tb
    return l


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
    k %= q
    while k:
        if k & 1:
            Rr = aff_add(Rr, P)
        P = aff_add(P, P)
        k >>= 1
    return Rr


def mont(x):
    return x * R % p


def unmont(l):
    return val(l) * Rinv % p


def coz_aff(X, Y, Z):
    """affine point of Montgomery-domain Jacobian limbs X, Y and the plain integer Z (Montgomery form)"""
    z = Z * Rinv % p
    zi = pow(z, p - 2, p)
    return (unmont(X) * zi * zi % p, unmont(Y) * zi * zi * zi % p)


FXC = (MASK + 16, 2 << 24, 32)
FYC = (MASK + 16, (63 << 24) // 16, 63)


def rep(rng, v_mont, cls, top=False):
    """v (Montgomery residue) plus a multiple of p inside the class' value bound, limbs loosened up to the class' limb bound;
    top: the largest multiple that fits"""
    lb, tb, vb = cls
    kmax = (vb * p // 16 - v_mont) // p
    kmax = max(0, min(kmax, (tb << 232) // p))
    k = kmax if top else int(rng.integers(0, kmax + 1))
    while k >= 0:
        v = v_mont + k * p
        if (v >> 232) <= tb and v * 16 < vb * p:
            return loose(rng, v, lb, tb)
        k -= 1
    raise AssertionError("no representation")


def test_dblu_and_zaddu(lib):
    rng = np.random.default_rng(31)
    for it in range(30):
        P = aff_mul(int(rng.integers(1, 2**62)), G)
        # dblu: inputs are multiplication results < 17/16 p
        x = mont(P[0]) + (p if it % 2 and mont(P[0]) < p // 16 else 0)
        y = mont(P[1]) + (p if it % 3 == 0 and mont(P[1]) < p // 16 else 0)
        out = (C.c_uint32 * 45)()
        lib.t_dblu(arr(limbs(x)), arr(limbs(y)), out)
        o = list(out)
        Z = val(o[36:45])
        assert coz_aff(o[0:9], o[9:18], Z) == aff_add(P, P)
        assert coz_aff(o[18:27], o[27:36], Z) == P
        for k, cls in ((0, FXC), (9, FYC), (18, FXC), (27, FYC)):
            assert max(o[k:k + 8]) <= cls[0] and val(o[k:k + 9]) * 16 < cls[2] * p
        # zaddu on a random common Z, operands at random / extreme places of their classes
        Q = aff_mul(int(rng.integers(1, 2**62)), G)
        z = int(rng.integers(1, 2**62)) * 0x1234567 % p
        top = it % 5 == 0

        def at_z(Pt):
            return (mont(Pt[0] * z * z % p), mont(Pt[1] * z * z * z % p))
        Pm, Qm = at_z(P), at_z(Q)
        ins = [rep(rng, Pm[0], FXC, top), rep(rng, Pm[1], FYC, top), rep(rng, Qm[0], FXC, top), rep(rng, Qm[1], FYC, top)]
        lib.t_zaddu(*[arr(v) for v in ins], out)
        o = list(out)
        r = unmont(o[36:45])
        assert r == (unmont(ins[0]) - unmont(ins[2])) % p
        Z3 = mont(z * r % p)
        assert coz_aff(o[0:9], o[9:18], Z3) == aff_add(P, Q)
        assert coz_aff(o[18:27], o[27:36], Z3) == P
        for k, cls in ((0, FXC), (9, FYC), (18, FXC), (27, FYC)):
            assert max(o[k:k + 8]) <= cls[0] and val(o[k:k + 9]) * 16 < cls[2] * p


def test_table_chain_gives_odd_multiples(lib):
    wb = lib.t_wb()
    ne = 1 << (wb - 1)
    rng = np.random.default_rng(32)
    for it in range(6):
        P = aff_mul(int(rng.integers(1, 2**62)) if it else 1, G)
        tab = (C.c_uint32 * (18 * ne))()
        lib.t_table_odd(arr(limbs(mont(P[0]))), arr(limbs(mont(P[1]))), tab)
        t = list(tab)
        for j in range(ne):
            x, y = val(t[18 * j:18 * j + 9]), val(t[18 * j + 9:18 * j + 18])
            assert x < p and y < p and (x * Rinv % p, y * Rinv % p) == aff_mul(2 * j + 1, P)


def words(k, n):
    return [(k >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def digits_of(lib, k, nkw, slen):
    d = (C.c_int32 * 160)()
    t = lib.t_digits(arr(words(k, nkw)), nkw, slen, d)
    return list(d)[:t]


EDGE = [0, 1, 2, 3, q - 2, q - 1, q, q + 1, 2**256 - 1, 2**255, 2**256 - 2]


def test_recode_odd(lib):
    wb = lib.t_wb()
    rng = np.random.default_rng(33)
    cases = [(k, 8, 32) for k in EDGE]
    cases += [(int.from_bytes(rng.bytes(32), "big"), 8, 32) for _ in range(40)]
    for slen in (1, 5, 16, 31):
        cases += [(int.from_bytes(rng.bytes(slen), "big"), 8, slen) for _ in range(5)] + [(0, 8, slen), (2**(8 * slen) - 1, 8, slen)]
    for slen in (33, 40, 48, 64, 67, 68):
        cases += [(int.from_bytes(rng.bytes(slen), "big"), 17, slen) for _ in range(5)]
        cases += [(2**(8 * slen) - 1, 17, slen), (2**(8 * slen) - 2, 17, slen), (0, 17, slen), (q, 17, slen)]
    for k, nkw, slen in cases:
        d = digits_of(lib, k, nkw, slen)
        kp = k if k & 1 else k + q
        t = -(-(max(8 * slen, 256) + 1) // wb) if nkw == 17 else -(-257 // wb)
        assert len(d) == t
        assert all(x % 2 == 1 and abs(x) < 2**wb for x in d)
        assert d[0] > 0
        acc = 0
        for x in d:
            acc = (acc << wb) + x
        assert acc == kp, (hex(k), nkw, slen)


def ladder(lib, tab, k, nkw, slen):
    out = (C.c_uint32 * 27)()
    bad = lib.t_ladder_odd(tab, arr(words(k, nkw)), nkw, slen, out)
    o = list(out)
    return bad, coz_aff(o[0:9], o[9:18], val(o[18:27])) if unmont(o[18:27]) else None


def test_host_ladder(lib):
    wb = lib.t_wb()
    ne = 1 << (wb - 1)
    rng = np.random.default_rng(34)
    P = aff_mul(int(rng.integers(1, 2**62)), G)
    tab = (C.c_uint32 * (18 * ne))()
    lib.t_table_odd(arr(limbs(mont(P[0]))), arr(limbs(mont(P[1]))), tab)
    ks = [(int.from_bytes(rng.bytes(32), "big") % q, 8, 32) for _ in range(4)] + [(1, 8, 32), (2, 8, 32), (q - 1, 8, 32), (0xBEEF, 8, 2)]
    ks += [(int.from_bytes(rng.bytes(68), "big"), 17, 68), (int.from_bytes(rng.bytes(40), "big"), 17, 40)]
    for k, nkw, slen in ks:
        bad, Q = ladder(lib, tab, k, nkw, slen)
        assert bad == 0 and Q == aff_mul(k, P), hex(k)
    # exceptional pairs: the last addition is P + (-P) when k' = 0 (mod q) and P + P when k' = 2 d (mod q) for the last digit d:
    # flagged (the kernel's ECAMD_STATUS_REDO), never a wrong point
    for k in (0, q, 2 * q):
        assert ladder(lib, tab, k, 17 if k >= 2**256 else 8, 33 if k >= 2**256 else 32)[0] == 1, hex(k)
    if wb == 4:
        assert digits_of(lib, q - 2, 8, 32)[-1] == -1 and ladder(lib, tab, q - 2, 8, 32)[0] == 1  # k' = q - 2 = 2 d0 mod q, below q
    flagged = 0
    for d in range(-(2**wb - 1), 2**wb, 2):
        for k in ((2 * d) % q, (2 * d) % q + q):
            bad, Q = ladder(lib, tab, k, 17 if k >= 2**256 else 8, 33 if k >= 2**256 else 32)
            assert bad == 1 or Q == aff_mul(k, P), hex(k)
            flagged += bad
    assert flagged >= 1


def test_mad_counts(counting):
    """per-item MADs of the odd-window pipeline, as DESIGN.md section 2.1 quotes them (w = 4: 64 x (4 dbl + 1 madd) in the loop,
    dblu + 7 zaddu with their Z updates and 7 back-substitution steps in the table and affine kernels; w = 5: 51 windows, 15
    entries)"""
    wb = counting.t_wb()
    ne = 1 << (wb - 1)
    P = aff_mul(0xC0FFEE, G)
    x, y = arr(limbs(mont(P[0]))), arr(limbs(mont(P[1])))
    tm = counting.t_table_mads(x, y)
    nm = 3 + (ne - 1) * 5 + (ne - 1) * 4 - 1
    ns = 3 + (ne - 1) * 2 + (ne - 1) * 1
    assert tm == nm * M_MADS + ns * S_MADS
    tab = (C.c_uint32 * (18 * ne))()
    counting.t_table_odd(x, y, tab)
    counting.t_mads_reset()
    out = (C.c_uint32 * 27)()
    counting.t_ladder_odd(tab, arr(words(2**255 + 12345, 8)), 8, 32, out)
    t = -(-257 // wb)
    assert counting.t_mads() == (t - 1) * (wb * (4 * M_MADS + 4 * S_MADS) + 8 * M_MADS + 3 * S_MADS)
    assert (tm, counting.t_mads()) == {4: (9549, 278208), 5: (19917, 262089)}[wb]
