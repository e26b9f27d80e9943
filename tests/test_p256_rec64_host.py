"""CPU tests of the 64-digit signed odd recoding of the secp256r1 fast path (recode_odd64, libecc_amd/csrc/ecamd_p256.h) and
of the 63-window ladder that k_p256_loop_odd<8, MASKED> runs over it, against Python integers through
tests/p256_rec64_host_shim.cpp (g++, no HIP), plus the ladder's MAD count (-DECAMD_COUNT_MADS)."""
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
SHIM = os.path.join(ROOT, "tests", "p256_rec64_host_shim.cpp")
M_MADS, S_MADS = 117, 81
FLAGGED = {0, 2, q - 2, q}


def _build(name, flags):
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so] + flags + [SHIM])
    lib = C.CDLL(so)
    lib.t_mads.restype = C.c_uint64
    return lib


@pytest.fixture(scope="module")
def lib():
    return _build("p256_rec64_host.so", [])


@pytest.fixture(scope="module")
def counting():
    return _build("p256_rec64_host_count.so", ["-DECAMD_COUNT_MADS"])


def _scalars():
    rng = np.random.default_rng(64)
    ks = list(range(64)) + list(range(q - 32, q + 33)) + list(range(2**256 - 32, 2**256))
    ks += [2**255 - 1, 2**255, 2**255 + 1]
    ks += [int.from_bytes(rng.bytes(32), "big") for _ in range(64)]
    for slen in (1, 5, 16, 31):
        ks += [int.from_bytes(rng.bytes(slen), "big") for _ in range(5)] + [0, 2**(8 * slen) - 1]
    return ks


SCALARS = _scalars()


def limbs(x, n=9):
    d = [(x >> (W * i)) & MASK for i in range(n - 1)]
    d.append(x >> (W * (n - 1)))
    return d


def val(l):
    return sum(int(v) << (W * i) for i, v in enumerate(l))


def arr(l, t=C.c_uint32):
    return (t * len(l))(*l)


def words(k):
    return [(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def jac_dbl(P):
    X, Y, Z = P
    if Z == 0:
        return P
    g = Y * Y % p
    b = 4 * X * g % p
    a = 3 * (X - Z * Z) * (X + Z * Z) % p
    x3 = (a * a - 2 * b) % p
    return (x3, (a * (b - x3) - 8 * g * g) % p, 2 * Y * Z % p)


def jac_add_aff(P, Q):
    X, Y, Z = P
    if Z == 0:
        return (Q[0], Q[1], 1)
    zz = Z * Z % p
    h = (Q[0] * zz - X) % p
    r = (Q[1] * zz * Z - Y) % p
    if h == 0:
        return jac_dbl(P) if r == 0 else (1, 1, 0)
    hh = h * h % p
    v = X * hh % p
    x3 = (r * r - hh * h - 2 * v) % p
    return (x3, (r * (v - x3) - Y * hh * h) % p, Z * h % p)


def aff_mul(k, P):
    """[k mod q]P as an affine pair, None at infinity"""
    k %= q
    acc = (1, 1, 0)
    for i in reversed(range(k.bit_length())):
        acc = jac_dbl(acc)
        if (k >> i) & 1:
            acc = jac_add_aff(acc, P)
    if acc[2] == 0:
        return None
    zi = pow(acc[2], p - 2, p)
    return (acc[0] * zi * zi % p, acc[1] * zi * zi * zi % p)


def mont(x):
    return x * R % p


def jac_aff(o):
    """affine point of 27 words of Montgomery-domain Jacobian limbs"""
    X, Y, Z = (val(o[9 * i:9 * i + 9]) * Rinv % p for i in range(3))
    if Z == 0:
        return None
    zi = pow(Z, p - 2, p)
    return (X * zi * zi % p, Y * zi * zi * zi % p)


def rule(k):
    """(k', sign) of the recoding"""
    if k & 1:
        return k, 0
    return (q - k, 1) if k < q else (k - q, 0)


def test_recode_odd64(lib):
    for k in SCALARS:
        d = (C.c_int32 * 64)()
        sign = lib.t_digits64(arr(words(k)), d)
        d = list(d)
        kp, s = rule(k)
        assert sign == s, hex(k)
        assert kp & 1 and 0 < kp < 2**256 and (kp if s == 0 else -kp) % q == k % q
        assert len(d) == 64 and all(x % 2 == 1 and abs(x) <= 15 for x in d), hex(k)
        assert d[0] > 0, hex(k)
        acc = 0
        for x in d:
            acc = (acc << 4) + x
        assert acc == kp, hex(k)


def test_host_ladder64(lib):
    rng = np.random.default_rng(65)
    P = aff_mul(int(rng.integers(1, 2**62)), G)
    tab = (C.c_uint32 * (18 * 8))()
    lib.t_table_odd(arr(limbs(mont(P[0]))), arr(limbs(mont(P[1]))), tab)
    out = (C.c_uint32 * 27)()
    flagged = set()
    for k in SCALARS:
        if lib.t_ladder64(tab, arr(words(k)), out):
            flagged.add(k)
        else:
            assert jac_aff(list(out)) == aff_mul(k, P), hex(k)
    assert flagged == FLAGGED


def test_mad_count(counting):
    """63 windows of 4 doublings (4M + 4S) and one mixed addition (8M + 3S): the figure DESIGN.md section 2.1 quotes"""
    P = aff_mul(0xC0FFEE, G)
    tab = (C.c_uint32 * (18 * 8))()
    counting.t_table_odd(arr(limbs(mont(P[0]))), arr(limbs(mont(P[1]))), tab)
    out = (C.c_uint32 * 27)()
    for k in (2**255 + 12345, 2**255 + 12344, 6):
        counting.t_mads_reset()
        counting.t_ladder64(tab, arr(words(k)), out)
        assert counting.t_mads() == 63 * (4 * (4 * M_MADS + 4 * S_MADS) + 8 * M_MADS + 3 * S_MADS) == 273861
