"""CPU tests of the secp256r1 field inversion (inv() of libecc_amd/csrc/ecamd_p256.h: constant-time divsteps): the header is
compiled for the host (tests/p256_inv_host.cpp, g++) as tests/test_u29_host.py does, and inv() is compared with Python's
pow(a, p - 2, p).  For every input the same program also reports the final f and g of the divstep run (g = 0 and f = +-1 for a
non-zero input: the fixed count was enough) and the number of divsteps it executed (always the fixed one)."""
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
BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "p256_inv_host.cpp")


@pytest.fixture(scope="module")
def lib():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "p256_inv_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    return C.CDLL(so)


def limbs(x):
    return [(x >> (W * i)) & MASK for i in range(8)] + [x >> (W * 8)]


def signed_val(l):
    return sum(int(v) << (W * i) for i, v in enumerate(l))


def run(lib, values):
    """values: integers below 2p (exact digits: the limbs of Fmul at most); checks every one, returns nothing"""
    n = len(values)
    a = np.array([limbs(v) for v in values], dtype=np.uint32)
    assert a[:, :8].max() <= MASK and a[:, 8].max() <= (2 << 24)
    out = np.zeros((n, 9), dtype=np.uint32)
    fg = np.zeros((n, 18), dtype=np.int32)
    steps = np.zeros(n, dtype=np.int32)
    lib.t_inv_batch(n, a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), fg.ctypes.data_as(C.c_void_p),
                    steps.ctypes.data_as(C.c_void_p))
    assert (steps == K.SAFEGCD_N * K.SAFEGCD_BATCHES).all()
    assert out[:, :8].max() <= MASK
    for i, v in enumerate(values):
        got = signed_val(out[i])
        # Montgomery domain in and out: v = a R  ->  a^-1 R = R^2 / v; inv(0) = 0
        assert got < 2 * p and got % p == pow(v, p - 2, p) * R * R % p, hex(v)
        f, g = signed_val(fg[i, :9]), signed_val(fg[i, 9:])
        assert g == 0, hex(v)
        if v % p:
            assert f in (1, -1), hex(v)
        else:
            assert got == 0 and f == p


def test_constants(lib):
    out = (C.c_uint32 * 12)()
    lib.t_inv_consts(out)
    assert list(out[0:9]) == limbs(K.SAFEGCD_E0) and K.SAFEGCD_E0 == R * R % p
    assert (out[9], out[10]) == (K.SAFEGCD_N, K.SAFEGCD_BATCHES)
    assert out[11] == 0, "the default build must run the divstep inversion"
    K.safegcd_checks()


def test_edge_values(lib):
    edge = [0, 1, 2, p - 1, p - 2, (p + 1) // 2, (p - 1) // 2, 2**255, (2**256 - 1) % p, R % p, R * R % p, R**3 % p]
    edge += [1 << k for k in range(256)] + [(1 << k) - 1 for k in range(2, 256)] + [p - (1 << k) for k in range(2, 255)]
    # the loosest form Fmul admits: the same residues as values in [p, 2p), and the largest value with every limb at its bound
    loose = [v + p for v in edge if v + p < 2 * p and limbs(v + p)[8] <= (2 << 24)]
    top = ((2 << 24) - 2 << (W * 8)) + (1 << (W * 8)) - 1
    assert top < 2 * p and limbs(top)[:8] == [MASK] * 8
    run(lib, edge + loose + [p, 2 * p - 1, top])


def test_random_values(lib):
    rng = np.random.default_rng(2901)
    raw = rng.integers(0, 256, size=(100000, 40), dtype=np.uint8)
    vals = [int.from_bytes(raw[i].tobytes(), "big") % (2 * p) for i in range(len(raw))]
    run(lib, vals)


def test_fermat_chain_agrees(lib):
    """the chain kept behind P256_INV_FERMAT gives the same residue"""
    rng = np.random.default_rng(2902)
    for _ in range(20):
        v = int.from_bytes(rng.bytes(40), "big") % (2 * p)
        out = (C.c_uint32 * 9)()
        lib.t_inv_fermat((C.c_uint32 * 9)(*limbs(v)), out)
        assert signed_val(out) % p == pow(v, p - 2, p) * R * R % p
    K.inv_chain()


def test_standalone_program():
    """the same source as a program of its own (the form that is built with -fsanitize=address,undefined): inv(x) x = 1 by the
    header's own multiplication, 10^5 random values and the edge cases"""
    exe = os.path.join(BUILD, "p256_inv_main")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DP256_INV_MAIN", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr
