"""CPU tests of batched ECDSA public-key recovery: the recorded reference verdicts (tests/golden/ecdsa_recover.json), the
field-level steps of libecc_amd/csrc/ecamd_recover.h against Python integers through tests/recover_host_shim.cpp (g++, no
HIP), and the two new symbols in header, binding and library."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libecc_amd
import oracles as O
import recover_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ecdsa_recover.json")
BUILD = os.path.join(ROOT, "tests", "_build")
SHIM = os.path.join(ROOT, "tests", "recover_host_shim.cpp")
SYMBOLS = ["ec_ecdsa_recover_batch", "ec_ecdsa_recover_batch_dev"]
PRIMES = [(1 << 61) - 1, (1 << 31) - 1, 0x3FFFFFFFFFFFFFC7, 1000003, 13]   # 2^62 - 57 is prime


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_has_every_family_on_every_curve():
    fx = load_fixture()
    assert sorted(fx) == sorted(RR.CURVES)
    for curve, items in fx.items():
        c = O.CURVES[curve]
        fams = {i["family"] for i in items}
        assert set(RR.FAMILIES) <= fams, (curve, fams)
        assert ("r_geq_p" in fams) == (c["q"] > c["p"]), curve
        assert sum(i["family"] == "honest" for i in items) == 16
        ql, cl = O.qlen(curve), O.clen(curve)
        for i in items:
            assert len(i["sig"]) == 4 * ql and i["ret"] in (0, -1)
            assert (i["key1"] is None) == (i["ret"] == -1) == (i["key2"] is None)
            for k in (i["key1"], i["key2"]):
                assert k is None or k == "infinity" or len(k) == 4 * cl
        # what the issue pins: an r that is no abscissa, r / s out of range and r >= p all return -1; the redo family returns 0 with
        # exactly one key at infinity; digests of 20, 32, 48 and 64 bytes are there
        for i in items:
            if i["family"] in ("not_abscissa", "r_geq_p"):
                assert i["ret"] == -1, (curve, i)
            if i["family"] == "redo":
                assert i["ret"] == 0 and [i["key1"], i["key2"]].count("infinity") == 1, (curve, i)
        assert {len(i["digest"]) // 2 for i in items if i["family"] == "digest_len"} == {20, 32, 48, 64}
        if curve in RR.PRIME_ORDER:
            for i in items:
                if i["family"] in ("honest", "digest_len"):
                    assert i["ret"] == 0 and i["signer"] in (i["key1"], i["key2"]), (curve, i)


def test_fixture_is_what_the_reference_says_now():
    if not O.have_ref():
        pytest.skip("oracle/_ref/libecc_ref.so is not built here")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_recover_fixture as M
    with open(FIXTURE) as f:
        assert M.dumps(M.build()) == f.read()


@pytest.fixture(scope="module")
def shim():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "recover_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SHIM])
    lib = C.CDLL(so)
    u64 = C.c_uint64
    lib.t_sums.argtypes = [u64] * 6 + [C.POINTER(u64)]
    lib.t_uv.argtypes = [u64] * 4 + [C.POINTER(u64)]
    lib.t_needs_redo.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
    lib.t_digest_window.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32)]
    lib.t_be_geq.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    return lib


def test_shared_denominator_sums_against_python_integers(shim):
    """A + B and A - B from one inverse of x_B - x_A against the chord of oracles.py_add (which needs no curve equation)"""
    rng = np.random.default_rng(81)
    out = (C.c_uint64 * 4)()
    for m in PRIMES:
        for _ in range(300):
            xa, ya, xb, yb = (int(rng.integers(0, m)) for _ in range(4))
            if xa == xb:
                continue
            shim.t_sums(m, xa, ya, xb, yb, pow(xb - xa, -1, m), out)
            assert (out[0], out[1]) == O.py_add((xa, ya), (xb, yb), 0, m)
            assert (out[2], out[3]) == O.py_add((xa, ya), (xb, (-yb) % m), 0, m)
    # on a real curve: A = [3]G, B = [5]G over secp256k1's field would not fit 62 bits, so a toy curve y^2 = x^3 + 7 mod 1000003
    m, G = 1000003, None
    for x in range(1, 100):
        w = (x ** 3 + 7) % m
        if pow(w, (m - 1) // 2, m) == 1:
            G = (x, pow(w, (m + 1) // 4, m))
            break
    A, B = O.py_mul(3, G, 0, m), O.py_mul(5, G, 0, m)
    shim.t_sums(m, A[0], A[1], B[0], B[1], pow(B[0] - A[0], -1, m), out)
    assert (out[0], out[1]) == O.py_mul(8, G, 0, m) and (out[2], out[3]) == O.py_mul(2, (G[0], (-G[1]) % m), 0, m)


def test_u_v_against_python_integers(shim):
    rng = np.random.default_rng(82)
    out = (C.c_uint64 * 2)()
    for m in PRIMES:
        cases = [(int(rng.integers(0, m)), int(rng.integers(1, m)), int(rng.integers(1, m))) for _ in range(200)]
        cases += [(0, 1, 1), (0, m - 1, m - 1), (m - 1, 1, m - 1)]   # e = 0: u must be 0, not q
        for e, s, r in cases:
            rinv = pow(r, -1, m)
            shim.t_uv(m, e, s, rinv, out)
            assert out[0] == (-e * rinv) % m and out[1] == s * rinv % m


def test_digest_window_against_python_integers(shim):
    """e before its reduction mod q, for every fixture curve's order and digests shorter and longer than it (both shift branches)"""
    rng = np.random.default_rng(83)
    out = (C.c_uint32 * 17)()
    for curve in RR.CURVES:
        q = O.CURVES[curve]["q"]
        qbits, ql = q.bit_length(), O.qlen(curve)
        for hlen in (1, 20, 28, 29, 32, 33, 48, 64, 65, 66, 67, 128):
            for dg in (rng.integers(0, 256, size=hlen, dtype=np.uint8).tobytes(), b"\xff" * hlen, bytes(hlen)):
                shim.t_digest_window(dg, hlen, ql, qbits, out)
                got = sum(int(out[w]) << (32 * w) for w in range(17))
                e = int.from_bytes(dg, "big")
                if 8 * hlen > qbits:
                    e >>= 8 * hlen - qbits
                assert got == e and got < 2 * q, (curve, hlen)
                assert got % q == RR.digest_to_e(dg, q)


def test_r_against_p_with_unequal_lengths(shim):
    rng = np.random.default_rng(84)
    for alen, blen in ((29, 28), (28, 28), (32, 32), (66, 66), (28, 29), (1, 4)):
        for _ in range(200):
            a = int.from_bytes(rng.integers(0, 256, size=alen, dtype=np.uint8).tobytes(), "big") >> int(rng.integers(0, 8 * alen))
            b = int.from_bytes(rng.integers(0, 256, size=blen, dtype=np.uint8).tobytes(), "big") >> int(rng.integers(0, 8 * blen))
            for x, y in ((a, b), (b % (1 << (8 * alen)), b), (a, a % (1 << (8 * blen)))):
                assert shim.t_be_geq(x.to_bytes(alen, "big"), alen, y.to_bytes(blen, "big"), blen) == (1 if x >= y else 0)
    p, q = O.CURVES["SECP224K1"]["p"], O.CURVES["SECP224K1"]["q"]
    for r, want in ((p - 1, 0), (p, 1), (p + 1, 1), (q - 1, 1), (1, 0)):
        assert shim.t_be_geq(r.to_bytes(29, "big"), 29, p.to_bytes(28, "big"), 28) == want


def test_infinity_and_equal_abscissae_go_to_the_redo_pass(shim):
    OK, INF, REDO = 0, 2, 0xFE
    assert shim.t_needs_redo(OK, OK, 0) == 0
    assert shim.t_needs_redo(OK, OK, 1) == 1            # A = +-B: a doubling, or the point at infinity
    for sa, sb in ((INF, OK), (OK, INF), (INF, INF), (REDO, OK), (OK, REDO)):
        for same in (0, 1):
            assert shim.t_needs_redo(sa, sb, same) == 1


def test_header_binding_and_library_have_the_recovery_calls():
    with open(os.path.join(ROOT, "include", "libecc_amd.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = libecc_amd.load_library()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in libecc_amd.EXPORTED_SYMBOLS
        assert hasattr(L, name)
    assert len(L.ec_ecdsa_recover_batch.argtypes) == 10 and len(L.ec_ecdsa_recover_batch_dev.argtypes) == 11
    assert hasattr(libecc_amd.api.Curve, "ecdsa_recover") and hasattr(libecc_amd.api.Curve, "ecdsa_recover_dev")
