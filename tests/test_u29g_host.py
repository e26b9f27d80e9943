"""CPU tests of the generic radix-2^29 field / Jacobian code (ecamd_u29g.h, ecamd_jacg.h) for
every field size libecc's curves use: host build of the product headers (tests/u29g_host_shim.cpp)
against Python integers, with operands spread over their whole bound class.  The vectors and the
assertions on each of them live in tests/u29g_vectors.py, which tests/test_gpu_u29g_units.py runs
through the device build of the same headers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import u29g_vectors as V  # noqa: E402
from oracles import CURVES  # noqa: E402
from u29g_vectors import Field, arr, drive  # noqa: E402

BUILD = V.BUILD
CASES = ["SECP192R1", "SECP224R1", "WEI25519", "BRAINPOOLP256R1", "SECP256K1", "SECP256R1", "BRAINPOOLP320R1",
         "SECP384R1", "WEI448", "GOST512", "BRAINPOOLP512R1", "SECP521R1"]


@pytest.fixture(scope="module")
def lib():
    return V.host_lib("")


@pytest.fixture(scope="module")
def lib_m521():
    """the secp521r1 flavour (plain residues on 18 limbs, 2^522 = 2 folded inside the product columns) of the same headers"""
    return V.host_lib("_m521p", ["-DG29_M521P", "-DSHIM_ONLY_521"])


@pytest.fixture(scope="module")
def lib_p25519():
    """the 2^255 - 19 flavour (nine limbs, plain residues, pseudo-Mersenne folds) of the same headers"""
    return V.host_lib("_p25519", ["-DG29_P25519", "-DSHIM_ONLY_255"])


@pytest.mark.parametrize("curve", CASES)
def test_field_ops(lib, curve, flavour=0):
    f = Field(lib, curve, flavour)
    done = drive(V.field_ops(f, flavour))
    n = {op: sum(1 for rec, _, _ in done if rec.op == op) for op in ("mul", "canon", "neg", "inv")}
    assert n == {"mul": 120, "canon": 22 if flavour in V.PLAIN_FLAVOURS else 7, "neg": 7, "inv": 1}


@pytest.mark.parametrize("curve", CASES)
def test_jacobian(lib, curve, flavour=0):
    f = Field(lib, curve, flavour)
    done = drive(V.jacobian(f, flavour))
    n = {op: sum(1 for rec, _, _ in done if rec.op == op) for op in ("dbl", "add", "madd", "dblt")}
    assert n == ({"dbl": 18, "add": 8, "madd": 15, "dblt": 7} if f.infot()[0] else {"dbl": 18, "add": 8, "madd": 0, "dblt": 0})


def test_secp521r1_mersenne_flavour(lib_m521):
    test_field_ops(lib_m521, "SECP521R1", 1)
    test_jacobian(lib_m521, "SECP521R1", 1)


def _check_mul_word(lib, curve, flavour, cst, lazy, lazy_limbs):
    assert len(drive(V.mul_word(Field(lib, curve, flavour), flavour, cst, lazy, lazy_limbs))) == 40


def test_p25519_flavour(lib_p25519):
    test_field_ops(lib_p25519, "WEI25519", 2)
    test_jacobian(lib_p25519, "WEI25519", 2)
    _check_mul_word(lib_p25519, "WEI25519", 2, 121665, 1 << 17, (1,))


@pytest.fixture(scope="module")
def lib_n384():
    """secp384r1's flavour of the 384-bit unit: Montgomery reduction on the four signed digits of p + 1, signed column sums"""
    return V.host_lib("_n384", ["-DG29_P384S", "-DSHIM_ONLY_384"])


def _sparse_flavour_checks(lib, curve):
    test_field_ops(lib, curve)
    test_jacobian(lib, curve)
    assert len(drive(V.sparse_small_products(Field(lib, curve)))) == 400


def test_secp384r1_mpinv1_flavour(lib_n384):
    assert CURVES["SECP384R1"]["p"] == 2**384 - 2**128 - 2**96 + 2**32 - 1
    _sparse_flavour_checks(lib_n384, "SECP384R1")


def _sparse_lib(pb, flag):
    return V.host_lib(f"_s{pb}", [flag, f"-DSHIM_ONLY_{pb}"])


def test_secp224r1_sparse_flavour():
    """p = 2^224 - 2^96 + 1 = +1 mod 2^29: negated quotient digits, "+ m_k" clears the column, m_k (p - 1) as two signed MADs"""
    assert CURVES["SECP224R1"]["p"] == 2**224 - 2**96 + 1
    _sparse_flavour_checks(_sparse_lib(224, "-DG29_P224S"), "SECP224R1")


def test_secp192r1_sparse_flavour():
    """p = 2^192 - 2^64 - 1 = -1 mod 2^29: m_k (p + 1) as two signed MADs"""
    assert CURVES["SECP192R1"]["p"] == 2**192 - 2**64 - 1
    _sparse_flavour_checks(_sparse_lib(192, "-DG29_P192S"), "SECP192R1")


@pytest.fixture(scope="module")
def lib_k256():
    """the secp256k1 flavour (nine limbs, plain residues, folds with 2^256 = 2^32 + 977) of the 256-bit unit"""
    return V.host_lib("_k256", ["-DG29_K256", "-DSHIM_ONLY_256"])


def test_secp256k1_flavour(lib_k256):
    assert CURVES["SECP256K1"]["p"] == 2**256 - 2**32 - 977
    test_field_ops(lib_k256, "SECP256K1", 4)
    test_jacobian(lib_k256, "SECP256K1", 4)


@pytest.fixture(scope="module")
def lib_p448():
    """the Goldilocks flavour (16 limbs, plain residues, folds with 2^448 = 2^224 + 1) of the 448-bit unit"""
    return V.host_lib("_p448", ["-DG29_P448", "-DSHIM_ONLY_448"])


def test_p448_flavour(lib_p448):
    assert CURVES["WEI448"]["p"] == 2**448 - 2**224 - 1
    test_field_ops(lib_p448, "WEI448", 5)
    test_jacobian(lib_p448, "WEI448", 5)
    _check_mul_word(lib_p448, "WEI448", 5, 39081, 1 << 10, (1, 9))


def test_mad_counts_match_the_work_model():
    """bench.py prices a kernel by the MADs its field operations issue (`field_mads`: per multiplication, per squaring).  The host
    build of the same headers counts the MADs it really executes (-DECAMD_COUNT_MADS: every chain and every single MAD bumps a
    counter): the two must agree for every flavour, or the roofline fractions of the bench lines are wrong."""
    import importlib.util
    import types
    for name in ("torch", "libecc_amd"):          # bench.py imports them at module level; the model itself is pure Python
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)
    spec = importlib.util.spec_from_file_location("bench_for_model", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    os.makedirs(BUILD, exist_ok=True)
    rng = np.random.default_rng(7)
    cases = [("SECP192R1", 0, ["-DG29_P192S", "-DSHIM_ONLY_192"]), ("SECP224R1", 0, ["-DG29_P224S", "-DSHIM_ONLY_224"]), ("BRAINPOOLP192R1", 0, []),
             ("BRAINPOOLP224R1", 0, []), ("BRAINPOOLP256R1", 0, []), ("BRAINPOOLP320R1", 0, []), ("BRAINPOOLP384R1", 0, []),
             ("BRAINPOOLP512R1", 0, []), ("SECP384R1", 0, ["-DG29_P384S", "-DSHIM_ONLY_384"]), ("SECP521R1", 1, ["-DG29_M521P", "-DSHIM_ONLY_521"]),
             ("WEI25519", 2, ["-DG29_P25519", "-DSHIM_ONLY_255"]), ("SECP256K1", 4, ["-DG29_K256", "-DSHIM_ONLY_256"]),
             ("WEI448", 5, ["-DG29_P448", "-DSHIM_ONLY_448"])]
    libs = {}
    for curve, flavour, flags in cases:
        key = tuple(flags)
        if key not in libs:
            so = os.path.join(BUILD, "u29g_count_%s.so" % ("_".join(f[2:] for f in flags) or "dense"))
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DECAMD_COUNT_MADS"] + flags +
                                  ["-o", so, os.path.join(ROOT, "tests", "u29g_host_shim.cpp")])
            libs[key] = C.CDLL(so)
        lib = libs[key]
        lib.g_madcount_get.restype = C.c_uint64
        f = Field(lib, curve, flavour)
        nl, M, S, _ = bench.field_mads(f.p)
        assert nl == f.nl, (curve, nl, f.nl)
        x, y = (int.from_bytes(rng.bytes(80), "big") % f.p for _ in range(2))
        out = (C.c_uint32 * f.nl)()
        lib.g_madcount_reset()
        f.fn("mul")(f.k, arr(f.digits(x)), arr(f.digits(y)), out, 0)
        got_m = lib.g_madcount_get()
        lib.g_madcount_reset()
        f.fn("mul")(f.k, arr(f.digits(x)), arr(f.digits(x)), out, 1)
        got_s = lib.g_madcount_get()
        assert (got_m, got_s) == (M, S), (curve, "counted", got_m, got_s, "model", M, S)


@pytest.mark.parametrize("curve,flavour,fixture", [("WEI25519", 2, "lib_p25519"), ("WEI448", 5, "lib_p448")])
def test_complete_formulas_on_the_radix29_types(curve, flavour, fixture, request):
    """ecamd_rcbg.h against the Renes-Costello-Batina polynomials over Python integers (u29g_vectors.complete_formulas)"""
    lib = request.getfixturevalue(fixture)
    assert len(drive(V.complete_formulas(Field(lib, curve, flavour)))) == 28


@pytest.mark.parametrize("curve,flavour,fixture,iso", [
    ("SECP192R1", 0, "lib", False), ("SECP256R1", 0, "lib", False), ("SECP256K1", 0, "lib", False), ("SECP256K1", 4, "lib_k256", False),
    ("BRAINPOOLP256R1", 0, "lib", False), ("BRAINPOOLP256R1", 0, "lib", True), ("BRAINPOOLP320R1", 0, "lib", True), ("SECP384R1", 0, "lib", False),
    ("SECP384R1", 3, "lib_n384", False), ("WEI448", 5, "lib_p448", False), ("BRAINPOOLP512R1", 0, "lib", True), ("SECP521R1", 0, "lib", False),
    ("SECP521R1", 1, "lib_m521", False)])
def test_lift_x_even(curve, flavour, fixture, iso, request):
    """jacg::lift_x_even against Python integers (u29g_vectors.lift_x), also on the isomorphic a = -3 image"""
    lib = request.getfixturevalue(fixture)
    c = CURVES[curve]
    u = V.iso_u(c["p"], c["a"]) if iso else None
    assert (u is not None) == iso
    assert len(drive(V.lift_x(Field(lib, curve, flavour, u), u))) == 69


@pytest.mark.parametrize("name,tag,curve,flavour", V.UNITS, ids=[u[0] for u in V.UNITS])
def test_records_per_unit(name, tag, curve, flavour):
    """every unit the GPU test runs: all its generators against the g++ build, and no operation below the number of records the
    tests above run on such a unit (a generator that drops records would go unnoticed otherwise)"""
    lib = V.host_lib(V.HOST_NAME[tag], V.HOST_FLAGS[tag])
    f, gens = V.generators(lib, tag, curve, flavour)
    V.check_counts(f, tag, flavour, {n: drive(g()) for n, g in gens})
