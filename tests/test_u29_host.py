"""CPU tests of the radix-2^29 lazy-reduction field / Jacobian code (libecc_amd/csrc/ecamd_u29.h,
ecamd_p256.h): the product headers are compiled for the host (tests/u29_host_shim.cpp, g++) and
driven against Python integers, including operands sitting at the extreme of their declared bound
classes (the compile-time bound tracking must make those overflow-free).  The vectors and the
assertions on each of them live in tests/u29_vectors.py, which tests/test_gpu_u29_unit.py runs
through the device build of the same headers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import u29_consts as K  # noqa: E402
import u29_vectors as V  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    return V.host_lib()


def _count(done, **want):
    assert {op: sum(1 for rec, _, _ in done if rec.op == op) for op in want} == want and len(done) == sum(want.values())


def test_constants(lib):
    out, _ = V.call(lib.t_consts, n_out=49)
    V.check_consts(out)
    K.inv_chain()


def test_mul_sqr_random_and_extreme(lib):
    _count(V.drive(V.mul_sqr(), lib), mul=305, sqr=305, mul_loose=201)


def test_fold_and_canonical(lib):
    _count(V.drive(V.fold_canonical(), lib), fold=300, canonical_words=7, from_words=7, is_zero=11)


def test_inversion_chain(lib):
    _count(V.drive(V.inversion(), lib), inv=5)


def test_jacobian_dbl_add(lib):
    _count(V.drive(V.jacobian_dbl_add(), lib), dbl=40, add=42)


def test_mixed_addition(lib):
    _count(V.drive(V.mixed_addition(), lib), madd=82)


def test_jacobian_chain_stays_in_bounds(lib):
    """200 consecutive doublings/additions through the loop-carried classes"""
    _count(V.drive(V.jacobian_chain(), lib), dbl=160, add=40)
