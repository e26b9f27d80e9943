"""GPU tests of the secp256r1 odd-digit window path (k_p256_table_odd / k_p256_affine_coz / k_p256_loop_odd): variable-base
scalar multiplications against the CPU oracle, byte for byte, including the scalars that drive its last addition onto an
exceptional pair (k' = 0 or 2d mod q for the last digit d), which must come back through the complete-formula kernel."""
import numpy as np
import pytest

from oracles import CURVES, Oracle
from test_gpu_parity import rand_bytes

pytestmark = pytest.mark.gpu
CURVE = "SECP256R1"


@pytest.fixture(scope="module")
def p256(gpu_ctx):
    cv = gpu_ctx.curve(CURVE)
    yield cv
    cv.free()


def points(o, rng, n):
    pts, st = o.scalar_mult(rand_bytes(rng, 32 * n))
    assert set(st) == {0}
    return pts


def test_exceptional_pairs_of_the_odd_recoding(gpu_ctx, p256):
    o = Oracle(CURVE)
    q = CURVES[CURVE]["q"]
    rng = np.random.default_rng(61)
    ks = [0, q, q - 1, q + 1, 1, 2, (1 << 256) - 1]
    for d in range(-31, 32, 2):
        ks += [(2 * d) % q, (2 * d) % q + q, (q + 2 * d) % (1 << 256)]
    ks = [k % (1 << 256) for k in ks]
    sc = b"".join(k.to_bytes(32, "big") for k in ks)
    pts = points(o, rng, len(ks))
    exp = o.scalar_mult(sc, pts)
    assert 2 in exp[1]
    assert p256.scalar_mult(sc, pts) == exp
    gpu_ctx.set_secret_scalars(True)
    try:
        assert p256.scalar_mult(sc, pts) == exp
    finally:
        gpu_ctx.set_secret_scalars(False)


@pytest.mark.parametrize("slen", [1, 2, 5, 16, 31, 32, 33, 40, 64, 68])
def test_scalar_lengths_even_and_odd(gpu_ctx, p256, slen):
    o = Oracle(CURVE)
    rng = np.random.default_rng(62 + slen)
    n = 96
    sc = bytearray(rand_bytes(rng, slen * n))
    for j in range(n):  # half even, half odd
        last = slen * j + slen - 1
        sc[last] = (sc[last] & 0xFE) | (j & 1)
    sc = bytes(sc) + b"\xff" * slen + b"\x00" * slen + b"\x88" * slen
    pts = points(o, rng, n + 3)
    exp = o.scalar_mult(sc, pts, slen)
    assert p256.scalar_mult(sc, pts, slen) == exp
    gpu_ctx.set_secret_scalars(True)
    try:
        assert p256.scalar_mult(sc, pts, slen) == exp
    finally:
        gpu_ctx.set_secret_scalars(False)


def test_random_items_2_16(p256):
    o = Oracle(CURVE)
    rng = np.random.default_rng(63)
    n = 1 << 16
    sc = rand_bytes(rng, 32 * n)
    pts = points(o, rng, n)
    assert p256.scalar_mult(sc, pts) == o.scalar_mult(sc, pts)
