"""GPU tests of the 64-digit signed odd recoding of the secp256r1 variable-base path (k_p256_loop_odd<8, MASKED> over
recode_odd64): byte for byte against the CPU oracle, status bytes included, in plain and in masked mode."""
import numpy as np
import pytest

from oracles import CURVES, Oracle
from test_gpu_parity import rand_bytes

pytestmark = pytest.mark.gpu
CURVE = "SECP256R1"
Q = CURVES[CURVE]["q"]


@pytest.fixture(scope="module")
def p256(gpu_ctx):
    cv = gpu_ctx.curve(CURVE)
    yield cv
    cv.free()


@pytest.fixture(scope="module")
def oracle():
    return Oracle(CURVE)


def points(o, rng, n):
    pts, st = o.scalar_mult(rand_bytes(rng, 32 * n))
    assert set(st) == {0}
    return pts


def both_modes(ctx, cv, o, sc, pts, slen=32):
    exp = o.scalar_mult(sc, pts, slen)
    assert cv.scalar_mult(sc, pts, slen) == exp
    ctx.set_secret_scalars(True)
    try:
        assert cv.scalar_mult(sc, pts, slen) == exp
    finally:
        ctx.set_secret_scalars(False)
    return exp


def test_edge_scalars(gpu_ctx, p256, oracle):
    ks = list(range(64)) + list(range(Q - 32, Q + 33)) + list(range(2**256 - 32, 2**256)) + [2**255 - 1, 2**255, 2**255 + 1]
    sc = b"".join(k.to_bytes(32, "big") for k in ks)
    pts = points(oracle, np.random.default_rng(71), len(ks))
    _, st = both_modes(gpu_ctx, p256, oracle, sc, pts)
    assert st[ks.index(0)] == 2 and st[ks.index(Q)] == 2  # at infinity, through the complete-formula kernel


def test_random_scalars_half_even(gpu_ctx, p256, oracle):
    rng = np.random.default_rng(72)
    n = 256
    sc = bytearray(rand_bytes(rng, 32 * n))
    for j in range(0, n, 2):
        sc[32 * j + 31] &= 0xFE
    both_modes(gpu_ctx, p256, oracle, bytes(sc), points(oracle, rng, n))


@pytest.mark.parametrize("slen", [1, 16, 31, 32])
def test_scalar_lengths(gpu_ctx, p256, oracle, slen):
    rng = np.random.default_rng(73 + slen)
    n = 64
    sc = bytearray(rand_bytes(rng, slen * n))
    for j in range(n):  # half even, half odd
        last = slen * j + slen - 1
        sc[last] = (sc[last] & 0xFE) | (j & 1)
    sc = bytes(sc) + b"\xff" * slen + b"\x00" * slen + b"\xfe" * slen
    both_modes(gpu_ctx, p256, oracle, sc, points(oracle, rng, n + 3), slen)
