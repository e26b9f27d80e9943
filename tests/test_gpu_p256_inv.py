"""GPU tests of the shared field inversion of the secp256r1 fast path (k_p256_affine_coz and k_p256_finalize: one inv() for the
items of a lane): variable-base scalar multiplications byte for byte against the CPU oracle, status bytes included.  Rejected
points (never in a group's product), results at infinity and items that go back through the complete-formula kernel are planted
at the first and last items of the lanes' groups and in between, for every items-per-inversion setting the batch size selects."""
import numpy as np
import pytest

from oracles import CURVES, Oracle
from test_gpu_parity import rand_bytes

pytestmark = pytest.mark.gpu
CURVE = "SECP256R1"
Q, P = CURVES[CURVE]["q"], CURVES[CURVE]["p"]
EDGE_SCALARS = [0, 1, 2, Q - 2, Q - 1, Q]
N_EDGE = len(EDGE_SCALARS) + 2  # + a point off the curve, + a coordinate >= p


@pytest.fixture(scope="module")
def p256(gpu_ctx):
    cv = gpu_ctx.curve(CURVE)
    yield cv
    cv.free()


@pytest.fixture(scope="module")
def oracle():
    return Oracle(CURVE)


@pytest.fixture(scope="module")
def pool(oracle):
    """4097 valid points and as many random scalars, computed once and only read by the small-batch cases"""
    rng = np.random.default_rng(2910)
    pts, st = oracle.scalar_mult(rand_bytes(rng, 32 * 4097))
    assert set(st) == {0}
    return pts, rand_bytes(rng, 32 * 4097)


def plant(sc, pts, i, kind):
    """edge item number `kind` at position i of the batch (bytearrays)"""
    if kind < len(EDGE_SCALARS):
        sc[32 * i:32 * i + 32] = EDGE_SCALARS[kind].to_bytes(32, "big")
    elif kind == len(EDGE_SCALARS):
        pts[64 * i + 63] ^= 1                                    # off the curve
    else:
        pts[64 * i:64 * i + 32] = (P + 5).to_bytes(32, "big")    # x >= p


def group_edges(n):
    """positions of the first and last items of a lane's group and their neighbours, for 2, 4 and 8 items per inversion: lane t
    of T = ceil(n / k) rounded up to 64 owns the items t, t + T, ..., t + (k - 1) T"""
    pos = {0, 1, n // 2, n - 2, n - 1}
    for k in (2, 4, 8):
        T = (((n + k - 1) // k) + 63) & ~63
        for j in range(1, k):
            pos |= {j * T - 1, j * T, j * T + 1, j * T + 63, j * T + 64}
    return sorted(x for x in pos if 0 <= x < n)


def planted_batch(sc, pts, n, rng):
    """plants every edge kind at the group edges of an n-item batch (in place); returns the planted positions"""
    pos = group_edges(n)
    # every kind at least once, and a rotation that moves each kind over the first / last places from batch to batch
    while len(pos) < 3 * N_EDGE and len(pos) < n:
        extra = int(rng.integers(0, n))
        if extra not in pos:
            pos.append(extra)
    for j, i in enumerate(pos):
        plant(sc, pts, i, (j + n) % N_EDGE)
    return pos


@pytest.mark.parametrize("n", [1, 63, 64, 65, 513, 4097])
def test_small_batches_every_item(gpu_ctx, p256, oracle, pool, n):
    rng = np.random.default_rng(2920 + n)
    if n == 1:
        # one item per batch: every edge kind and a plain item, each the whole group of its lane
        for kind in range(N_EDGE + 1):
            sc, pts = bytearray(pool[1][:32]), bytearray(pool[0][:64])
            if kind < N_EDGE:
                plant(sc, pts, 0, kind)
            assert p256.scalar_mult(bytes(sc), bytes(pts)) == oracle.scalar_mult(bytes(sc), bytes(pts))
        return
    sc, pts = bytearray(pool[1][:32 * n]), bytearray(pool[0][:64 * n])
    planted_batch(sc, pts, n, rng)
    exp = oracle.scalar_mult(bytes(sc), bytes(pts))
    assert {0, 1, 2} <= set(exp[1])  # fine, rejected and at infinity all occur
    assert p256.scalar_mult(bytes(sc), bytes(pts)) == exp


@pytest.mark.parametrize("n", [(1 << 17) + 65, (1 << 19) + 65])
def test_large_batches_sample(p256, oracle, n):
    """the other two items-per-inversion settings: a seeded 2048-item sample and every planted item against the oracle"""
    rng = np.random.default_rng(2930 + n % 1000)
    pts, st = p256.scalar_mult(rand_bytes(rng, 32 * n))  # base points [t]G from the fixed-base path
    assert set(st) == {0}
    sc, pts = bytearray(rand_bytes(rng, 32 * n)), bytearray(pts)
    planted = planted_batch(sc, pts, n, rng)
    sc, pts = bytes(sc), bytes(pts)
    out, st = p256.scalar_mult(sc, pts)
    idx = sorted(set(planted) | set(int(x) for x in rng.choice(n, size=2048, replace=False)))
    cut = lambda b, w: b"".join(b[w * i:w * i + w] for i in idx)
    exp = oracle.scalar_mult(cut(sc, 32), cut(pts, 64))
    assert {0, 1, 2} <= set(exp[1])
    assert (cut(out, 64), bytes(st[i] for i in idx)) == exp
    # whatever was not sampled: fine items only, none of them left at zero
    rest = np.frombuffer(st, dtype=np.uint8).copy()
    rest[planted] = 0
    assert not rest.any()
    assert np.frombuffer(out, dtype=np.uint8).reshape(n, 64).any(axis=1).sum() >= n - len(planted)


def test_fixed_base_ends_in_the_same_finalisation(p256, oracle, pool):
    n = 4097
    sc = bytearray(pool[1][:32 * n])
    for j, i in enumerate(group_edges(n)):
        sc[32 * i:32 * i + 32] = EDGE_SCALARS[j % len(EDGE_SCALARS)].to_bytes(32, "big")
    exp = oracle.scalar_mult(bytes(sc))
    assert {0, 2} <= set(exp[1])
    assert p256.scalar_mult(bytes(sc)) == exp


def test_masked_mode(gpu_ctx, p256, oracle, pool):
    n = 513
    rng = np.random.default_rng(2940)
    sc, pts = bytearray(pool[1][:32 * n]), bytearray(pool[0][:64 * n])
    planted_batch(sc, pts, n, rng)
    exp = oracle.scalar_mult(bytes(sc), bytes(pts))
    gpu_ctx.set_secret_scalars(True)
    try:
        assert p256.scalar_mult(bytes(sc), bytes(pts)) == exp
    finally:
        gpu_ctx.set_secret_scalars(False)
