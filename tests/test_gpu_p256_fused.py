"""GPU tests of the secp256r1 kernels whose doublings form Y3 through one two-product Montgomery reduction (ecamd_p256.h: dbl with
u29::mul2; madd as well in a -DP256_FUSED_Y3_MADD=1 build): variable-base scalar multiplication (k_p256_loop_odd, KW = 8 and 17, public and masked mode), the fixed-base comb and
the interleaved ECDSA verification loop, byte for byte against the CPU oracle.  Sizes: one item, one wave, one wave and one item,
and 4099 (several blocks, no multiple of the eight items that share an inversion)."""
import numpy as np
import pytest

from oracles import CURVES, Oracle
from test_gpu_parity import make_sigs, rand_bytes

pytestmark = pytest.mark.gpu
CURVE = "SECP256R1"
SIZES = [1, 64, 65, 4099]


@pytest.fixture(scope="module")
def p256(gpu_ctx):
    cv = gpu_ctx.curve(CURVE)
    yield cv
    cv.free()


@pytest.fixture(scope="module")
def oracle():
    return Oracle(CURVE)


def special_scalars():
    q = CURVES[CURVE]["q"]
    ks = [3, 0, 1, 2, q - 2, q - 1, q, q + 1, (1 << 256) - 1]
    # the last digit's exceptional pairs of the odd recoding (k' = 2d), which come back through the complete-formula kernel
    return ks + [6, q + 6, q - 6, 10, q - 10]


def make_case(o, n, slen, seed):
    """(scalars, points): the special scalars against G, -G and a random point, then random scalars against random points with G
    and -G strewn in"""
    rng = np.random.default_rng(seed)
    p = CURVES[CURVE]["p"]
    g, st = o.scalar_mult((1).to_bytes(32, "big"))
    assert set(st) == {0}
    neg_g = g[:32] + (p - int.from_bytes(g[32:], "big")).to_bytes(32, "big")
    rnd, st = o.scalar_mult(rand_bytes(rng, 32 * n))
    assert set(st) == {0}
    sp = special_scalars()
    rsc = rand_bytes(rng, slen * n)
    sc, pts = [], []
    for i in range(n):
        if i < 3 * len(sp):
            sc.append(sp[i % len(sp)].to_bytes(slen, "big"))
            which = i // len(sp)
        else:
            sc.append(rsc[slen * i:slen * i + slen])
            which = 2 if i % 5 else (i // 5) % 2
        pts.append((g, neg_g, rnd[64 * i:64 * i + 64])[which])
    return b"".join(sc), b"".join(pts)


@pytest.mark.parametrize("slen", [32, 40])
@pytest.mark.parametrize("n", SIZES)
def test_variable_base_public_and_masked(gpu_ctx, p256, oracle, n, slen):
    """slen = 40 runs the KW = 17 loop"""
    sc, pts = make_case(oracle, n, slen, 240 + n + slen)
    exp = oracle.scalar_mult(sc, pts, slen)
    assert p256.scalar_mult(sc, pts, slen) == exp
    gpu_ctx.set_secret_scalars(True)
    try:
        assert p256.scalar_mult(sc, pts, slen) == exp
    finally:
        gpu_ctx.set_secret_scalars(False)


@pytest.mark.parametrize("n", SIZES)
def test_fixed_base_comb(gpu_ctx, p256, oracle, n):
    sc, _ = make_case(oracle, n, 32, 250 + n)
    exp = oracle.scalar_mult(sc)
    assert p256.scalar_mult(sc) == exp
    gpu_ctx.set_secret_scalars(True)
    try:
        assert p256.scalar_mult(sc) == exp
    finally:
        gpu_ctx.set_secret_scalars(False)


def test_ecdsa_verification_batch_257(p256):
    """k_p256_verify_loop: valid signatures, and damaged signatures, digests and public keys"""
    rng = np.random.default_rng(260)
    n = 257
    o, pubs, sigs, dg, hl, _ = make_sigs(CURVE, "SHA256", n, rng)
    pubs, sigs, dg = bytearray(pubs), bytearray(sigs), bytearray(dg)
    for i in range(0, n, 5):
        sigs[64 * i + (i % 64)] ^= 1 << (i % 8)
    for i in range(1, n, 17):
        dg[hl * i + 3] ^= 0x40
    for i in range(2, n, 31):
        pubs[64 * i + 40] ^= 2  # off the curve
    pubs, sigs, dg = bytes(pubs), bytes(sigs), bytes(dg)
    exp = o.ecdsa_verify(pubs, sigs, dg, hl)
    assert exp[3] == 0 and exp[4] == 0 and exp[0] == 1 and exp[1] == 1 and exp[2] == 1
    assert p256.ecdsa_verify(pubs, sigs, dg, hl) == exp
