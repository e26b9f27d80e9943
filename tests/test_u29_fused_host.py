"""CPU tests of the two-product Montgomery primitives (ecamd_u29.h: mul2, mulsqr) and of the Y3 formulas that go through them
(ecamd_p256.h: dbl, madd, add_jac).  tests/u29_fused_host_shim.cpp is compiled for the host with both switches
(P256_FUSED_Y3_DBL, P256_FUSED_Y3_MADD) set to 1 and with both set to 0 (the two-reduction formulas); both builds run the Jacobian vectors of
tests/u29_vectors.py against affine arithmetic in Python integers, and must agree with each other on every affine point."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import u29_vectors as V  # noqa: E402

p, R, Rinv, W, MASK = V.p, V.R, V.Rinv, V.W, V.MASK
SRC = os.path.join(ROOT, "tests", "u29_fused_host_shim.cpp")
ON = ["-DP256_FUSED_Y3_DBL=1", "-DP256_FUSED_Y3_MADD=1"]
OFF = ["-DP256_FUSED_Y3_DBL=0", "-DP256_FUSED_Y3_MADD=0"]
CLASSES = ("dbl_a", "dbl_b", "dbl_c", "dbl_d", "dbl_out", "madd_a", "madd_b", "madd_c", "madd_d", "madd_out", "sqr_c", "sqr_out")


def _build(name, flags, shared=True):
    os.makedirs(V.BUILD, exist_ok=True)
    out = os.path.join(V.BUILD, name)
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + (["-fPIC", "-shared"] if shared else []) + flags + ["-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def libs():
    on, off = C.CDLL(_build("u29_fused_on.so", ON)), C.CDLL(_build("u29_fused_off.so", OFF))
    assert on.t_fused_switches() == 3 and off.t_fused_switches() == 0
    return on, off


@pytest.fixture(scope="module")
def bounds(libs):
    o = (C.c_uint64 * (3 * len(CLASSES)))()
    libs[0].t_fused_bounds(o)
    return {name: tuple(int(v) for v in o[3 * i:3 * i + 3]) for i, name in enumerate(CLASSES)}


def _at_bounds(b):
    """every limb at LB, the top limb at TB"""
    return [b[0]] * 8 + [b[1]]


def _value_limit(b):
    """values of the class lie below VB p / 16, and below what its top-limb bound lets exact lower digits reach"""
    return min(b[2] * p // 16, (b[1] + 1) << (8 * W))


def _max_value(b):
    """the largest value the class admits (just under VB p / 16), on limbs as loose as LB and TB allow"""
    v = _value_limit(b) - 1
    l = V.limbs(v)
    for i in range(7, -1, -1):  # push as much as fits from limb i + 1 down into limb i
        k = min((b[0] - l[i]) >> W, l[i + 1])
        l[i] += k << W
        l[i + 1] -= k
    assert V.val(l) == v and max(l[:8]) <= b[0] and l[8] <= b[1]
    return l


def _random(rng, b):
    v = int.from_bytes(rng.bytes(40), "big") % _value_limit(b)
    return V.loose(rng, v, b[0], b[1])


def _operands(rng, bs, n):
    """operand tuples: all at the limb bounds, all at the largest value, each alone at its limb bounds, then random ones"""
    yield [_at_bounds(b) for b in bs], False
    yield [_max_value(b) for b in bs], True
    for k in range(len(bs)):
        yield [_at_bounds(b) if i == k else _max_value(b) for i, b in enumerate(bs)], False
    for _ in range(n):
        yield [_random(rng, b) for b in bs], True


def _check(out, want, bout, in_value_bounds):
    assert V.val(out) % p == want % p
    assert max(out[:8]) <= MASK  # exact low digits: is_zero_mulout, canonical and weaken rely on them
    if in_value_bounds:
        assert V.val(out) * 16 < bout[2] * p and out[8] <= bout[1]


@pytest.mark.parametrize("site", ["dbl", "madd"])
def test_mul2_random_and_extreme(libs, bounds, site):
    rng = np.random.default_rng(31 if site == "dbl" else 32)
    bs = [bounds[f"{site}_{x}"] for x in "abcd"]
    for lib in libs:  # the primitive is the same in both builds
        for ops, inb in _operands(rng, bs, 300):
            out, _ = V.call(getattr(lib, f"t_mul2_{site}"), *ops)
            a, b, c, d = (V.val(x) for x in ops)
            _check(out, (a * b + c * d) * Rinv, bounds[f"{site}_out"], inb)


def test_mulsqr_random_and_extreme(libs, bounds):
    rng = np.random.default_rng(33)
    bs = [bounds["dbl_a"], bounds["dbl_b"], bounds["sqr_c"]]
    for ops, inb in _operands(rng, bs, 300):
        out, _ = V.call(libs[0].t_mulsqr, *ops)
        a, b, c = (V.val(x) for x in ops)
        _check(out, (a * b + c * c) * Rinv, bounds["sqr_out"], inb)


def test_fused_result_fits_the_loop_carried_class(bounds):
    """Y3 must still weaken into FY = F<MASK + 16, (6 << 24) + 16, 96> (the headers assert the same at compile time)"""
    for site in ("dbl", "madd"):
        lb, tb, vb = bounds[f"{site}_out"]
        assert lb == MASK and tb <= (6 << 24) + 16 and vb <= 96


@pytest.mark.parametrize("gen", ["jacobian_dbl_add", "mixed_addition", "jacobian_chain"])
def test_formulas_agree_with_affine_arithmetic_and_with_each_other(libs, gen):
    """whole dbl / add_jac / madd with the switches on and off: every record is checked against affine arithmetic by the vectors
    themselves; the two builds must give the same affine point (canonical X, Y after the Z^-1 normalisation) and the same flag"""
    on, off = (V.drive(dict(V.GENERATORS)[gen](), lib) for lib in libs)
    assert len(on) == len(off) >= 82
    for (ra, oa, fa), (rb, ob, fb) in zip(on, off):
        assert ra.op == rb.op and fa == fb
        assert V.jac_to_aff(oa) == V.jac_to_aff(ob)
        if ra.ins == rb.ins:  # same operands (always, outside the chain): X3 and Z3 do not depend on how Y3 was reduced
            assert oa[0:9] == ob[0:9] and oa[18:27] == ob[18:27]
            assert V.val(oa[9:18]) % p == V.val(ob[9:18]) % p


def test_default_switches():
    """the headers as they stand: dbl's Y3 fused, madd's not (profiles/r24_p256_fused_y3.md)"""
    assert C.CDLL(_build("u29_fused_default.so", [])).t_fused_switches() == 1


def test_stand_alone_program_all_builds():
    """the program that is also built with -fsanitize=address,undefined (by hand, see profiles/r24_p256_fused_y3.md): 64 windows of
    4 dbl + 1 madd from G, the affine end point against Python and the same from every build"""
    k, outs = 1, []
    for w in range(64):
        k = 16 * k + (-1 if w & 1 else 1)
    want = V.aff_mul(k, V.G)
    for name, flags in (("u29_fused_main_on", ON), ("u29_fused_main_off", OFF), ("u29_fused_main_default", [])):
        exe = _build(name, ["-DU29_FUSED_MAIN"] + flags, shared=False)
        text = subprocess.run([exe, "64"], check=True, capture_output=True, text=True).stdout
        lines = text.split("\n")
        assert " failures 0" in lines[0]
        assert (int(lines[1].split()[1], 16), int(lines[2].split()[1], 16)) == want
        outs.append(lines[1:3])
    assert outs[0] == outs[1] == outs[2]
