#!/usr/bin/env python3
"""Derive (and print as C initialisers) the radix-2^29 constants of libecc_amd/csrc/ecamd_u29*.h
from the P-256 domain parameters.  tests/test_u29_host.py re-derives them and compares with what the
header holds, so nothing here needs to be trusted."""
W, NL = 29, 9
MASK = (1 << W) - 1
p = 2**256 - 2**224 + 2**192 + 2**96 - 1
b = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B
R = 1 << (W * NL)


def digits(x, n=NL):
    d = [(x >> (W * i)) & MASK for i in range(n - 1)]
    d.append(x >> (W * (n - 1)))
    return d


def fmt(name, x):
    return f"static constexpr u32 {name}[9] = {{" + ", ".join(f"0x{v:08x}" for v in digits(x)) + "};"


def inv_chain():
    """addition chain for x^(p-2); returns list of ops and checks the exponent"""
    e = {}
    e["x"] = 1
    ops = []

    def sqn(src, n):
        return e[src] << n

    e["e2"] = (e["x"] << 1) + e["x"]
    e["e4"] = (e["e2"] << 2) + e["e2"]
    e["e8"] = (e["e4"] << 4) + e["e4"]
    e["e16"] = (e["e8"] << 8) + e["e8"]
    e["e32"] = (e["e16"] << 16) + e["e16"]
    r = (e["e32"] << 32) + e["x"]
    r = (r << 128) + e["e32"]
    r = (r << 32) + e["e32"]
    r = (r << 16) + e["e16"]
    r = (r << 8) + e["e8"]
    r = (r << 4) + e["e4"]
    r = (r << 2) + e["e2"]
    r = (r << 2) + e["x"]
    assert r == p - 2, hex(r ^ (p - 2))
    return r


# ---- the divstep inversion of ecamd_p256.h (inv_safegcd) ----
SAFEGCD_N = W                 # divsteps per batch: one limb
SAFEGCD_BATCHES = 21
SAFEGCD_BOUND = 590           # divsteps that always suffice for a 256-bit modulus in the variant that starts at delta = 1/2
SAFEGCD_E0 = R * R % p        # e starts here: d ends as +-e0 / (a R) = +-a^-1 R, back in the Montgomery domain


def safegcd_checks():
    """what the divstep inversion takes for granted about p and its constants"""
    assert SAFEGCD_N * SAFEGCD_BATCHES >= SAFEGCD_BOUND and p < 2**256
    # the multiple of p that clears a sum's low limb is the low limb itself: p^-1 = -1 mod 2^29 ...
    assert pow(p, -1, 1 << SAFEGCD_N) == (1 << SAFEGCD_N) - 1
    # ... and m p = m (p + 1) - m, with p + 1 on limbs 3, 6, 7 and 8 only
    assert [i for i, v in enumerate(digits(p + 1)) if v] == [3, 6, 7, 8]
    # the state fits nine signed limbs: |f|, |g| <= p and d, e in (-2p, p), top limb included
    assert 2 * p < 1 << (W * (NL - 1) + 31)
    x = 0x1234567 * R % p
    assert pow(x, -1, p) * SAFEGCD_E0 % p == pow(0x1234567, -1, p) * R % p


if __name__ == "__main__":
    print("p   ", [hex(v) for v in digits(p)])
    print("p+1 ", [hex(v) for v in digits(p + 1)])
    print("2^256 mod p", [hex(v) for v in digits((1 << 256) % p)])
    print(fmt("R2", R * R % p))
    print(fmt("ONE", R % p))
    print(fmt("BM", b * R % p))
    print(fmt("THREE_M", 3 * R % p))
    inv_chain()
    print("inversion chain ok")
    safegcd_checks()
    print(f"divstep inversion: {SAFEGCD_BATCHES} x {SAFEGCD_N} = {SAFEGCD_BATCHES * SAFEGCD_N} divsteps, e0 = R2")
