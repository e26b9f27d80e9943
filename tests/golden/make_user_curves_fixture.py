#!/usr/bin/env python3
"""Find the user-defined curves of tests/user_curves.py and record the UNMODIFIED reference's answers on them:
    python tests/golden/make_user_curves_fixture.py  ->  tests/golden/user_curves.json

The curves are ours.  Two families whose order is known without point counting:
  A   p = 4 q - 1, p and q prime (so p = 3 mod 4):  y^2 = x^3 + a x, supersingular, #E = p + 1 = 4 q, cofactor 4, b = 0 and
      (0, 0) a point of order two;
  B   p = 6 q - 1, p and q prime (so p = 2 mod 3 and p = 1 mod 4):  y^2 = x^3 + b, supersingular, #E = p + 1 = 6 q, cofactor 6.
The generator is [h] (a random point), checked to be of order q.  Everything comes from a seeded generator, so a second run
finds the same curves.

The reference's answers (prj_pt_mul, prj_pt_add, prj_pt_dbl, ECDSA with supplied nonces, ECDSA verification, aff_pt_y_from_x) are
recorded for every curve its default build can hold, bitlen(p) <= 521: the driver hands the parameters to libecc's own
import_params (oracle/ref_driver.c:refdrv_define_curve).  The 544-bit curve is beyond that build: it rests on the Python
integers and the restatement oracle alone ("ref": null).  The inputs are not stored, tests/user_curves.py rebuilds them; the
fixture keeps a SHA-256 of each batch, and of the reference's answers those to the items user_curves.ref_items names (every
verdict of the verification batch; elsewhere an even spread plus the items each batch exists for), packed by user_curves.pack."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import user_curves as U  # noqa: E402

OUT = os.path.join(HERE, "user_curves.json")
SEED = 20261019

# (name, bitlen(p), family, residue of q mod 4 or None, hash of the ECDSA batches, why)
SIZES = [
    ("U160A", 160, "A", None, "SHA256", "smallest accepted p: 6 words, zero top word; digest longer than q, qbits % 8 = 6"),
    ("U161B", 161, "B", None, "SHA256", "one bit into the sixth word"),
    ("U200B", 200, "B", 1, "SHA256", "7 words: odd width, fix64; p = 5 mod 8 for the square root"),
    ("U233A", 233, "A", None, "SHA256", "8 words, no built-in p of this size"),
    ("U257A", 257, "A", None, "SHA256", "10 words with top word 1; clen 33, qlen 32"),
    ("U300B", 300, "B", 3, "SHA256", "10 words; p = 1 mod 8: Tonelli-Shanks with more than one round; digest shorter than q"),
    ("U350A", 350, "A", None, "SHA256", "12 words"),
    ("U400B", 400, "B", None, "SHA512", "14 words"),
    ("U480A", 480, "A", None, "SHA512", "16 words, top word half full"),
    ("U513A", 513, "A", None, "SHA512", "17 words, just past 16; q has 511 bits: digest one bit longer than q"),
    ("U521B", 521, "B", None, "SHA512", "521 bits and no Mersenne prime: the generic radix-2^29 unit of that size, end to end"),
    ("U544A", 544, "A", None, "SHA512", "largest accepted p, above 2^543 + 2^542: fills 17 words; Python and the restatement oracle only"),
    ("X256A", 256, "A", None, "SHA256", "p just above 2^255: the generic radix-2^29 unit on a modulus of zero limbs"),
    ("X512A", 512, "A", None, "SHA512", "p just below 2^512: the generic radix-2^29 unit on a modulus of all-ones limbs"),
]


SMALL = [s for s in range(3, 4000, 2) if all(s % d for d in range(3, int(s ** 0.5) + 1, 2))]


def find_pair(rng, bits, family, qmod4, name):
    """q and p = h q - 1, both prime, bitlen(p) = bits"""
    h = 4 if family == "A" else 6
    if name == "X256A":
        q, step = (1 << 253) + 1, 2                       # p = 2^255 + a little
    elif name == "X512A":
        q, step = (1 << 510) - 1, -2                      # p = 2^512 - a little
    else:
        lo, hi = ((1 << (bits - 1)) + h) // h, ((1 << bits) - 1) // h
        if name == "U544A":
            lo = ((1 << 543) + (1 << 542)) // 4 + 1       # 2 p - 2^544 is large: the Montgomery product overflows its words often
        q, step = rng.randrange(lo, hi) | 1, 2
    while True:
        p = h * q - 1
        if p.bit_length() == bits and (qmod4 is None or q % 4 == qmod4) and all(q % s and p % s for s in SMALL) and \
                U.is_prime(q) and U.is_prime(p):
            return p, q
        q += step


def make_curve(rng, name, bits, family, qmod4, hash_name, why):
    p, q = find_pair(rng, bits, family, qmod4, name)
    h = 4 if family == "A" else 6
    a, b = (rng.randrange(1, p), 0) if family == "A" else (0, rng.randrange(1, p))
    # family A: with -a no square (0, 0) is the only point of order two, the group is cyclic and has points of order 4; U233A
    # takes the other kind, three points of order two
    while family == "A" and (pow(p - a, (p - 1) // 2, p) == 1) != (name == "U233A"):
        a = rng.randrange(1, p)
    cv = {"name": name, "family": family, "h": h, "hash": hash_name, "why": why, "p": p, "a": a, "b": b, "order": h * q, "q": q}
    while True:
        R = U.lift_x(rng.randrange(p), cv)
        G = None if R is None else U.mul(h, R, cv)
        if G is not None:
            break
    assert U.on_curve(G, cv) and U.mul(q, G, cv) is None
    cv["gx"], cv["gy"] = G
    return cv


def record(cv):
    """the reference's answers to the batches of tests/user_curves.py, or None when it cannot hold the curve"""
    import oracles as O
    if U.pbits(cv) > 521:
        # the default build's buffers for keys and signatures are sized for its own largest curve, 521 bits (its integers
        # would hold more): nothing beyond is asked of it
        return None
    assert O.ref_name(cv) is not None
    R = O.RefLib(cv)
    ref = {"smul": {}}
    for label, slen, sc, pts in U.smul_batches(cv):
        out, st = R.scalar_mult(sc, pts, slen=slen)
        ref["smul"][label] = U.pack(U.ref_items(cv, label), st, out)
    A, B, _ = U.add_batch(cv)
    for key, o in (("add", R.pt_add(A, B)), ("dbl", R.pt_add(A))):
        ref[key] = U.pack(U.ref_items(cv, key), o[1], o[0])
    privs, nonces, msgs, ml, _ = U.sign_batch(cv)
    sigs, _, st = R.ecdsa_sign(cv["hash"], privs, nonces, msgs, ml)
    ref["sign"] = U.pack(U.ref_items(cv, "sign"), st, sigs)
    pubs, sg, msgs, ml, _, _ = U.verify_batch(cv)
    ref["verify"] = R.ecdsa_verify(cv["hash"], pubs, sg, msgs, ml).hex()      # the items whose digest is not H(m) do not count
    y1, y2, st = O.ref_y_from_x(cv, U.yfx_batch(cv))
    ref["yfx"] = U.pack(U.ref_items(cv, "yfx"), st, y1, y2)
    return ref


def build():
    rng = random.Random(SEED)
    curves = []
    for row in SIZES:
        cv = make_curve(rng, *row)
        ref = record(cv)
        assert (ref is None) == (U.pbits(cv) > 521), cv["name"]
        c = {k: (format(cv[k], "x") if k in U.PARAM_KEYS else cv[k]) for k in ("name", "family", "h", "hash", "why") + U.PARAM_KEYS}
        c["sha256"] = U.batch_hashes(cv)
        c["ref"] = ref
        curves.append(c)
    return {"note": "User-defined curves (ours, seeded search) and the unmodified reference's recorded answers on them; 'ref' is null "
                    "where the default reference build cannot hold the field (bitlen(p) > 521): that curve rests on Python "
                    "integers and the restatement oracle alone.  Written by make_user_curves_fixture.py.",
            "seed": SEED, "curves": curves}


def dumps(fx):
    return json.dumps(fx, indent=0, sort_keys=True) + "\n"


def main():
    import oracles as O
    assert O.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    fx = build()
    with open(OUT, "w") as f:
        f.write(dumps(fx))
    print("wrote", [(c["name"], "ref" if c["ref"] else "no ref") for c in fx["curves"]], os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
