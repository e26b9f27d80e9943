#!/usr/bin/env python3
"""Record the UNMODIFIED reference's ecdsa_public_key_from_sig answers (return value, the two affine keys or "infinity") for the
crafted families of tests/recover_ref.py, so that this pin travels without oracle/_ref:
    python tests/golden/make_recover_fixture.py  ->  tests/golden/ecdsa_recover.json
The inputs come from a seeded generator; the answers are whatever the reference says, quirks included (an r that is no abscissa
of the curve returns -1: the function's "restart" with r + 2q cannot succeed)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import recover_ref as RR  # noqa: E402

OUT = os.path.join(HERE, "ecdsa_recover.json")
SEED = 8001


def build():
    """the fixture as the dict that is written out"""
    rng = np.random.default_rng(SEED)
    out = {}
    for curve in RR.CURVES:
        items = []
        for family, triples in RR.crafted_families(curve, rng).items():
            for sig, dg, signer in triples:
                p1, p2, s1, s2 = RR.ref_recover(curve, sig, dg, len(dg))
                ret = -1 if s1[0] == RR.ECAMD_ERR else 0
                assert (s1[0] == RR.ECAMD_ERR) == (s2[0] == RR.ECAMD_ERR)
                items.append({"family": family, "sig": sig.hex(), "digest": dg.hex(), "signer": signer.hex() if signer else None,
                              "ret": ret,
                              "key1": None if ret else ("infinity" if s1[0] == RR.ECAMD_INF else p1.hex()),
                              "key2": None if ret else ("infinity" if s2[0] == RR.ECAMD_INF else p2.hex())})
        out[curve] = items
    return out


def dumps(fx):
    return json.dumps(fx, indent=0, sort_keys=True) + "\n"


def main():
    import oracles as O
    assert O.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    fx = build()
    with open(OUT, "w") as f:
        f.write(dumps(fx))
    print("wrote", {c: len(v) for c, v in fx.items()})


if __name__ == "__main__":
    main()
