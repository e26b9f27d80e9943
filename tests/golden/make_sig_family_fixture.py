#!/usr/bin/env python3
"""Record the UNMODIFIED reference's answers for the crafted ECGDSA / ECRDSA / SM2 families of tests/sigfam_ref.py, so that this
pin travels without oracle/_ref:
    python tests/golden/make_sig_family_fixture.py  ->  tests/golden/sig_family.json
Per curve and scheme: "verify" items (hash name, message, public key, signature -> ec_pub_key_import_from_aff_buf + ec_verify's
0 / -1) and "sign" items (hash name, message, x, k -> -2 where ec_key_pair_import_from_priv_key_buf fails, else _ec_sign's
return value and signature bytes).  What the GPU entry points are fed is the digest: hashlib's H(m), or H(Z || m) for SM2 with
the id tests/sigfam_ref.py uses.  An SM2 sign item carries it ("digest", an input: Z needs the public key of x); for the other items
sigfam_ref.load_fixture computes it from the item's hash, message and key.  The answers are whatever the reference says.
SM2's "r + k = q" has no item: no message can be made to hash to the e it needs (and the reference's test for it compares
r + q with q, sig/sm2.c:407-411, so it would sign anyway); tests/test_sig_family_host.py covers it on the restatement."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracles as O  # noqa: E402
import sigfam_ref as S  # noqa: E402

OUT = os.path.join(HERE, "sig_family.json")
SEED = 9001


def build():
    """the fixture as the dict that is written out"""
    rng = np.random.default_rng(SEED)
    out = {}
    for curve in S.CURVES:
        ql = O.qlen(curve)
        out[curve] = {}
        for name, alg in S.SCHEMES.items():
            ver, sgn = [], []
            for family, items in S.verify_families(curve, alg, rng).items():
                for h, msg, pub, sig in items:
                    ver.append({"family": family, "hash": h, "msg": msg.hex(), "pub": pub.hex(), "sig": sig.hex(),
                                "ret": S.ref_verify(curve, alg, h, pub, sig, msg)})
            for family, items in S.sign_families(curve, alg, rng).items():
                for h, msg, x, k in items:
                    ret, sig = S.ref_sign(curve, alg, h, x, k, msg)
                    P = S.pub_point(curve, alg, x) if S.key_ok(alg, O.CURVES[curve]["q"], x) else None
                    pub = S.pt_bytes(curve, P) if P else bytes(2 * O.clen(curve))
                    sgn.append({"family": family, "hash": h, "msg": msg.hex(), "x": x.to_bytes(ql + 1, "big").hex(),
                                "k": k.to_bytes(ql + 1, "big").hex(), "ret": ret, "sig": sig.hex() if sig else None})
                    if alg == S.SM2:
                        sgn[-1]["digest"] = S.digest_for(curve, alg, h, pub, msg).hex()
            out[curve][name] = {"verify": ver, "sign": sgn}
    return out


def dumps(fx):
    """one item per line; a field of DELTA that an item shares with the item before it in its list is left out (the crafted
    families vary one field of a base item), and sigfam_ref.load_fixture puts it back"""
    out = ["{"]
    for ci, curve in enumerate(sorted(fx)):
        out.append(json.dumps(curve) + ": {")
        for si, name in enumerate(sorted(fx[curve])):
            for ki, kind in enumerate(("sign", "verify")):
                items = fx[curve][name][kind]
                out.append(("%s: {" % json.dumps(name) if ki == 0 else "") + json.dumps(kind) + ": [")
                for j, i in enumerate(items):
                    short = {k: v for k, v in i.items() if not (j and k in S.DELTA and items[j - 1].get(k) == v)}
                    out.append(json.dumps(short, sort_keys=True) + ("," if j + 1 < len(items) else ""))
                out.append("]," if ki == 0 else ("]}," if si + 1 < len(fx[curve]) else "]}"))
        out.append("}," if ci + 1 < len(fx) else "}")
    out.append("}")
    return "\n".join(out) + "\n"


def main():
    assert O.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    fx = build()
    with open(OUT, "w") as f:
        f.write(dumps(fx))
    print("wrote", {c: {s: (len(v["verify"]), len(v["sign"])) for s, v in d.items()} for c, d in fx.items()})


if __name__ == "__main__":
    main()
