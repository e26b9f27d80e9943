#!/usr/bin/env python3
"""Record the UNMODIFIED reference's answers for the crafted BIP0340 / ECFSDSA families of tests/schnorr_ref.py, so that this pin
travels without oracle/_ref:
    python tests/golden/make_schnorr_items_fixture.py  ->  tests/golden/schnorr_items.json
Per curve and scheme: "verify" items (hash name, message, key bytes, key format 0 affine / 1 projective, signature ->
ec_pub_key_import_from_aff_buf / ec_pub_key_import_from_buf + ec_verify's 0 / -1) and "sign" items (hash name, message, x and v,
the value the `rand` hook returns -> -2 where ec_key_pair_import_from_priv_key_buf fails, else _ec_sign's return value and
signature bytes).  For ECFSDSA v is the nonce k; for BIP0340 the hook is asked for a value below 2^(8 qlen), v is that AUX value,
and "k" is the nonce schnorr_ref.bip0340_nonce derives from it -- what ec_schnorr_sign_batch takes.  The answers are whatever the
reference says.  A signature is filed as its halves "r" and "s"; a message that is schnorr_ref.pattern_msg of its length is named
by that length ("msgpat")."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracles as O  # noqa: E402
import schnorr_ref as S  # noqa: E402

OUT = os.path.join(HERE, "schnorr_items.json")
SEED = 11340


def build():
    """the fixture as the dict that is written out"""
    rng = np.random.default_rng(SEED)
    out = {}
    for curve in S.CURVES:
        ql, cl = O.qlen(curve), O.clen(curve)
        q = O.CURVES[curve]["q"]
        out[curve] = {}
        for name, alg in S.SCHEMES.items():
            rl = S.r_len(alg, cl)
            ver, sgn = [], []
            for family, items in S.verify_families(curve, alg, rng).items():
                for h, msg, key, fmt, sig in items:
                    ver.append({"family": family, "hash": h, "msg": msg.hex(), "key": key.hex(), "fmt": fmt, "r": sig[:rl].hex(),
                                "s": sig[rl:].hex(), "ret": S.ref_verify(curve, alg, h, key, fmt, sig, msg)})
            for family, items in S.sign_families(curve, alg, rng).items():
                for h, msg, x, v in items:
                    ret, sig = S.ref_sign(curve, alg, h, x, v, msg)
                    it = {"family": family, "hash": h, "msg": msg.hex(), "x": x.to_bytes(ql + 1, "big").hex(),
                          "v": v.to_bytes(ql + 1, "big").hex(), "ret": ret, "out": sig.hex() if sig else None}
                    if alg == S.BIP0340 and 0 < x < q:
                        it["k"] = S.bip0340_nonce(curve, h, x, v, msg).to_bytes(ql, "big").hex()
                    sgn.append(it)
            out[curve][name] = {"verify": ver, "sign": sgn}
    return out


def dumps(fx):
    """one item per line; a field of DELTA that an item shares with the item before it in its list is left out (the crafted
    families vary one field of a base item), and schnorr_ref.load_fixture puts it back"""
    out = ["{"]
    for ci, curve in enumerate(sorted(fx)):
        out.append(json.dumps(curve) + ": {")
        for si, name in enumerate(sorted(fx[curve])):
            for ki, kind in enumerate(("sign", "verify")):
                items = fx[curve][name][kind]
                out.append(("%s: {" % json.dumps(name) if ki == 0 else "") + json.dumps(kind) + ": [")
                for j, i in enumerate(items):
                    short = {k: v for k, v in i.items() if not (j and k in S.DELTA and items[j - 1].get(k) == v)}
                    if short.get("msg") and short["msg"] == S.pattern_msg(len(short["msg"]) // 2).hex():
                        short["msgpat"] = len(short.pop("msg")) // 2
                    out.append(json.dumps(short, sort_keys=True, separators=(",", ":")) + ("," if j + 1 < len(items) else ""))
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
