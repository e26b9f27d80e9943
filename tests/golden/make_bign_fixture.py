#!/usr/bin/env python3
"""Record the UNMODIFIED reference's answers for the crafted BIGN / DBIGN families of tests/bign_ref.py, so that this pin travels
without oracle/_ref:
    python tests/golden/make_bign_fixture.py  ->  tests/golden/bign.json
"belt": the reference's belt_hash of bign_ref.pattern_msg(n) for n = 0 .. 100 and 4092.  Per curve: "verify" items (hash name, OID,
message, public key, signature -> ec_pub_key_import_from_aff_buf + ec_verify's 0 / -1 under BIGN, and under DBIGN, which must agree)
and "sign" items (hash name, OID, message, x, k -> -2 where ec_key_pair_import_from_priv_key_buf fails, else _ec_sign's return value
and signature bytes with the nonce k from the `rand` hook).  The family "dbign" is the reference's own DETERMINISTIC signature
(DBIGN overrides the hook with its generator): its nonce, which stays with the caller of the GPU entry points, is solved from the
signature (k = s1 + hbar + (s0 + 2^(8l)) x) and filed, so that signing with that k must reproduce the reference's bytes.
The answers are whatever the reference says.  A signature is filed as its halves "s0" and "s1"; a message that is
bign_ref.pattern_msg of its length is named by that length ("msgpat")."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracles as O  # noqa: E402
import bign_ref as B  # noqa: E402

OUT = os.path.join(HERE, "bign.json")
SEED = 12018
BELT_LENGTHS = list(range(101)) + [4092]
# families whose items the reference must reject / accept, whatever else is recorded
MIXED = ("s1_range", "oid", "other_key", "s0_byte32")


def build():
    """the fixture as the dict that is written out"""
    rng = np.random.default_rng(SEED)
    out = {"belt": [[n, B.ref_belt_hash(B.pattern_msg(n)).hex()] for n in BELT_LENGTHS]}
    for curve in B.CURVES:
        q, ql, l = O.CURVES[curve]["q"], O.qlen(curve), B.s0_len(curve)
        ver, sgn = [], []
        for family, items in B.verify_families(curve, rng).items():
            rets = []
            for h, oid, msg, pub, sig in items:
                ret = B.ref_verify(curve, h, oid, pub, sig, msg)
                assert ret == B.ref_verify(curve, h, oid, pub, sig, msg, alg=B.DBIGN), (curve, family)
                rets.append(ret)
                ver.append({"family": family, "hash": h, "oid": oid.hex(), "msg": msg.hex(), "pub": pub.hex(), "s0": sig[:l].hex(),
                            "s1": sig[l:].hex(), "ret": ret})
            # a fixture that cannot tell an always-reject implementation from a right one is no fixture
            if family in ("honest", "msg_len"):
                assert rets == [0] * len(rets), (curve, family, rets)
            if family in MIXED:
                assert 0 in rets and -1 in rets, (curve, family, rets)
        assert {i["ret"] for i in ver} == {0, -1}
        for family, items in B.sign_families(curve, rng).items():
            for h, oid, msg, x, k in items:
                ret, sig = B.ref_sign(curve, h, oid, x, k, msg)
                sgn.append({"family": family, "hash": h, "oid": oid.hex(), "msg": msg.hex(), "x": x.to_bytes(ql + 1, "big").hex(),
                            "k": k.to_bytes(ql + 1, "big").hex(), "ret": ret, "out": sig.hex() if sig else None})
        for h in B.hashes_for(curve)[:2]:
            msg, x = B.pattern_msg(int(rng.integers(1, 64))), 1 + B.rand_int(rng, q - 1)
            ret, sig = B.ref_sign(curve, h, B.OID_BELT, x, 0, msg, alg=B.DBIGN)
            assert ret == 0
            k = (int.from_bytes(sig[l:], "little") + int.from_bytes(B.H(h, msg), "little") +
                 (int.from_bytes(sig[:l], "little") + (1 << (8 * l))) * x) % q
            sgn.append({"family": "dbign", "hash": h, "oid": B.OID_BELT.hex(), "msg": msg.hex(), "x": x.to_bytes(ql + 1, "big").hex(),
                        "k": k.to_bytes(ql + 1, "big").hex(), "ret": ret, "out": sig.hex()})
        out[curve] = {"verify": ver, "sign": sgn}
    return out


def dumps(fx):
    """one item per line; a field of DELTA that an item shares with the item before it in its list is left out (the crafted
    families vary one field of a base item), and bign_ref.load_fixture puts it back"""
    out = ["{", '"belt": [']
    out.append(",\n".join(json.dumps(e, separators=(",", ":")) for e in fx["belt"]))
    out.append("],")
    curves = sorted(c for c in fx if c != "belt")
    for ci, curve in enumerate(curves):
        for ki, kind in enumerate(("sign", "verify")):
            items = fx[curve][kind]
            out.append(("%s: {" % json.dumps(curve) if ki == 0 else "") + json.dumps(kind) + ": [")
            for j, i in enumerate(items):
                short = {k: v for k, v in i.items() if not (j and k in B.DELTA and items[j - 1].get(k) == v)}
                if short.get("msg") and short["msg"] == B.pattern_msg(len(short["msg"]) // 2).hex():
                    short["msgpat"] = len(short.pop("msg")) // 2
                out.append(json.dumps(short, sort_keys=True, separators=(",", ":")) + ("," if j + 1 < len(items) else ""))
            out.append("]," if ki == 0 else ("]}," if ci + 1 < len(curves) else "]}"))
    out.append("}")
    return "\n".join(out) + "\n"


def main():
    assert O.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    fx = build()
    with open(OUT, "w") as f:
        f.write(dumps(fx))
    print("wrote", {c: (len(d["verify"]), len(d["sign"])) for c, d in fx.items() if c != "belt"})


if __name__ == "__main__":
    main()
