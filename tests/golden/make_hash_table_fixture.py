#!/usr/bin/env python3
"""Record the UNMODIFIED reference's answers for the ten hashes ec_digest_slots_batch adds to the device, and for a few protocol items
that use them, so that this pin travels without oracle/_ref:
    python tests/golden/make_hash_table_fixture.py  ->  tests/golden/hash_table.json
"kats": per hash, the reference's one-shot (sha3_256, sha512_224, ripemd160, bash384, ...) of hashtable_ref.counting(n) at
hashtable_ref.kat_lengths(hash): [[n, digest hex]].
"items": per "SCHEME/CURVE/HASH" four items {x, pub, msg, k, signed, sig, ret}: `signed` is the reference's signature of msg under the key
x with the nonce k (_ec_sign with the nonce from the `rand` hook; for DBIGN the reference's own deterministic signature, and k is
solved from it: k = s1 + H(m) + (s0 + 2^(8l)) x, as tests/golden/make_bign_fixture.py does); `sig` is what is verified and `ret`
ec_verify's 0 / -1 for (pub, sig, msg).  Items 0 and 1 are honest (sig = signed; one message shorter and one longer than a block),
item 2 carries the signature of another message, item 3 a signature with one bit flipped.  x and k are big-endian, qlen octets."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracles as O  # noqa: E402
import sigfam_ref as S  # noqa: E402
import bign_ref as B  # noqa: E402
import hashtable_ref as T  # noqa: E402

SEED = 19020
MSG_LENS = (5, 150, 33, 97)


def ref_sign(scheme, curve, h, x, k, msg):
    if scheme == "ECDSA":
        return S.ref_sign(curve, T.ECDSA, h, x, k, msg)
    return B.ref_sign(curve, h, T.OID_BASH[h], x, k, msg, alg=T.DBIGN if scheme == "DBIGN" else T.BIGN)


def ref_verify(scheme, curve, h, pub, sig, msg):
    if scheme == "ECDSA":
        return S.ref_verify(curve, T.ECDSA, h, pub, sig, msg)
    return B.ref_verify(curve, h, T.OID_BASH[h], pub, sig, msg, alg=T.DBIGN if scheme == "DBIGN" else T.BIGN)


def dbign_k(curve, h, x, msg, sig):
    q, l = O.CURVES[curve]["q"], B.s0_len(curve)
    return (int.from_bytes(sig[l:], "little") + int.from_bytes(T.ref_hash(h, msg), "little") +
            (int.from_bytes(sig[:l], "little") + (1 << (8 * l))) * x) % q


def build():
    """the fixture as the dict that is written out"""
    # the reference's numbers of the hashes that tests/oracles.py and tests/bign_ref.py do not list
    O.HASH_IDS.update(T.HASH_IDS)
    B.HASH_IDS.update(T.HASH_IDS)
    rng = np.random.default_rng(SEED)
    kats = {name: [[n, T.ref_hash(name, T.counting(n)).hex()] for n in T.kat_lengths(name)] for name in T.TABLE}
    items = {}
    for scheme, curve, h in T.COMBOS:
        q, ql = O.CURVES[curve]["q"], O.qlen(curve)
        x = 1 + S.rand_int(rng, q - 1)
        pub = S.pt_bytes(curve, S.pub_point(curve, T.ECDSA, x))
        rows = []
        for j, n in enumerate(MSG_LENS):
            msg = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
            k = 0 if scheme == "DBIGN" else 1 + S.rand_int(rng, q - 1)
            ret, signed = ref_sign(scheme, curve, h, x, k, msg)
            assert ret == 0, (scheme, curve, h, j)
            if scheme == "DBIGN":
                k = dbign_k(curve, h, x, msg, signed)
            sig = signed
            if j == 2:
                other = bytes([msg[0] ^ 1]) + msg[1:]
                ret2, sig = ref_sign(scheme, curve, h, x, 0 if scheme == "DBIGN" else k, other)
                assert ret2 == 0
            if j == 3:
                sig = signed[:7] + bytes([signed[7] ^ 4]) + signed[8:]
            rows.append({"x": x.to_bytes(ql, "big").hex(), "pub": pub.hex(), "msg": msg.hex(), "k": k.to_bytes(ql, "big").hex(),
                         "signed": signed.hex(), "sig": sig.hex(), "ret": ref_verify(scheme, curve, h, pub, sig, msg)})
        # a fixture that cannot tell an always-accept or an always-reject implementation from a right one is no fixture
        assert [r["ret"] for r in rows] == [0, 0, -1, -1], (scheme, curve, h, [r["ret"] for r in rows])
        items["%s/%s/%s" % (scheme, curve, h)] = rows
    return {"kats": kats, "items": items}


def dumps(fx):
    """one known answer and one item per line"""
    out = ["{", '"kats": {']
    names = list(fx["kats"])
    for i, name in enumerate(names):
        out.append(json.dumps(name) + ": [")
        out.append(",\n".join(json.dumps(e, separators=(",", ":")) for e in fx["kats"][name]))
        out.append("]," if i + 1 < len(names) else "]")
    out.append("},")
    out.append('"items": {')
    keys = list(fx["items"])
    for i, key in enumerate(keys):
        out.append(json.dumps(key) + ": [")
        out.append(",\n".join(json.dumps(e, sort_keys=True, separators=(",", ":")) for e in fx["items"][key]))
        out.append("]," if i + 1 < len(keys) else "]")
    out.append("}")
    out.append("}")
    return "\n".join(out) + "\n"


def main():
    assert O.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    fx = build()
    with open(T.FIXTURE, "w") as f:
        f.write(dumps(fx))
    print("wrote", {k: len(v) for k, v in fx["kats"].items()}, {k: len(v) for k, v in fx["items"].items()})


if __name__ == "__main__":
    main()
