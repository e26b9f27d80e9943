"""Writes tests/golden/eddsa_sign.json: what the UNMODIFIED reference (oracle/_ref/libecc_ref.so, through tests/eddsa_sign_ref.py)
answers to eddsa_import_key_pair_from_priv_key_buf + eddsa_export_pub_key + _ec_sign with the call's adata and a NULL `rand`, for
EDDSA25519 / CTX / PH and EDDSA448 / PH.  Per variant:
  edge_r / edge_h   |M| chosen so that the hashed length of r = H(dom || prefix || M), |dom| + klen + |M|, resp. of
            H(dom || R || A || M), |dom| + 2 klen + |M|, lands on every padding edge (SHA-512: 111, 112, 127, 128, 129, 239, 240;
            SHAKE256: 135, 136, 137, 271, 272, 273), for |adata| in 0, 1, 3, 255 where the variant takes a context (lengths below 0
            do not exist and are left out); the PH variants: the same edges on |M| itself (edge_m), since PH(M) is what they hash
  ctx       a ten-octet message under every |adata| (a context of 255 octets pushes every edge above out of reach)
  msg_len   |M| = 0, 1 and 1000
  key       all-zero and all-0xFF secret keys
  null_ctx  adata == NULL where the variant takes one: the reference's return value is recorded, whatever it is
Run from the repository root:  python tests/golden/make_eddsa_sign_fixture.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eddsa_sign_ref as E   # noqa: E402

SHA_EDGES = [111, 112, 127, 128, 129, 239, 240]
SHAKE_EDGES = [135, 136, 137, 271, 272, 273]
ADATA_LENS = [0, 1, 3, 255]


def edges(alg):
    return SHAKE_EDGES if E.is448(alg) else SHA_EDGES


def item(alg, family, sk, adata, msg):
    ret, pub, sig = E.ref_sign(alg, sk, adata, msg)
    return {"alg": alg, "family": family, "sk": sk.hex(), "adata": adata.hex() if adata is not None else None, "msg": msg.hex(),
            "pub": pub.hex() if pub else None, "sig": sig.hex() if sig else None, "ret": ret}


def build():
    out = []
    for name, alg in E.ALGS.items():
        rng = np.random.default_rng(8032 + alg)
        kl = E.klen(alg)

        def rnd(n):
            return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()

        adatas = [rnd(n) for n in ADATA_LENS] if E.takes_ctx(alg) else [b""]
        if alg == E.EDDSA25519CTX:
            adatas = adatas[1:]                    # RFC 8032: the context of Ed25519ctx should not be empty; the reference signs
            out.append(item(alg, "empty_ctx", rnd(kl), b"", rnd(5)))   # with an empty one all the same: recorded
        for ad in adatas:
            dl = len(E.dom(alg, ad))
            out.append(item(alg, "ctx", rnd(kl), ad, rnd(10)))
            if E.is_ph(alg):
                for ml in edges(alg):
                    out.append(item(alg, "edge_m", rnd(kl), ad, rnd(ml)))
            lens = sorted({e - dl - kl for e in edges(alg)} | {e - dl - 2 * kl for e in edges(alg)})
            for ml in lens:
                if ml >= 0:
                    fam = "edge_r" if ml + dl + kl in edges(alg) else "edge_h"
                    out.append(item(alg, fam, rnd(kl), ad, rnd(ml)))
        ad = adatas[1] if len(adatas) > 1 else adatas[0]
        for ml in (0, 1, 1000):
            out.append(item(alg, "msg_len", rnd(kl), ad, rnd(ml)))
        for sk in (bytes(kl), b"\xff" * kl):
            out.append(item(alg, "key", sk, ad, rnd(33)))
        if E.takes_ctx(alg):
            out.append(item(alg, "null_ctx", rnd(kl), None, rnd(7)))
    return out


def dumps(fx):
    return "[\n" + ",\n".join(json.dumps(i) for i in fx) + "\n]\n"


if __name__ == "__main__":
    with open(os.path.join(ROOT, "tests", "golden", "eddsa_sign.json"), "w") as f:
        f.write(dumps(build()))
