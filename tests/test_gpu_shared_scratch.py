"""GPU tests of ONE context's scratch shared across the signature families: every verification family, public-key recovery and
one-call EdDSA signing interleaved on one context under a small max_chunk, each call's bytes against the same call on a context of
its own and against the recorded reference answers of the family's fixture (tests/golden); the batch-wide arrays of
ec_schnorr_verify_msg_all_batch across host chunks with item-by-item calls around it; and the subgroup check of the key, once per
family, on a cofactor curve.  The inputs are those of the family test files."""
import hashlib
import json
import os

import numpy as np
import pytest

import libecc_amd
import oracles as O
import sigfam_ref as SF
import sighash_ref as SH
import schnorr_ref as SS
import bign_ref as B
import eddsa_sign_ref as E
import test_gpu_sig_family as TF
import test_gpu_sig_hashed as TH
import test_gpu_schnorr_items as TS
import test_gpu_bign as TB
import test_gpu_recover as TR
import test_gpu_eddsa_sign as TE

pytestmark = pytest.mark.gpu
CHUNK = 32           # n = 70: three chunks, the last one short, more than one wave; n = 150: every buffer grows (and is wiped) again


def cycle(items, n):
    assert items
    return [items[i % len(items)] for i in range(n)]


def largest(groups):
    return max(sorted(groups.items()), key=lambda g: len(g[1]))


def verdicts(items):
    return bytes(0 if i["ret"] == 0 else 1 for i in items)


def group_by(items, keys):
    out = {}
    for i in items:
        out.setdefault(tuple(i[k] for k in keys), []).append(i)
    return out


_RECOVER = []


def recover_items(curve):
    if not _RECOVER:
        with open(os.path.join(O.GOLDEN, "ecdsa_recover.json")) as f:
            _RECOVER.append(json.load(f))
    return largest(TR.by_digest_len(_RECOVER[0][curve]))[1]


def ecdsa_pool(curve):
    """(key, signature, digest): both keys the reference recovered from each signature of the recovery fixture (on a cofactor curve some
    lie outside the subgroup of order q: those are rejected)"""
    return [(bytes.fromhex(i[k]), bytes.fromhex(i["sig"]), bytes.fromhex(i["digest"])) for i in recover_items(curve) if i["ret"] == 0
            for k in ("key1", "key2") if i[k] != "infinity"]


def ecdsa_call(curve, n):
    """keys recovered by the reference with their signatures, every third digest damaged; the verdicts are the C restatement's"""
    items = cycle(ecdsa_pool(curve), n)
    pubs = b"".join(i[0] for i in items)
    sigs = b"".join(i[1] for i in items)
    dgs = [bytearray(i[2]) for i in items]
    for k in range(0, n, 3):
        dgs[k][0] ^= 0x80
    dgs = b"".join(bytes(d) for d in dgs)
    hlen = len(dgs) // n
    exp = O.Oracle(curve).ecdsa_verify(pubs, sigs, dgs, hlen)
    assert exp.count(0) >= n // 8 and exp.count(1) >= n // 8
    return "ecdsa", lambda cv, ed: cv.ecdsa_verify(pubs, sigs, dgs, hlen), exp


def sigfam_call(curve, n, name="ECGDSA"):
    hlen, group = largest(TF.by_digest_len(TF.load(curve)[name]["verify"]))
    pubs, sigs, dgs, exp = TF.verify_arrays(cycle(group, n))
    return name, lambda cv, ed: cv.sig_verify(SF.SCHEMES[name], pubs, sigs, dgs, hlen), exp


def hashed_call(curve, n, name="ECSDSA"):
    alg = SH.SCHEMES[name]
    h, group = largest(TH.by_hash(TH.load(curve)[name]["verify"]))
    items = cycle(group, n)
    pubs = [bytes.fromhex(i["pub"]) for i in items]
    inp, stride = TH.inputs_for(curve, alg, h, pubs, [bytes.fromhex(i["msg"]) for i in items])
    sigs = b"".join(bytes.fromhex(i["sig"]) for i in items)
    return name, lambda cv, ed: cv.sig_hashed_verify(alg, TH.HT[h], b"".join(pubs), sigs, inp, stride), verdicts(items)


_BIGN = []


def bign_call(curve, n):
    if not _BIGN:
        _BIGN.append(B.load_fixture(os.path.join(O.GOLDEN, "bign.json")))
    (h, oid), group = largest(group_by(_BIGN[0][curve]["verify"], ("hash", "oid")))
    items = cycle(group, n)
    msgs = [bytes.fromhex(i["msg"]) for i in items]
    stride = B.stride_for(max(len(m) for m in msgs))
    inp = b"".join(B.device_input(h, m, stride) for m in msgs)
    pubs = b"".join(bytes.fromhex(i["pub"]) for i in items)
    sigs = b"".join(bytes.fromhex(i["sig"]) for i in items)
    return "bign", lambda cv, ed: cv.bign_verify(TB.A.SIG_BIGN, TB.HT[h], pubs, sigs, inp, stride, bytes.fromhex(oid)), verdicts(items)


def schnorr_call(curve, n, name="ECFSDSA", fmt=SS.PRJ):
    """ECFSDSA with projective keys: the key import's and the on-curve test's slots are in use as well"""
    alg = SS.SCHEMES[name]
    groups = {k: g for k, g in group_by(TS.load(curve)[name]["verify"], ("hash", "fmt")).items() if k[1] == fmt}
    (h, _), group = largest(groups)
    items = cycle(group, n)
    keys = b"".join(bytes.fromhex(i["key"]) for i in items)
    sigs = [bytes.fromhex(i["r"] + i["s"]) for i in items]
    slots, stride = TS.vslots(curve, alg, h, sigs, [bytes.fromhex(i["msg"]) for i in items], blank_fill=0x5A)
    return name, lambda cv, ed: cv.schnorr_verify(alg, TS.HT[h], keys, fmt, b"".join(sigs), slots, stride), verdicts(items)


def recover_call(curve, n):
    sigs, dgs, hlen, exp = TR.fixture_arrays(curve, cycle(recover_items(curve), n))
    return "recover", lambda cv, ed: cv.ecdsa_recover(sigs, dgs, hlen), exp


_EDDSA = []


def eddsa_sign_call(n):
    if not _EDDSA:
        _EDDSA.append(E.load_fixture(os.path.join(O.GOLDEN, "eddsa_sign.json")))
    alg = E.EDDSA25519
    adata, group = TE.groups([i for i in _EDDSA[0] if i["alg"] == alg and i["ret"] == 0])[0]
    items = cycle(group, n)
    ad = bytes.fromhex(adata) if adata is not None else None
    sks, pubs, msgs = ([bytes.fromhex(i[k]) for i in items] for k in ("sk", "pub", "msg"))
    exp = ([(0, bytes.fromhex(i["sig"])) for i in items], pubs)
    return "eddsa_sign", lambda cv, ed: TE.sign(ed, alg, sks, None, ad, msgs), exp


def sequence(curve, n):
    """the calls of one pass, in the order the scratch is handed from one family to the next"""
    seq = [ecdsa_call(curve, n), sigfam_call(curve, n), hashed_call(curve, n), bign_call(curve, n), schnorr_call(curve, n)]
    if curve == "SECP256R1":
        seq += [recover_call(curve, n), eddsa_sign_call(n)]
    return seq + [ecdsa_call(curve, n)]


def fresh(call, curve):
    """the call on a context of its own that has done nothing else"""
    ctx = libecc_amd.Context(0)
    try:
        ctx.set_max_chunk(CHUNK)
        return call(ctx.curve(curve), ctx.curve("WEI25519"))
    finally:
        ctx.close()


@pytest.mark.parametrize("curve", ["SECP256R1", "WEI25519"])
def test_families_interleaved_on_one_context(curve):
    """SECP256R1: every family; WEI25519 (a cofactor curve: the [q]Y pass runs too): the verification families"""
    shared = libecc_amd.Context(0)
    try:
        shared.set_max_chunk(CHUNK)
        cv, ed = shared.curve(curve), shared.curve("WEI25519")
        for n in (70, 150):
            for name, call, exp in sequence(curve, n):
                got = call(cv, ed)
                assert got == exp, (curve, n, name, "against the recorded reference answers")
                assert got == fresh(call, curve), (curve, n, name, "against a context of its own")
    finally:
        shared.close()


def _slots(parts, stride):
    out = bytearray()
    for m in parts:
        out += len(m).to_bytes(4, "little") + m + bytes(stride - 4 - len(m))
    return bytes(out)


def test_batch_wide_arrays_across_host_chunks():
    """ec_schnorr_verify_msg_all_batch (ECFSDSA on SECP256K1) filed in three uneven host chunks, with an item-by-item call on the same
    context immediately before and after: the verdict is that of a fresh context under the same seed, for an honest batch and for one
    with a damaged item in the last chunk"""
    curve, n, hash_name = "SECP256K1", 333, "SHA256"
    q, cl, ql = O.CURVES[curve]["q"], O.clen(curve), O.qlen(curve)
    rng = np.random.default_rng(777)
    _, item_call, item_exp = schnorr_call(curve, 70, fmt=SS.AFF)
    seed = bytes(range(32))
    old = os.environ.get("ECAMD_HOST_SCHEDULE")
    os.environ["ECAMD_HOST_SCHEDULE"] = "64,100"          # three staging chunks: 64, 100, 169 items
    ctxs = [libecc_amd.Context(0), libecc_amd.Context(0)]
    try:
        cv = ctxs[0].curve(curve)
        rnd = lambda: int.from_bytes(rng.integers(0, 256, size=ql + 8, dtype=np.uint8).tobytes(), "big") % (q - 1) + 1
        x, k = [rnd() for _ in range(n)], [rnd() for _ in range(n)]
        Y, st = cv.scalar_mult(b"".join(v.to_bytes(ql, "big") for v in x))
        W, st2 = cv.scalar_mult(b"".join(v.to_bytes(ql, "big") for v in k))
        assert set(st) == {0} and set(st2) == {0}
        msgs = rng.integers(0, 256, size=23 * n, dtype=np.uint8).tobytes()
        sigs, parts = bytearray(), []
        for i in range(n):
            hin = W[2 * cl * i:2 * cl * (i + 1)] + msgs[23 * i:23 * (i + 1)]
            e = int.from_bytes(hashlib.sha256(hin).digest(), "big") % q
            sigs += W[2 * cl * i:2 * cl * (i + 1)] + ((k[i] + e * x[i]) % q).to_bytes(ql, "big")    # sig/ecfsdsa.c:300-330
            parts.append(hin)
        stride = (4 + 2 * cl + 23 + 3) & ~3
        slots = _slots(parts, stride)
        bad = bytearray(sigs)
        bad[(2 * cl + ql) * (n - 2) + 2 * cl + ql - 1] ^= 1
        for batch, want in ((bytes(sigs), True), (bytes(bad), False)):
            got = []
            for c, around in ((ctxs[0], True), (ctxs[1], False)):
                h = c.curve(curve)
                if around:
                    assert item_call(h, None) == item_exp
                assert c.L.ecamd_ctx_set_msm_seed(c.h, seed) == 0
                got.append(bool(h.schnorr_verify_msg_all(Y, 0, batch, 0, O.HASH_IDS[hash_name], slots, stride, 0xffffffff)))   # no blank for a key in ECFSDSA's hash input
                if around:
                    assert item_call(h, None) == item_exp
            assert got == [want, want], (want, got)
    finally:
        for c in ctxs:
            c.close()
        if old is None:
            del os.environ["ECAMD_HOST_SCHEDULE"]
        else:
            os.environ["ECAMD_HOST_SCHEDULE"] = old


def torsion_key(curve, pub, rng):
    """pub + T for a point T of small order: on the curve, outside the prime-order subgroup (sigfam_ref builds T for its key_torsion items)"""
    cv = O.CURVES[curve]
    cl = O.clen(curve)
    T = SF.small_order_point(curve, rng)
    X, Y = int.from_bytes(pub[:cl], "big"), int.from_bytes(pub[cl:], "big")
    return SF.pt_bytes(curve, O.py_add((X, Y), T, cv["a"], cv["p"]))


def honest(items):
    return next(i for i in items if i["ret"] == 0 and i.get("family") == "honest")


def test_subgroup_check_once_per_family():
    """WEI25519, 70 items under max_chunk 32: the keys of items 0, 33 and 69 are on the curve but outside the subgroup of order q; exactly
    those are rejected, as each family's Python restatement says of the two distinct items"""
    curve, n, where = "WEI25519", 70, (0, 33, 69)
    cl = O.clen(curve)
    rng = np.random.default_rng(4025)
    want = bytes(1 if k in where else 0 for k in range(n))
    ctx = libecc_amd.Context(0)
    try:
        ctx.set_max_chunk(CHUNK)
        cv = ctx.curve(curve)

        def keys_of(pub):
            tk = torsion_key(curve, pub, rng)
            return tk, b"".join(tk if k in where else pub for k in range(n))

        # ECDSA
        pub, sig, dg = next(i for i in ecdsa_pool(curve) if O.Oracle(curve).ecdsa_verify(i[0], i[1], i[2], len(i[2])) == b"\0")
        tk, keys = keys_of(pub)
        assert O.Oracle(curve).ecdsa_verify(pub + tk, sig * 2, dg * 2, len(dg)) == b"\0\1"
        assert cv.ecdsa_verify(keys, sig * n, dg * n, len(dg)) == want, "ecdsa"
        # ECGDSA / ECRDSA / SM2
        for name, alg in sorted(SF.SCHEMES.items()):
            it = honest(TF.load(curve)[name]["verify"])
            pub, sig, dg = (bytes.fromhex(it[k]) for k in ("pub", "sig", "digest"))
            tk, keys = keys_of(pub)
            assert (SF.verify(curve, alg, pub, sig, dg), SF.verify(curve, alg, tk, sig, dg)) == (0, 1), name
            assert cv.sig_verify(alg, keys, sig * n, dg * n, len(dg)) == want, name
        # ECSDSA / ECOSDSA / ECKCDSA
        for name, alg in sorted(SH.SCHEMES.items()):
            it = honest(TH.load(curve)[name]["verify"])
            pub, sig, msg, h = bytes.fromhex(it["pub"]), bytes.fromhex(it["sig"]), bytes.fromhex(it["msg"]), it["hash"]
            tk, keys = keys_of(pub)
            assert (SH.verify(curve, alg, h, pub, sig, msg), SH.verify(curve, alg, h, tk, sig, msg)) == (0, 1), name
            inp, stride = TH.inputs_for(curve, alg, h, [keys[2 * cl * k:2 * cl * (k + 1)] for k in range(n)], [msg] * n)
            assert cv.sig_hashed_verify(alg, TH.HT[h], keys, sig * n, inp, stride) == want, name
        # BIGN
        if not _BIGN:
            _BIGN.append(B.load_fixture(os.path.join(O.GOLDEN, "bign.json")))
        it = honest(_BIGN[0][curve]["verify"])
        pub, sig, msg, h, oid = bytes.fromhex(it["pub"]), bytes.fromhex(it["sig"]), bytes.fromhex(it["msg"]), it["hash"], bytes.fromhex(it["oid"])
        tk, keys = keys_of(pub)
        assert (B.verify(curve, h, oid, pub, sig, msg), B.verify(curve, h, oid, tk, sig, msg)) == (0, 1), "bign"
        stride = B.stride_for(len(msg))
        assert cv.bign_verify(TB.A.SIG_BIGN, TB.HT[h], keys, sig * n, B.device_input(h, msg, stride) * n, stride, oid) == want, "bign"
        # BIP0340 / ECFSDSA, affine keys
        for name, alg in sorted(SS.SCHEMES.items()):
            pool = [i for i in TS.load(curve)[name]["verify"] if i["fmt"] == SS.AFF]
            if not pool:
                continue
            it = honest(pool)
            pub, sig, msg, h = bytes.fromhex(it["key"]), bytes.fromhex(it["r"] + it["s"]), bytes.fromhex(it["msg"]), it["hash"]
            tk, keys = keys_of(pub)
            assert (SS.verify(curve, alg, h, pub, SS.AFF, sig, msg), SS.verify(curve, alg, h, tk, SS.AFF, sig, msg)) == (0, 1), name
            slots, stride = TS.vslots(curve, alg, h, [sig] * n, [msg] * n)
            assert cv.schnorr_verify(alg, TS.HT[h], keys, SS.AFF, sig * n, slots, stride) == want, name
    finally:
        ctx.close()
