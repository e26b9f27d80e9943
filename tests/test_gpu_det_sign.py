"""GPU tests of DBIGN and BIP0340 signing with the nonce derived on the device (ec_dbign_nonce_batch, ec_dbign_sign_batch,
ec_bip0340_nonce_batch, ec_bip0340_sign_batch and their _dev forms): the recorded answers of the unmodified reference and its own
vectors (tests/golden/det_sign.json) and the Python restatements (tests/det_sign_ref.py).  Every batch is a few hundred items at most."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import libecc_amd
import oracles as O
import bign_ref as B
import schnorr_ref as S
import sigfam_ref as R
import det_sign_ref as D

pytestmark = pytest.mark.gpu
OID = B.OID_BELT


@pytest.fixture(scope="module")
def ctx():
    c = libecc_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return D.load_fixture(os.path.join(O.GOLDEN, "det_sign.json"))


def split(buf, n):
    w = len(buf) // n if n else 0
    return [buf[w * j:w * (j + 1)] for j in range(n)]


# ---- DBIGN ----
def dbign_inputs(h, msgs, slots):
    if slots:
        stride = B.stride_for(max(len(m) for m in msgs))
        return D.HT[h], b"".join(B.slot(m, stride) for m in msgs), stride
    return 0, b"".join(D.H(h, m) for m in msgs), D.HSIZE[h]


def on_device(call, ins, out_sizes):
    """call(*device pointers of ins and of fresh outputs, stream) on torch tensors; an input None stays None: the outputs' bytes"""
    import torch
    dev = torch.device("cuda:0")
    d_in = [None if b is None else torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in ins]
    d_out = [torch.full((max(1, n),), 0xEE, dtype=torch.uint8, device=dev) for n in out_sizes]
    call(*[None if d is None else d.data_ptr() for d in d_in + d_out], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert all(d is None or bytes(d.cpu().numpy()) == b for d, b in zip(d_in, ins))       # the caller's arrays are not written
    return [bytes(d.cpu().numpy())[:n] for d, n in zip(d_out, out_sizes)]


def dbign_sign(cv, h, privs, msgs, oid, t, slots, dev=False):
    ht, inp, stride = dbign_inputs(h, msgs, slots)
    n = len(privs)
    if dev:
        sigs, st = on_device(lambda p, i, sg, s_, stream: cv.dbign_sign_dev(ht, n, p, i, stride, oid, t, sg, s_, stream),
                             [b"".join(privs), inp], [n * cv.bign_siglen(), n])
    else:
        sigs, st = cv.dbign_sign(ht, b"".join(privs), inp, stride, oid, t)
    return list(zip(st, split(sigs, n)))


def dbign_nonce(cv, h, privs, msgs, oid, t, dev=False):
    n, dgs = len(privs), b"".join(D.H(h, m) for m in msgs)
    if dev:
        return on_device(lambda p, i, k, s_, stream: cv.dbign_nonce_dev(n, p, i, D.HSIZE[h], oid, t, k, s_, stream),
                         [b"".join(privs), dgs], [n * cv.qlen, n])
    return cv.dbign_nonce(b"".join(privs), dgs, D.HSIZE[h], oid, t)


def dbign_expected(curve, i):
    return (0, bytes.fromhex(i["sig"])) if i["ret"] == 0 else (1, bytes(B.sig_len(curve)))


@functools.lru_cache(maxsize=None)
def bign_pub(curve, x):
    p, a, b, q, G = B._curve(curve)
    return B.pt_bytes(curve, B.fast_mul(x, G, a, p))


def dbign_all_verify(cv, curve, h, privs, msgs, oid, got):
    """every status-0 signature is accepted by ec_bign_verify_batch (x = 0 signs in the reference but has no key to verify under)"""
    sel = [j for j, (st, _) in enumerate(got) if st == 0 and int.from_bytes(privs[j], "big") != 0]
    assert sel
    res = cv.bign_verify(B.DBIGN, 0, b"".join(bign_pub(curve, int.from_bytes(privs[j], "big")) for j in sel), b"".join(got[j][1] for j in sel),
                         b"".join(D.H(h, msgs[j]) for j in sel), D.HSIZE[h], oid)
    assert res == bytes(len(sel)), (curve, h)


def by_t(items):
    """the items of one hash grouped by their additional data (one call takes one t)"""
    out = {}
    for i in items:
        out.setdefault(i["t"], []).append(i)
    return out


@pytest.mark.parametrize("dev", [False, True], ids=["host_pointers", "device_pointers"])
@pytest.mark.parametrize("curve", D.DBIGN_CURVES)
def test_dbign_fixture(ctx, fx, curve, dev):
    cv = ctx.curve(curve)
    for h in D.DBIGN_HASHES:
        for th, items in by_t([i for i in fx["dbign"][curve] if i["hash"] == h]).items():
            t = bytes.fromhex(th)
            privs, msgs = [bytes.fromhex(i["x"]) for i in items], [bytes.fromhex(i["msg"]) for i in items]
            for slots in (True, False):
                got = dbign_sign(cv, h, privs, msgs, OID, t, slots, dev)
                assert got == [dbign_expected(curve, i) for i in items], (curve, h, slots)
            dbign_all_verify(cv, curve, h, privs, msgs, OID, got)
            ks, st = dbign_nonce(cv, h, privs, msgs, OID, t, dev)
            assert st == bytes(len(items)) and ks == b"".join(bytes.fromhex(i["k"]) for i in items), (curve, h)
    assert ctx.L.ecamd_ctx_wipe_scratch(ctx.h) == 0
    cv.free()


@pytest.mark.parametrize("slots", [True, False])
def test_dbign_reference_vectors(ctx, fx, slots):
    cv = ctx.curve("BIGN256V1")
    for v in fx["dbign_vectors"]:
        priv, msg, oid, t = (bytes.fromhex(v[f]) for f in ("x", "msg", "oid", "t"))
        got = dbign_sign(cv, v["hash"], [priv], [msg], oid, t, slots)
        assert got == [(0, bytes.fromhex(v["sig"]))], (slots, v["t"])
        dbign_all_verify(cv, "BIGN256V1", v["hash"], [priv], [msg], oid, got)
    cv.free()


@functools.lru_cache(maxsize=None)
def dbign_mixed(curve, h="SHA256", n=128, seed=128):
    """n items with the rejection counts 0, 1, >= 2 in turn, so that every 64-item wave holds an item with none and one with >= 2:
    (privs, msgs, nonces, expected (status, signature))"""
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    rng = np.random.default_rng(seed)
    privs, msgs, ks, rs = [], [], [], []
    while len(privs) < n:
        x, m = 1 + R.rand_int(rng, q - 1), rng.integers(0, 256, size=int(rng.integers(0, 40)), dtype=np.uint8).tobytes()
        st, k, r = D.dbign_nonce(curve, h, x, OID, D.T_SAMPLE, m)
        if st == 0 and min(r, 2) == len(privs) % 3:
            privs.append(x.to_bytes(ql, "big")); msgs.append(m); ks.append(k.to_bytes(ql, "big")); rs.append(r)
    for w in range(0, n, 64):
        assert 0 in rs[w:w + 64] and max(rs[w:w + 64]) >= 2
    want = [B.sign_digest(curve, OID, int.from_bytes(x, "big"), int.from_bytes(k, "big"), D.H(h, m)) for x, k, m in zip(privs, ks, msgs)]
    return privs, msgs, ks, want


@pytest.mark.parametrize("curve", D.RETRY_CURVES)
def test_dbign_retries_mixed_in_every_wave_and_two_calls(ctx, curve):
    h = "SHA256"
    privs, msgs, ks, want = dbign_mixed(curve)
    cv = ctx.curve(curve)
    dgs = b"".join(D.H(h, m) for m in msgs)
    got_k, st = cv.dbign_nonce(b"".join(privs), dgs, D.HSIZE[h], OID, D.T_SAMPLE)
    assert st == bytes(len(privs)) and split(got_k, len(privs)) == ks
    for slots in (True, False):
        got = dbign_sign(cv, h, privs, msgs, OID, D.T_SAMPLE, slots)
        assert got == want, (curve, slots)
        # one call equals two calls
        ht, inp, stride = dbign_inputs(h, msgs, slots)
        sigs, st2 = cv.bign_sign(B.DBIGN, ht, b"".join(privs), got_k, inp, stride, OID)
        assert list(zip(st2, split(sigs, len(privs)))) == got
    dbign_all_verify(cv, curve, h, privs, msgs, OID, got)
    cv.free()


def test_dbign_wave_and_chunk_boundaries(ctx):
    curve, h = "SECP224K1", "SHA256"
    privs, msgs, ks, want = dbign_mixed(curve)
    privs, msgs, want = privs + privs[:2], msgs + msgs[:2], want + want[:2]
    cv = ctx.curve(curve)
    for n in (1, 63, 64, 65):
        assert dbign_sign(cv, h, privs[:n], msgs[:n], OID, D.T_SAMPLE, True) == want[:n], n
    try:
        ctx.set_max_chunk(64)
        for slots in (True, False):
            assert dbign_sign(cv, h, privs, msgs, OID, D.T_SAMPLE, slots) == want and len(want) == 130
        got_k, st = cv.dbign_nonce(b"".join(privs), b"".join(D.H(h, m) for m in msgs), D.HSIZE[h], OID, D.T_SAMPLE)
        assert st == bytes(130) and split(got_k, 130) == ks + ks[:2]
    finally:
        ctx.set_max_chunk(1 << 20)
    cv.free()


def test_dbign_bad_slot_rejects_its_own_item_only(ctx):
    curve, h = "SECP224K1", "SHA256"
    privs, msgs, ks, want = dbign_mixed(curve)
    privs, msgs, want = privs[:70], msgs[:70], list(want[:70])
    stride = B.stride_for(max(len(m) for m in msgs))
    sl = [B.slot(m, stride) for m in msgs]
    for j, ln in ((0, stride - 3), (63, 0xFFFFFFFF), (69, stride)):
        sl[j] = B.slot(msgs[j], stride, length=ln)
        want[j] = (1, bytes(B.sig_len(curve)))
    cv = ctx.curve(curve)
    sigs, st = cv.dbign_sign(D.HT[h], b"".join(privs), b"".join(sl), stride, OID, D.T_SAMPLE)
    assert list(zip(st, split(sigs, 70))) == want
    cv.free()


# ---- BIP0340 ----
def bip_slots(curve, h, msgs, stride=None):
    stride = stride or D.bip_stride(curve, h, max(len(m) for m in msgs))
    return b"".join(D.bip_slot(curve, h, m, stride) for m in msgs), stride


def bip_sign(cv, curve, h, privs, auxs, msgs, pubs=None, dev=False, nonce=False):
    """[(status, signature)] of ec_bip0340_sign_batch, or with nonce=True [(status, nonce)] of ec_bip0340_nonce_batch"""
    sl, stride = bip_slots(curve, h, msgs)
    n, pb = len(privs), None if pubs is None else b"".join(pubs)
    if dev:
        fn = cv.bip0340_nonce_dev if nonce else cv.bip0340_sign_dev
        out, st = on_device(lambda p, y, a, s, o, s_, stream: fn(D.HT[h], n, p, y, a, s, stride, o, s_, stream),
                            [b"".join(privs), pb, b"".join(auxs), sl], [n * (cv.qlen if nonce else cv.clen + cv.qlen), n])
    else:
        out, st = (cv.bip0340_nonce if nonce else cv.bip0340_sign)(D.HT[h], b"".join(privs), pb, b"".join(auxs), sl, stride)
    return list(zip(st, split(out, n)))


def bip_expected(curve, i):
    return (0, bytes.fromhex(i["sig"])) if i["ret"] == 0 else (1, bytes(O.clen(curve) + O.qlen(curve)))


def bip_all_verify(cv, curve, h, pubs, msgs, got):
    sel = [j for j, (st, _) in enumerate(got) if st == 0]
    assert sel
    cl = O.clen(curve)
    stride = D.bip_stride(curve, h, max(len(m) for m in msgs))
    sl = b"".join(S.slot(S.BIP0340, h, cl, msgs[j], stride, r=got[j][1][:cl]) for j in sel)
    res = cv.schnorr_verify(S.BIP0340, D.HT[h], b"".join(pubs[j] for j in sel), S.AFF, b"".join(got[j][1] for j in sel), sl, stride)
    assert res == bytes(len(sel)), (curve, h)


def item_pub(curve, i):
    x = int(i["x"], 16)
    return D.bip_pub(curve, x) if 0 < x < O.CURVES[curve]["q"] else None


@pytest.mark.parametrize("dev", [False, True], ids=["host_pointers", "device_pointers"])
@pytest.mark.parametrize("curve", D.BIP_CURVES)
def test_bip0340_fixture(ctx, fx, curve, dev):
    cv = ctx.curve(curve)
    for h in D.BIP_HASHES:
        items = [i for i in fx["bip0340"][curve] if i["hash"] == h]
        privs, auxs, msgs = ([bytes.fromhex(i[f]) for i in items] for f in ("x", "aux", "msg"))
        got = bip_sign(cv, curve, h, privs, auxs, msgs, dev=dev)
        assert got == [bip_expected(curve, i) for i in items], (curve, h)
        bip_all_verify(cv, curve, h, [item_pub(curve, i) for i in items], msgs, got)
        got = bip_sign(cv, curve, h, privs, auxs, msgs, dev=dev, nonce=True)
        assert got == [(0 if i["ret"] == 0 else 1, bytes.fromhex(i["k"])) for i in items], (curve, h)
    assert ctx.L.ecamd_ctx_wipe_scratch(ctx.h) == 0
    cv.free()


def test_bip0340_reference_vectors(ctx, fx):
    curve = "SECP256K1"
    cv = ctx.curve(curve)
    vs = fx["bip0340_vectors"]
    privs, auxs, msgs = ([bytes.fromhex(v[f]) for v in vs] for f in ("x", "aux", "msg"))
    got = bip_sign(cv, curve, "SHA256", privs, auxs, msgs)
    assert got == [(0, bytes.fromhex(v["sig"])) for v in vs]
    pubs = [D.bip_pub(curve, int(v["x"], 16)) for v in vs]
    assert bip_sign(cv, curve, "SHA256", privs, auxs, msgs, pubs) == got
    bip_all_verify(cv, curve, "SHA256", pubs, msgs, got)
    cv.free()


@functools.lru_cache(maxsize=None)
def bip_batch(curve="SECP256K1", h="SHA256", n=130, seed=340):
    """n items over eight keys (odd and even Y.y among them): (privs, pubs, auxs, msgs, nonces, expected)"""
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    rng = np.random.default_rng(seed)
    keys = []
    while len(keys) < 8 or len({k[1][-1] & 1 for k in keys}) < 2:
        x = 1 + R.rand_int(rng, q - 1)
        keys.append((x, D.bip_pub(curve, x)))
    privs, pubs, auxs, msgs, ks, want = [], [], [], [], [], []
    for j in range(n):
        x, pub = keys[j % len(keys)]
        aux, m = R.rand_int(rng, 1 << (8 * ql)), rng.integers(0, 256, size=int(rng.integers(0, 70)), dtype=np.uint8).tobytes()
        (st, sig), k = D.bip_sign(curve, h, x, aux, m, pub)
        privs.append(x.to_bytes(ql, "big")); pubs.append(pub); auxs.append(aux.to_bytes(ql, "big")); msgs.append(m)
        ks.append(k.to_bytes(ql, "big")); want.append((st, sig))
    return privs, pubs, auxs, msgs, ks, want


def test_bip0340_wave_and_chunk_boundaries_keys_and_two_calls(ctx):
    curve, h = "SECP256K1", "SHA256"
    privs, pubs, auxs, msgs, ks, want = bip_batch()
    assert {p[-1] & 1 for p in pubs} == {0, 1}
    cv = ctx.curve(curve)
    for n in (1, 63, 64, 65):
        assert bip_sign(cv, curve, h, privs[:n], auxs[:n], msgs[:n]) == want[:n], n
    sl, stride = bip_slots(curve, h, msgs)
    try:
        ctx.set_max_chunk(64)
        assert bip_sign(cv, curve, h, privs, auxs, msgs) == want and len(want) == 130
        got = bip_sign(cv, curve, h, privs, auxs, msgs, pubs)            # supplied keys
        assert got == want
        for pb in (None, b"".join(pubs)):
            got_k, st = cv.bip0340_nonce(D.HT[h], b"".join(privs), pb, b"".join(auxs), sl, stride)
            assert st == bytes(130) and split(got_k, 130) == ks
            # one call equals two calls
            sigs, st2 = cv.schnorr_sign(S.BIP0340, D.HT[h], b"".join(privs), pb, got_k, sl, stride)
            assert list(zip(st2, split(sigs, 130))) == want
    finally:
        ctx.set_max_chunk(1 << 20)
    bip_all_verify(cv, curve, h, pubs, msgs, got)
    cv.free()


def test_bip0340_bad_key_and_bad_slots_reject_their_own_item_only(ctx):
    curve, h = "SECP256K1", "SHA256"
    privs, pubs, auxs, msgs, ks, want = bip_batch()
    privs, pubs, auxs, msgs, want = privs[:70], list(pubs[:70]), auxs[:70], msgs[:70], list(want[:70])
    cl, ql = O.clen(curve), O.qlen(curve)
    zero = (1, bytes(cl + ql))
    cv = ctx.curve(curve)
    # a supplied key off the curve
    for j in (0, 64):
        pubs[j] = pubs[j][:-1] + bytes([pubs[j][-1] ^ 1])
    sl, stride = bip_slots(curve, h, msgs)
    sigs, st = cv.bip0340_sign(D.HT[h], b"".join(privs), b"".join(pubs), b"".join(auxs), sl, stride)
    assert list(zip(st, split(sigs, 70))) == [zero if j in (0, 64) else w for j, w in enumerate(want)]
    # slots: a length beyond the stride, one short of the fixed fields
    fixed = 2 * D.HSIZE[h] + 2 * cl
    sls = split(sl, 70)
    for j, ln in ((1, stride - 3), (63, fixed - 1), (69, 0xFFFFFFFF)):
        sls[j] = D.bip_slot(curve, h, msgs[j], stride, length=ln)
    sigs, st = cv.bip0340_sign(D.HT[h], b"".join(privs), None, b"".join(auxs), b"".join(sls), stride)
    assert list(zip(st, split(sigs, 70))) == [zero if j in (1, 63, 69) else w for j, w in enumerate(want)]
    ks2, st = cv.bip0340_nonce(D.HT[h], b"".join(privs), None, b"".join(auxs), b"".join(sls), stride)
    assert st == bytes(1 if j in (1, 63, 69) else 0 for j in range(70)) and split(ks2, 70)[1] == bytes(ql)
    # a stride too small for the fixed fields rejects every item
    small = (4 + fixed - 4) & ~3
    sigs, st = cv.bip0340_sign(D.HT[h], b"".join(privs[:3]), None, b"".join(auxs[:3]), bytes(3 * small), small)
    assert st == b"\x01\x01\x01" and sigs == bytes(3 * (cl + ql))
    cv.free()


def test_secret_scalar_mode_gives_the_same_bytes(ctx, fx):
    ctx.set_secret_scalars(True)
    try:
        for curve in D.RETRY_CURVES:
            privs, msgs, ks, want = dbign_mixed(curve)
            cv = ctx.curve(curve)
            assert dbign_sign(cv, "SHA256", privs, msgs, OID, D.T_SAMPLE, True) == want, curve
            got_k, st = cv.dbign_nonce(b"".join(privs), b"".join(D.H("SHA256", m) for m in msgs), 32, OID, D.T_SAMPLE)
            assert split(got_k, len(privs)) == ks
            cv.free()
        for curve in D.DBIGN_CURVES:
            cv = ctx.curve(curve)
            for h in D.DBIGN_HASHES:
                items = [i for i in fx["dbign"][curve] if i["hash"] == h and i["t"] == ""]
                privs, msgs = [bytes.fromhex(i["x"]) for i in items], [bytes.fromhex(i["msg"]) for i in items]
                assert dbign_sign(cv, h, privs, msgs, OID, b"", False) == [dbign_expected(curve, i) for i in items], (curve, h)
            cv.free()
        for curve in D.BIP_CURVES:
            cv = ctx.curve(curve)
            for h in D.BIP_HASHES:
                items = [i for i in fx["bip0340"][curve] if i["hash"] == h]
                privs, auxs, msgs = ([bytes.fromhex(i[f]) for i in items] for f in ("x", "aux", "msg"))
                assert bip_sign(cv, curve, h, privs, auxs, msgs) == [bip_expected(curve, i) for i in items], (curve, h)
            cv.free()
        privs, pubs, auxs, msgs, ks, want = bip_batch()
        cv = ctx.curve("SECP256K1")
        assert bip_sign(cv, "SECP256K1", "SHA256", privs, auxs, msgs) == want
        cv.free()
    finally:
        ctx.set_secret_scalars(False)


def test_call_level_arguments(ctx):
    cv = ctx.curve("SECP256K1")
    other = libecc_amd.Context(0)
    cv2 = other.curve("SECP256K1")
    L, N = ctx.L, None
    priv, dg, aux = bytes([1] * 32), bytes(64), bytes(32)
    k, st = C.create_string_buffer(32), C.create_string_buffer(b"\x07", 1)
    sig, bsig = C.create_string_buffer(48), C.create_string_buffer(64)
    slot = D.bip_slot("SECP256K1", "SHA256", b"m", 136)
    o = (OID, len(OID))

    def dsign(c=ctx.h, v=cv.h, ht=0, n=1, p=priv, i=dg, stride=32, t=N, tl=0, out=sig, s=st):
        return L.ec_dbign_sign_batch(c, v, ht, n, p, i, stride, *o, t, tl, out, s)

    def dnonce(c=ctx.h, v=cv.h, n=1, p=priv, i=dg, dl=32, oid=o, t=N, tl=0, out=k, s=st):
        return L.ec_dbign_nonce_batch(c, v, n, p, i, dl, *oid, t, tl, out, s)

    def bsign(c=ctx.h, v=cv.h, ht=2, n=1, p=priv, a=aux, sl=slot, stride=136, out=bsig, s=st, f=L.ec_bip0340_sign_batch):
        return f(c, v, ht, n, p, N, a, sl, stride, out, s)

    def bnonce(**kw):
        return bsign(out=k, f=L.ec_bip0340_nonce_batch, **kw)
    try:
        # n = 0: nothing touched, NULL pointers welcome
        assert dnonce(n=0, p=N, i=N, out=N, s=N) == 0 and dsign(n=0, p=N, i=N, out=N, s=N) == 0
        assert bsign(n=0, p=N, a=N, sl=N, out=N, s=N) == 0 and bnonce(n=0, p=N, a=N, sl=N, s=N) == 0
        assert L.ec_dbign_nonce_batch_dev(ctx.h, cv.h, 0, N, N, 32, *o, N, 0, N, N, N) == 0
        assert L.ec_dbign_sign_batch_dev(ctx.h, cv.h, 2, 0, N, N, 8, *o, N, 0, N, N, N) == 0
        assert L.ec_bip0340_nonce_batch_dev(ctx.h, cv.h, 2, 0, N, N, N, N, 136, N, N, N) == 0
        assert L.ec_bip0340_sign_batch_dev(ctx.h, cv.h, 2, 0, N, N, N, N, 136, N, N, N) == 0
        # unknown hash_type
        for ht in (5, 17, -1):
            assert dsign(ht=ht) == -1 and b"hash_type" in L.ecamd_last_error()
        for ht in (0, 5, 16, -1):
            assert bsign(ht=ht) == -1 and b"hash_type" in L.ecamd_last_error() and bnonce(ht=ht) == -1
        # t: 65 octets, NULL with a length; an OID that is NULL with a length
        assert dsign(t=bytes(65), tl=65) == -1 and b"t_len" in L.ecamd_last_error()
        assert dsign(tl=1) == -1 and dnonce(tl=1) == -1 and dnonce(t=bytes(65), tl=65) == -1 and dnonce(oid=(N, 3)) == -1
        # NULL aux and the other NULL arguments
        assert bsign(a=N) == -1 and bnonce(a=N) == -1 and bsign(p=N) == -1 and bsign(s=N) == -1
        assert dsign(i=N) == -1 and dnonce(out=N) == -1
        assert L.ec_bip0340_sign_batch_dev(ctx.h, cv.h, 2, 1, N, N, N, N, 136, N, N, N) == -1
        # strides and digest lengths
        for stride in (0, 6, 4100):
            assert bsign(stride=stride) == -1 and dsign(ht=2, stride=stride) == -1, stride
        for dl in (0, 129):
            assert dsign(stride=dl) == -1 and dnonce(dl=dl) == -1
        # a handle of another context, NULL handles
        assert dsign(v=cv2.h) == -1 and bsign(v=cv2.h) == -1 and bnonce(c=N) == -1 and dnonce(v=N) == -1
        assert st.raw == b"\x07" and sig.raw == bytes(48) and bsig.raw == bytes(64) and k.raw == bytes(32)
        assert bsign() == 0 and st.raw == b"\x00"
        assert dsign() == 0 and st.raw == b"\x00"
    finally:
        cv2.free()
        other.close()
        cv.free()
