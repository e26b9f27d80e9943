"""GPU tests of ECKCDSA, ECSDSA, ECOSDSA, ECFSDSA and BIP0340 over the whole hash table (ec_sig_hashed_*_ht_batch, ec_schnorr_*_ht_batch,
ec_bip0340_*_ht_batch and their _dev forms): byte for byte against the recorded answers of the unmodified reference
(tests/golden/sighash_ht.json; the items are tests/sighash_ht_ref.py's).  Every case has 130 items: two full waves and a tail of two.

Not covered: e = 0 (ECSDSA / ECOSDSA refuse it, ECFSDSA and BIP0340 take it) -- nobody can craft a digest that is 0 mod q under any
of these hashes; the rule is exercised at the level of the shared front ends by tests/test_gpu_sig_hashed.py and
tests/test_gpu_schnorr_items.py, whose code the new names run unchanged.  BIP0340 with a supplied nonce k = 0 or k = q has no reference
call (the reference derives k); the entry point's rule, status 1 with zero bytes, is asserted as such."""
import ctypes as C

import pytest

import libecc_amd
import oracles as O
import sighash_ht_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = libecc_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


def split(buf, size, n):
    return [buf[size * j:size * (j + 1)] for j in range(n)]


def sign_inputs(scheme, curve, name):
    """(privs, v values, messages, inputs, stride) of the N signing items: what the entry points take"""
    alg, ql = R.SCHEMES[scheme], O.qlen(curve)
    items = [R.sign_item(scheme, curve, name, i) for i in range(R.N)]
    top = (1 << (8 * ql)) - 1
    privs = b"".join(min(x, top).to_bytes(ql, "big") for x, _, _ in items)
    vs = b"".join(v.to_bytes(ql, "big") for _, v, _ in items)
    msgs = [m for _, _, m in items]
    if alg == R.ECKCDSA:
        stride = R.HSIZE[name]
        # h = H(z || m) under the key the item signs with: [1/x]G, which an edge key (0, q, q + 1) does not have -- any digest does
        inp = b"".join(R.kcdsa_h(name, R.pub(scheme, curve, i % R.N_KEYS), m) for i, m in enumerate(msgs))
    else:
        stride = R.stride_for(alg, name, curve)
        inp = b"".join(R.slot(alg, name, curve, m, stride) for m in msgs)
    return privs, vs, msgs, inp, stride


def device_sign(cv, scheme, curve, name, ht=True):
    """[(status, signature)] of the N signing items through the scheme's own call (BIP0340: the nonce derived on the device)"""
    alg, hid = R.SCHEMES[scheme], R.HASH_IDS[name]
    privs, vs, msgs, inp, stride = sign_inputs(scheme, curve, name)
    if alg in R.HSIG:
        sigs, st = (cv.sig_hashed_sign_ht if ht else cv.sig_hashed_sign)(alg, hid, privs, vs, inp, stride)
    elif alg == R.ECFSDSA:
        sigs, st = (cv.schnorr_sign_ht if ht else cv.schnorr_sign)(alg, hid, privs, None, vs, inp, stride)
    else:
        sigs, st = (cv.bip0340_sign_ht if ht else cv.bip0340_sign)(hid, privs, None, vs, inp, stride)
    return list(zip(st, split(sigs, R.sig_len(alg, name, curve), R.N)))


_signed = {}


def case_sigs(cv, fx, scheme, curve, name):
    """the device's signatures of a case, once they are known to be the reference's; None where the reference did not sign"""
    key = R.case_key(scheme, curve, name)
    if key not in _signed:
        got = device_sign(cv, scheme, curve, name)
        R.expected_sigs(fx[key], scheme, curve, name, got)
        _signed[key] = (got, R.ref_sigs_or_none(fx[key], scheme, curve, name, got))
    return _signed[key]


def verify_inputs(scheme, curve, name, sigs):
    alg = R.SCHEMES[scheme]
    cl = O.clen(curve)
    fill = next(s for s in sigs if s is not None)
    src = [s if s is not None else fill for s in sigs]
    items = [R.verify_item(scheme, curve, name, i, src) for i in range(R.N)]
    pubs, sg = b"".join(it[0] for it in items), b"".join(it[1] for it in items)
    if alg == R.ECKCDSA:
        stride = R.HSIZE[name]
        inp = b"".join(R.kcdsa_h(name, pk, m) for pk, _, m, _ in items)
    else:
        stride = R.stride_for(alg, name, curve)
        rl = R.r_len(alg, name, curve)
        # ECFSDSA / BIP0340: the slot's commitment field holds other octets than the signature's: the device writes the signature's own
        inp = b"".join(R.slot(alg, name, curve, m, stride, r=bytes([0x5a]) * rl if alg in (R.ECFSDSA, R.BIP0340) else None, fault=f)
                       for _, _, m, f in items)
    return pubs, sg, inp, stride


def device_verify(cv, scheme, curve, name, sigs, ht=True):
    alg, hid = R.SCHEMES[scheme], R.HASH_IDS[name]
    pubs, sg, inp, stride = verify_inputs(scheme, curve, name, sigs)
    if alg in R.HSIG:
        return (cv.sig_hashed_verify_ht if ht else cv.sig_hashed_verify)(alg, hid, pubs, sg, inp, stride)
    return (cv.schnorr_verify_ht if ht else cv.schnorr_verify)(alg, hid, pubs, 0, sg, inp, stride)


@pytest.mark.parametrize("scheme,curve", R.cases())
def test_signatures_and_verdicts_equal_the_reference(ctx, fx, scheme, curve):
    """per hash one signing and one verification call over the 130 items of the case: the reference's signature bytes and status
    (SIGN_EDGES: k = 0, k = q, x = 0, x = q, x = q + 1 under each scheme's own rule) and its verdicts (VERIFY_EDGES: s = 0, q, q - 1, r
    with a bit flipped, a key off the curve, ECFSDSA's W off the curve, altered messages, and the two slot faults)"""
    cv = ctx.curve(curve)
    for name in R.NEW_NAMES:
        got, sigs = case_sigs(cv, fx, scheme, curve, name)
        res = device_verify(cv, scheme, curve, name, sigs)
        want = fx[R.case_key(scheme, curve, name)]["ver"]
        assert "".join(str(b) for b in res) == want, (scheme, curve, name)
        assert want.count("0") >= R.N - len(R.VERIFY_EDGES)
    cv.free()


@pytest.mark.parametrize("scheme,curve", R.cases())
def test_chunks_of_64_give_the_same_bytes(ctx, fx, scheme, curve):
    cv = ctx.curve(curve)
    names = R.NEW_NAMES[R.cases().index((scheme, curve)) % 2::2]      # every hash on half of the cases of a scheme
    want = {name: case_sigs(cv, fx, scheme, curve, name) for name in names}
    try:
        ctx.set_max_chunk(64)
        for name in names:
            assert device_sign(cv, scheme, curve, name) == want[name][0], (scheme, curve, name)
            res = device_verify(cv, scheme, curve, name, want[name][1])
            assert "".join(str(b) for b in res) == fx[R.case_key(scheme, curve, name)]["ver"], (scheme, curve, name)
    finally:
        ctx.set_max_chunk(1 << 20)
    cv.free()


@pytest.mark.parametrize("scheme,curve", R.cases())
def test_sha256_through_the_new_names_equals_the_old_names(ctx, scheme, curve):
    cv = ctx.curve(curve)
    old = device_sign(cv, scheme, curve, R.TWIN, ht=False)
    assert device_sign(cv, scheme, curve, R.TWIN, ht=True) == old
    assert sum(1 for st, _ in old if st == 0) >= R.N - len(R.SIGN_EDGES)
    sigs = [s if st == 0 else None for st, s in old]
    res = device_verify(cv, scheme, curve, R.TWIN, sigs, ht=False)
    assert device_verify(cv, scheme, curve, R.TWIN, sigs, ht=True) == res
    assert res.count(0) >= R.N - len(R.VERIFY_EDGES) and res.count(1) >= 6
    cv.free()


@pytest.mark.parametrize("curve", R.curves_for("BIP0340"))
def test_bip0340_nonces_follow_from_the_recorded_signatures(ctx, fx, curve):
    """ec_bip0340_nonce_ht_batch: k' = s - e d' from the reference's signature is the nonce after the flip by R.y's parity, which the
    fixture records; and ec_schnorr_sign_ht_batch fed with those nonces signs the same bytes (k = 0 and k = q: status 1, zero bytes)"""
    cv = ctx.curve(curve)
    q, ql, cl = O.CURVES[curve]["q"], cv.qlen, cv.clen
    for name in R.NEW_NAMES:
        rec = fx[R.case_key("BIP0340", curve, name)]
        got, sigs = case_sigs(cv, fx, "BIP0340", curve, name)
        privs, aux, msgs, slots, stride = sign_inputs("BIP0340", curve, name)
        nonces, st = cv.bip0340_nonce_ht(R.HASH_IDS[name], privs, None, aux, slots, stride)
        ks = split(nonces, ql, R.N)
        for i in range(R.N):
            if sigs[i] is None:
                assert st[i] == 1 and ks[i] == bytes(ql), (curve, name, i)
                continue
            ke = R.bip_k_even(name, curve, i % R.N_KEYS, sigs[i], msgs[i])
            assert st[i] == 0 and int.from_bytes(ks[i], "big") == (q - ke if rec["rodd"][i] == "1" else ke), (curve, name, i)
        assert {(i % R.N_KEYS < 4, rec["rodd"][i]) for i in range(R.N) if sigs[i] is not None} == \
            {(True, "0"), (True, "1"), (False, "0"), (False, "1")}      # keys and commitments with odd and even y
        kk = list(ks)
        kk[5], kk[129] = bytes(ql), q.to_bytes(ql, "big")
        s2, st2 = cv.schnorr_sign_ht(R.BIP0340, R.HASH_IDS[name], privs, None, b"".join(kk), slots, stride)
        for i, sg in enumerate(split(s2, cl + ql, R.N)):
            assert (st2[i], sg) == ((1, bytes(cl + ql)) if i in (5, 129) else got[i]), (curve, name, i)
    cv.free()


def test_eckcdsa_composition_stays_in_device_memory(ctx, fx):
    """h = H(z || m) by ec_digest_slots_batch_dev over slots the caller lays out, handed to ec_sig_hashed_verify_ht_batch_dev on the
    same stream: the reference's verdicts on whole messages"""
    import torch
    dev = torch.device("cuda:0")

    def t(bs):
        return torch.frombuffer(bytearray(bs), dtype=torch.uint8).to(dev)

    scheme = "ECKCDSA"
    for curve, name in (("SECP192R1", "RIPEMD160"), ("SECP192R1", "SHA3_224"), ("SECP521R1", "BASH512"), ("BRAINPOOLP384R1", "STREEBOG256")):
        cv = ctx.curve(curve)
        hid, hs = R.HASH_IDS[name], R.HSIZE[name]
        got, sigs = case_sigs(cv, fx, scheme, curve, name)
        fill = next(s for s in sigs if s is not None)
        items = [R.verify_item(scheme, curve, name, i, [s if s is not None else fill for s in sigs]) for i in range(R.N)]
        stride = (4 + R.BLOCK[name] + R.max_msg(name) + 3) & ~3
        zslots = b"".join((len(R.kcdsa_z(name, pk) + m)).to_bytes(4, "little") + (R.kcdsa_z(name, pk) + m).ljust(stride - 4, b"\0")
                          for pk, _, m, _ in items)
        d_slots, d_pub, d_sig = t(zslots), t(b"".join(it[0] for it in items)), t(b"".join(it[1] for it in items))
        d_h = torch.zeros(R.N * hs, dtype=torch.uint8, device=dev)
        d_res = torch.full((R.N,), 0xEE, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        ctx.digest_slots_dev(hid, R.N, d_slots.data_ptr(), stride, d_h.data_ptr(), stream)
        cv.sig_hashed_verify_ht_dev(R.ECKCDSA, hid, R.N, d_pub.data_ptr(), d_sig.data_ptr(), d_h.data_ptr(), hs, d_res.data_ptr(), stream)
        torch.cuda.synchronize()
        assert "".join(str(b) for b in bytes(d_res.cpu().numpy())) == fx[R.case_key(scheme, curve, name)]["ver"], (curve, name)
        cv.free()


def test_dev_forms_give_the_same_bytes(ctx, fx):
    """device pointers on a stream of the caller's, every scheme under one hash each on SECP521R1 (BIP0340: both the nonce and the
    signing call)"""
    import torch
    dev = torch.device("cuda:0")

    def t(bs):
        return torch.frombuffer(bytearray(bs), dtype=torch.uint8).to(dev)

    def out(n):
        return torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)

    curve = "SECP521R1"
    cv = ctx.curve(curve)
    ql, cl = cv.qlen, cv.clen
    side = torch.cuda.Stream()
    for scheme, name in (("ECKCDSA", "RIPEMD160"), ("ECSDSA", "SHA3_512"), ("ECOSDSA", "BASH384"), ("ECFSDSA", "SM3"), ("BIP0340", "STREEBOG512"),
                         ("BIP0340", "RIPEMD160")):
        alg, hid = R.SCHEMES[scheme], R.HASH_IDS[name]
        sl = R.sig_len(alg, name, curve)
        got, sigs = case_sigs(cv, fx, scheme, curve, name)
        privs, vs, msgs, inp, stride = sign_inputs(scheme, curve, name)
        pubs, sg, vinp, vstride = verify_inputs(scheme, curve, name, sigs)
        d_priv, d_v, d_in, d_pub, d_sg, d_vin = t(privs), t(vs), t(inp), t(pubs), t(sg), t(vinp)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            d_sig, d_st, d_res, s = out(R.N * sl), out(R.N), out(R.N), side.cuda_stream
            if alg in R.HSIG:
                cv.sig_hashed_sign_ht_dev(alg, hid, R.N, d_priv.data_ptr(), d_v.data_ptr(), d_in.data_ptr(), stride, d_sig.data_ptr(), d_st.data_ptr(), s)
                cv.sig_hashed_verify_ht_dev(alg, hid, R.N, d_pub.data_ptr(), d_sg.data_ptr(), d_vin.data_ptr(), vstride, d_res.data_ptr(), s)
            else:
                if alg == R.ECFSDSA:
                    cv.schnorr_sign_ht_dev(alg, hid, R.N, d_priv.data_ptr(), None, d_v.data_ptr(), d_in.data_ptr(), stride, d_sig.data_ptr(),
                                           d_st.data_ptr(), s)
                else:
                    cv.bip0340_sign_ht_dev(hid, R.N, d_priv.data_ptr(), None, d_v.data_ptr(), d_in.data_ptr(), stride, d_sig.data_ptr(), d_st.data_ptr(), s)
                    d_k, d_kst = out(R.N * ql), out(R.N)
                    cv.bip0340_nonce_ht_dev(hid, R.N, d_priv.data_ptr(), None, d_v.data_ptr(), d_in.data_ptr(), stride, d_k.data_ptr(), d_kst.data_ptr(), s)
                    side.synchronize()
                    assert (bytes(d_k.cpu().numpy()), bytes(d_kst.cpu().numpy())) == cv.bip0340_nonce_ht(hid, privs, None, vs, inp, stride), name
                cv.schnorr_verify_ht_dev(alg, hid, R.N, d_pub.data_ptr(), 0, d_sg.data_ptr(), d_vin.data_ptr(), vstride, d_res.data_ptr(), s)
            side.synchronize()
            assert list(zip(bytes(d_st.cpu().numpy()), split(bytes(d_sig.cpu().numpy()), sl, R.N))) == got, (scheme, name)
            assert "".join(str(b) for b in bytes(d_res.cpu().numpy())) == fx[R.case_key(scheme, curve, name)]["ver"], (scheme, name)
    assert ctx.L.ecamd_ctx_wipe_scratch(ctx.h) == 0
    cv.free()


def test_unusable_slot_is_status_1_with_zero_bytes(ctx, fx):
    """signing: a slot shorter than its fixed fields, and slots that do not fit the stride, reject their own items only"""
    for scheme, curve, name in (("ECSDSA", "SECP256R1", "SHA3_256"), ("ECOSDSA", "SECP192R1", "RIPEMD160"), ("ECFSDSA", "SECP521R1", "BASH256"),
                                ("BIP0340", "SECP256K1", "SHA512_256")):
        cv = ctx.curve(curve)
        alg, hid = R.SCHEMES[scheme], R.HASH_IDS[name]
        sl = R.sig_len(alg, name, curve)
        got, _ = case_sigs(cv, fx, scheme, curve, name)
        privs, vs, msgs, inp, stride = sign_inputs(scheme, curve, name)
        slots = split(inp, stride, R.N)
        bad = {0: "slot_short", 64: "slot_unfit", 129: "slot_unfit"}
        for i, f in bad.items():
            slots[i] = R.slot(alg, name, curve, msgs[i], stride, fault=f)
        slots[3] = (0xFFFFFFFF).to_bytes(4, "little") + slots[3][4:]
        if alg in R.HSIG:
            sigs, st = cv.sig_hashed_sign_ht(alg, hid, privs, vs, b"".join(slots), stride)
        elif alg == R.ECFSDSA:
            sigs, st = cv.schnorr_sign_ht(alg, hid, privs, None, vs, b"".join(slots), stride)
        else:
            sigs, st = cv.bip0340_sign_ht(hid, privs, None, vs, b"".join(slots), stride)
        for i, sg in enumerate(split(sigs, sl, R.N)):
            assert (st[i], sg) == ((1, bytes(sl)) if i in (0, 3, 64, 129) else got[i]), (scheme, i)
        cv.free()


def test_secret_scalar_mode(ctx, fx):
    """the two BIP0340 nonce calls refuse Streebog with a reason; every other new call signs the bytes of the default mode, Streebog
    included"""
    curve = "BRAINPOOLP384R1"
    L = ctx.L
    cv = ctx.curve(curve)
    ql, cl = cv.qlen, cv.clen
    got = {(s, n): case_sigs(cv, fx, s, curve, n) for s, n in (("ECSDSA", "STREEBOG256"), ("ECKCDSA", "STREEBOG512"), ("ECFSDSA", "STREEBOG256"),
                                                              ("BIP0340", "SHA3_384"), ("ECOSDSA", "RIPEMD160"))}
    bip = case_sigs(cv, fx, "BIP0340", curve, "STREEBOG256")
    ctx.set_secret_scalars(True)
    try:
        for (scheme, name), (want, sigs) in got.items():
            assert device_sign(cv, scheme, curve, name) == want, (scheme, name)
            res = device_verify(cv, scheme, curve, name, sigs)
            assert "".join(str(b) for b in res) == fx[R.case_key(scheme, curve, name)]["ver"], (scheme, name)
        # BIP0340 with supplied nonces hashes the challenge only: Streebog is served
        privs, aux, msgs, slots, stride = sign_inputs("BIP0340", curve, "STREEBOG256")
        ctx.set_secret_scalars(False)
        nonces, _ = cv.bip0340_nonce_ht(13, privs, None, aux, slots, stride)
        ctx.set_secret_scalars(True)
        s2, st2 = cv.schnorr_sign_ht(R.BIP0340, 13, privs, None, nonces, slots, stride)
        assert list(zip(st2, split(s2, cl + ql, R.N))) == bip[0]
        st, out = C.create_string_buffer(b"\x07", 1), C.create_string_buffer(cl + ql)
        for ht in (13, 14):
            sl1 = R.slot(R.BIP0340, "STREEBOG256" if ht == 13 else "STREEBOG512", curve, b"m", 512)
            assert L.ec_bip0340_nonce_ht_batch(ctx.h, cv.h, ht, 1, bytes([1] * ql), None, bytes(ql), sl1, 512, out, st) == -1
            assert b"Streebog" in L.ecamd_last_error() and b"secret" in L.ecamd_last_error()
            assert L.ec_bip0340_sign_ht_batch(ctx.h, cv.h, ht, 1, bytes([1] * ql), None, bytes(ql), sl1, 512, out, st) == -1
            assert b"Streebog" in L.ecamd_last_error()
            assert L.ec_bip0340_nonce_ht_batch_dev(ctx.h, cv.h, ht, 0, None, None, None, None, 512, None, None, None) == -1
            assert L.ec_bip0340_sign_ht_batch_dev(ctx.h, cv.h, ht, 0, None, None, None, None, 512, None, None, None) == -1
        assert st.raw == b"\x07" and out.raw == bytes(cl + ql)
    finally:
        ctx.set_secret_scalars(False)
    assert device_sign(cv, "BIP0340", curve, "STREEBOG256") == bip[0]
    cv.free()


def test_call_level_arguments(ctx):
    cv = ctx.curve("SECP256R1")
    other = libecc_amd.Context(0)
    ocv = other.curve("SECP256R1")
    L = ctx.L
    b32, b64, st, res = bytes([1] * 32), bytes(64), C.create_string_buffer(b"\x07", 1), C.create_string_buffer(b"\x07", 1)
    sig = C.create_string_buffer(128)
    slot = (200).to_bytes(4, "little") + bytes(508)

    def calls(ht, n=1, h=None, c=None):
        h, c = h or ctx.h, c or cv.h
        return [L.ec_sig_hashed_verify_ht_batch(h, c, R.ECSDSA, ht, n, b64, sig, slot, 512, res),
                L.ec_sig_hashed_sign_ht_batch(h, c, R.ECOSDSA, ht, n, b32, b32, slot, 512, sig, st),
                L.ec_schnorr_verify_ht_batch(h, c, R.ECFSDSA, ht, n, b64, 0, sig, slot, 512, res),
                L.ec_schnorr_sign_ht_batch(h, c, R.BIP0340, ht, n, b32, None, b32, slot, 512, sig, st),
                L.ec_bip0340_nonce_ht_batch(h, c, ht, n, b32, None, b32, slot, 512, sig, st),
                L.ec_bip0340_sign_ht_batch(h, c, ht, n, b32, None, b32, slot, 512, sig, st)]

    def dev_calls(ht):
        return [L.ec_sig_hashed_verify_ht_batch_dev(ctx.h, cv.h, R.ECSDSA, ht, 0, None, None, None, 512, None, None),
                L.ec_sig_hashed_sign_ht_batch_dev(ctx.h, cv.h, R.ECOSDSA, ht, 0, None, None, None, 512, None, None, None),
                L.ec_schnorr_verify_ht_batch_dev(ctx.h, cv.h, R.ECFSDSA, ht, 0, None, 0, None, None, 512, None, None),
                L.ec_schnorr_sign_ht_batch_dev(ctx.h, cv.h, R.BIP0340, ht, 0, None, None, None, None, 512, None, None, None),
                L.ec_bip0340_nonce_ht_batch_dev(ctx.h, cv.h, ht, 0, None, None, None, None, 512, None, None, None),
                L.ec_bip0340_sign_ht_batch_dev(ctx.h, cv.h, ht, 0, None, None, None, None, 512, None, None, None)]

    for ht in R.NOT_SERVED:
        for r in calls(ht) + dev_calls(ht):
            assert r == -1, ht
            assert b"hash_type" in L.ecamd_last_error()
    assert st.raw == b"\x07" and res.raw == b"\x07" and sig.raw == bytes(128)
    for ht in (6, 15, 20):
        assert dev_calls(ht) == [0] * 6 and calls(ht, n=0) == [0] * 6          # n = 0: nothing touched
        assert calls(ht, h=other.h) == [-1] * 6 and calls(ht, c=ocv.h) == [-1] * 6   # a handle of another context
    assert L.ec_sig_hashed_sign_ht_batch(ctx.h, cv.h, R.ECSDSA, 6, 1, None, b32, slot, 512, sig, st) == -1
    assert L.ec_schnorr_sign_ht_batch(ctx.h, cv.h, R.ECFSDSA, 6, 1, b32, None, b32, slot, 510, sig, st) == -1
    assert b"stride" in L.ecamd_last_error()
    assert L.ec_sig_hashed_verify_ht_batch(ctx.h, cv.h, R.ECKCDSA, 15, 1, b64, sig, b64, 32, res) == -1     # RIPEMD-160's digests are 20 octets
    assert L.ec_sig_hashed_verify_ht_batch(ctx.h, cv.h, R.ECKCDSA, 15, 1, b64, sig, b64, 20, res) == 0 and res.raw == b"\x01"
    # the old names still refuse 5 .. 20
    for ht in list(range(5, 12)) + [13, 14, 15, 17, 18, 19, 20]:
        rs = [L.ec_sig_hashed_verify_batch(ctx.h, cv.h, R.ECSDSA, ht, 1, b64, sig, slot, 512, res),
              L.ec_sig_hashed_sign_batch(ctx.h, cv.h, R.ECOSDSA, ht, 1, b32, b32, slot, 512, sig, st),
              L.ec_schnorr_verify_batch(ctx.h, cv.h, R.ECFSDSA, ht, 1, b64, 0, sig, slot, 512, res),
              L.ec_schnorr_sign_batch(ctx.h, cv.h, R.BIP0340, ht, 1, b32, None, b32, slot, 512, sig, st),
              L.ec_bip0340_nonce_batch(ctx.h, cv.h, ht, 1, b32, None, b32, slot, 512, sig, st),
              L.ec_bip0340_sign_batch(ctx.h, cv.h, ht, 1, b32, None, b32, slot, 512, sig, st)]
        assert rs == [-1] * 6, ht
        assert b"hash_type must be 1 .. 4" in L.ecamd_last_error()
    ocv.free()
    other.close()
    cv.free()
