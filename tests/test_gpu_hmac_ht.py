"""GPU tests of HMAC and deterministic ECDSA over the whole hash table (ec_hmac_slots_batch, ec_rfc6979_nonce_ht_batch,
ec_decdsa_sign_ht_batch and their _dev forms): byte for byte against the recorded answers of the unmodified reference
(tests/golden/hmac_ht.json) and, where hashlib has the hash, against hmac.new (tests/hmac_ht_ref.py)."""
import ctypes as C
import functools

import pytest

import libecc_amd
import oracles as O
import hmac_ht_ref as M
import sigfam_ref as R
from bign_ref import fast_mul

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = libecc_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return M.load_fixture()


# ---- ec_hmac_slots_batch ----
@functools.lru_cache(maxsize=None)
def hmac_case(name):
    """(key slots, key stride, message slots, stride) of the N_GPU items of a hash"""
    pairs = [M.hmac_pair(name, i) for i in range(M.N_GPU)]
    ks, ms = M.stride_for(max(p[0] for p in pairs)), M.stride_for(max(p[1] for p in pairs))
    return (b"".join(M.slot(M.key_bytes(kl), ks) for kl, _ in pairs), ks, b"".join(M.slot(M.msg_bytes(ml), ms) for _, ml in pairs), ms)


_macs = {}


def hmac_want(ctx, fx, name):
    """the N_GPU MACs of one device call, once they are known to be the reference's: every item against the fixture (items with the
    same lengths give the same bytes) and against hmac.new where hashlib has the hash"""
    if name not in _macs:
        keys, ks, msgs, ms = hmac_case(name)
        got, hl = ctx.hmac_slots(M.HASH_IDS[name], keys, ks, msgs, ms), M.HASH_SIZES[name]
        mac_of = {}
        for i in range(M.N_GPU):
            mac, p = got[hl * i:hl * i + hl], M.hmac_pair(name, i)
            assert mac_of.setdefault(p, mac) == mac, (name, i)
            if M.have_hashlib(name):
                assert mac == M.py_hmac(name, M.key_bytes(p[0]), M.msg_bytes(p[1])), (name, i)
        M.assert_macs(fx, name, mac_of)
        _macs[name] = got
    return _macs[name]


@pytest.mark.parametrize("name", M.NAMES)
def test_hmac_slots(ctx, fx, name):
    """130 items (two full waves and two lanes) cycling through the key and message lengths; again in chunks of 64"""
    keys, ks, msgs, ms = hmac_case(name)
    want = hmac_want(ctx, fx, name)
    try:
        ctx.set_max_chunk(64)
        assert ctx.hmac_slots(M.HASH_IDS[name], keys, ks, msgs, ms) == want, name
    finally:
        ctx.set_max_chunk(1 << 20)


@pytest.mark.parametrize("name", M.NAMES)
def test_hmac_unfit_slots_give_zeros_and_leave_the_neighbours(ctx, fx, name):
    keys, ks, msgs, ms = hmac_case(name)
    want, hl = hmac_want(ctx, fx, name), M.HASH_SIZES[name]
    kb, mb = bytearray(keys), bytearray(msgs)
    kb[ks * 3:ks * 3 + 4] = (ks - 3).to_bytes(4, "little")            # item 3: the key does not fit
    mb[ms * 66:ms * 66 + 4] = (0xFFFFFFFF).to_bytes(4, "little")      # item 66: the message does not fit
    mb[ms * 129:ms * 129 + 4] = ms.to_bytes(4, "little")              # the last lane of the tail
    got = ctx.hmac_slots(M.HASH_IDS[name], bytes(kb), ks, bytes(mb), ms)
    for j in range(M.N_GPU):
        assert got[hl * j:hl * j + hl] == (bytes(hl) if j in (3, 66, 129) else want[hl * j:hl * j + hl]), (name, j)


# ---- the _ht nonces and signatures ----
@functools.lru_cache(maxsize=None)
def pub_of(curve, x):
    c = O.CURVES[curve]
    return R.pt_bytes(curve, fast_mul(x, (c["gx"], c["gy"]), c["a"], c["p"]))


def sign_ht(ctx, cv, name, privs, msgs, slots, digests=None):
    ql = cv.qlen
    if slots:
        stride = M.stride_for(max(len(m) for m in msgs))
        inp = b"".join(M.slot(m, stride) for m in msgs)
    else:
        stride, inp = M.HASH_SIZES[name], b"".join(digests)
    sigs, st = cv.decdsa_sign_ht(M.HASH_IDS[name], b"".join(privs), inp, stride, not slots)
    return [(st[j], sigs[2 * ql * j:2 * ql * (j + 1)]) for j in range(len(privs))]


def device_digests(ctx, name, msgs):
    stride = M.stride_for(max(len(m) for m in msgs))
    hl = M.HASH_SIZES[name]
    d = ctx.digest_slots(M.HASH_IDS[name], b"".join(M.slot(m, stride) for m in msgs), stride)
    return [d[hl * j:hl * j + hl] for j in range(len(msgs))]


EDGE_AT = (1, 3, 5)      # where the edge keys sit in a call: each between two good items
_items = {}


def pair_items(ctx, cv, fx, curve, name, with_edges=True):
    """(keys, messages, [(status, signature)], nonces or None per item) of a (curve, hash) pair, the edge keys (x = 0, q - 1, q) between
    good items.  The signatures are those of one ec_decdsa_sign_ht_batch call from message slots, once they are known to be the
    reference's (hmac_ht_ref.assert_sigs); the nonces are solved from them."""
    if (curve, name) not in _items:
        privs, msgs = (list(v) for v in zip(*(M.derive(curve, name, i) for i in range(M.n_items(curve)))))
        for at, priv in zip(EDGE_AT, M.edge_keys(curve)):
            privs.insert(at, priv); msgs.insert(at, M.EDGE_MSG)
        got = sign_ht(ctx, cv, name, privs, msgs, True)
        M.assert_sigs(fx, curve, name, [g for j, g in enumerate(got) if j not in EDGE_AT], [got[j] for j in EDGE_AT])
        dgs = device_digests(ctx, name, msgs)
        ks = [None if j in EDGE_AT else M.k_from_sig(curve, privs[j], dgs[j], got[j][1]).to_bytes(cv.qlen, "big") for j in range(len(got))]
        _items[(curve, name)] = (privs, msgs, got, ks)
    privs, msgs, want, ks = _items[(curve, name)]
    keep = [j for j in range(len(privs)) if with_edges or j not in EDGE_AT]
    return [privs[j] for j in keep], [msgs[j] for j in keep], [want[j] for j in keep], [ks[j] for j in keep]


def assert_all_verify(ctx, cv, curve, name, privs, msgs, got):
    """every status-0 signature is accepted by the composition the header documents: ec_digest_slots_batch_dev into a device buffer,
    then ec_ecdsa_verify_batch_dev on the same stream (x = 0 signs in the reference but has no public key to verify under)"""
    import torch
    dev = torch.device("cuda:0")

    def t(bs):
        return torch.frombuffer(bytearray(bs), dtype=torch.uint8).to(dev)

    sel = [j for j, (st, _) in enumerate(got) if st == 0 and int.from_bytes(privs[j], "big") != 0]
    assert sel
    n, hl = len(sel), M.HASH_SIZES[name]
    stride = M.stride_for(max(len(msgs[j]) for j in sel))
    d_slots = t(b"".join(M.slot(msgs[j], stride) for j in sel))
    d_pub = t(b"".join(pub_of(curve, int.from_bytes(privs[j], "big")) for j in sel))
    d_sig = t(b"".join(got[j][1] for j in sel))
    d_dig = torch.zeros(n * hl, dtype=torch.uint8, device=dev)
    d_res = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    ctx.digest_slots_dev(M.HASH_IDS[name], n, d_slots.data_ptr(), stride, d_dig.data_ptr(), stream)
    cv.ecdsa_verify_dev(n, d_pub.data_ptr(), d_sig.data_ptr(), d_dig.data_ptr(), hl, d_res.data_ptr(), stream)
    torch.cuda.synchronize()
    assert bytes(d_res.cpu().numpy()) == bytes(n), (curve, name)


@pytest.mark.parametrize("curve", M.CURVES)
def test_fixture_signatures_and_nonces(ctx, fx, curve):
    """per (curve, hash) one call each from message slots and from digests: the reference's bytes and status, the edge keys (x = 0 and
    q - 1 sign, x = q is status 1 with zero bytes) between good items; the nonces are the ones the reference signed with"""
    cv = ctx.curve(curve)
    for name in M.NEW_NAMES:
        privs, msgs, want, ks = pair_items(ctx, cv, fx, curve, name)
        dgs = device_digests(ctx, name, msgs)
        assert sign_ht(ctx, cv, name, privs, msgs, False, dgs) == want, (curve, name, "digests")
        assert_all_verify(ctx, cv, curve, name, privs, msgs, want)
        sel = [j for j, k in enumerate(ks) if k is not None]
        nonces, st = cv.rfc6979_nonce_ht(M.HASH_IDS[name], b"".join(privs[j] for j in sel), b"".join(dgs[j] for j in sel))
        assert st == bytes(len(sel)) and nonces == b"".join(ks[j] for j in sel), (curve, name)
    cv.free()


def test_one_item_and_sixty_five(ctx, fx):
    """n = 1, and n = 65 (a full wave and one lane) on one pair, in one chunk and in chunks of 64"""
    curve, name = "BRAINPOOLP256R1", "SHA3_256"
    cv = ctx.curve(curve)
    privs, msgs, want, ks = pair_items(ctx, cv, fx, curve, name, with_edges=False)
    privs, msgs, want = privs + privs[:1], msgs + msgs[:1], want + want[:1]
    assert len(privs) == 65
    try:
        for chunk in (1 << 20, 64):
            ctx.set_max_chunk(chunk)
            assert sign_ht(ctx, cv, name, privs, msgs, True) == want, chunk
    finally:
        ctx.set_max_chunk(1 << 20)
    assert sign_ht(ctx, cv, name, privs[5:6], msgs[5:6], True) == want[5:6]
    dg = device_digests(ctx, name, msgs[5:6])
    assert cv.rfc6979_nonce_ht(M.HASH_IDS[name], privs[5], dg[0]) == (ks[5], b"\0")
    cv.free()


@pytest.mark.parametrize("name", M.OLD_NAMES)
def test_sha2_through_the_ht_names_equals_the_old_names(ctx, name):
    curve = "SECP256R1"
    cv = ctx.curve(curve)
    privs = [M.derive(curve, name, i)[0] for i in range(8)]
    msgs = [M.derive(curve, name, i)[1] for i in range(8)]
    ht, hl = M.HASH_IDS[name], M.HASH_SIZES[name]
    stride = M.stride_for(max(len(m) for m in msgs))
    slots, dgs = b"".join(M.slot(m, stride) for m in msgs), b"".join(M.py_hash(name, m) for m in msgs)
    old = cv.decdsa_sign(ht, b"".join(privs), slots, stride, False)
    assert old[1] == bytes(8)
    assert cv.decdsa_sign_ht(ht, b"".join(privs), slots, stride, False) == old
    assert cv.decdsa_sign_ht(ht, b"".join(privs), dgs, hl, True) == old
    assert cv.rfc6979_nonce_ht(ht, b"".join(privs), dgs) == cv.rfc6979_nonce(ht, b"".join(privs), dgs)
    cv.free()


def test_unfit_message_slot_rejects_its_own_item_only(ctx, fx):
    curve, name = "SECP256R1", "BASH256"
    cv = ctx.curve(curve)
    privs, msgs, want, _ = pair_items(ctx, cv, fx, curve, name, with_edges=False)
    stride = M.stride_for(max(len(m) for m in msgs))
    sl = [M.slot(m, stride) for m in msgs]
    for j, ln in ((0, stride - 3), (3, 0xFFFFFFFF), (len(sl) - 1, stride)):
        sl[j] = M.slot(msgs[j], stride, length=ln)
    sigs, st = cv.decdsa_sign_ht(M.HASH_IDS[name], b"".join(privs), b"".join(sl), stride, False)
    for j in range(len(sl)):
        assert (st[j], sigs[64 * j:64 * j + 64]) == ((1, bytes(64)) if j in (0, 3, len(sl) - 1) else want[j]), j
    cv.free()


def test_dev_forms_on_a_callers_stream(ctx, fx):
    """device pointers on a stream of the caller's: the bytes of the host forms"""
    import torch
    dev = torch.device("cuda:0")

    def t(bs):
        return torch.frombuffer(bytearray(bs), dtype=torch.uint8).to(dev)

    curve = "SECP521R1"
    cv = ctx.curve(curve)
    ql = cv.qlen
    side = torch.cuda.Stream()
    for name in ("RIPEMD160", "STREEBOG512", "SHA3_384", "BASH512", "SHA256"):
        ht, hl = M.HASH_IDS[name], M.HASH_SIZES[name]
        if name in M.NEW_NAMES:
            privs, msgs, want, _ = pair_items(ctx, cv, fx, curve, name)
        else:
            privs, msgs = [M.derive(curve, name, i)[0] for i in range(8)], [M.derive(curve, name, i)[1] for i in range(8)]
            want = sign_ht(ctx, cv, name, privs, msgs, True)
        n = len(privs)
        stride = M.stride_for(max(len(m) for m in msgs))
        dgs = device_digests(ctx, name, msgs)
        d_priv, d_slots, d_dig = t(b"".join(privs)), t(b"".join(M.slot(m, stride) for m in msgs)), t(b"".join(dgs))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for d_in, st_, dig in ((d_slots, stride, False), (d_dig, hl, True)):
                d_sig = torch.full((n * 2 * ql,), 0xEE, dtype=torch.uint8, device=dev)
                d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
                cv.decdsa_sign_ht_dev(ht, n, d_priv.data_ptr(), d_in.data_ptr(), st_, dig, d_sig.data_ptr(), d_st.data_ptr(), side.cuda_stream)
                side.synchronize()
                sig, st = bytes(d_sig.cpu().numpy()), bytes(d_st.cpu().numpy())
                assert [(st[j], sig[2 * ql * j:2 * ql * (j + 1)]) for j in range(n)] == want, (name, dig)
            d_k = torch.full((n * ql,), 0xEE, dtype=torch.uint8, device=dev)
            d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
            cv.rfc6979_nonce_ht_dev(ht, n, d_priv.data_ptr(), d_dig.data_ptr(), d_k.data_ptr(), d_st.data_ptr(), side.cuda_stream)
            side.synchronize()
            assert (bytes(d_k.cpu().numpy()), bytes(d_st.cpu().numpy())) == cv.rfc6979_nonce_ht(ht, b"".join(privs), b"".join(dgs)), name
            keys, ks, mm, ms = hmac_case(name)
            d_keys, d_msgs = t(keys), t(mm)
            d_mac = torch.full((M.N_GPU * hl,), 0xEE, dtype=torch.uint8, device=dev)
            ctx.hmac_slots_dev(ht, M.N_GPU, d_keys.data_ptr(), ks, d_msgs.data_ptr(), ms, d_mac.data_ptr(), side.cuda_stream)
            side.synchronize()
            assert bytes(d_mac.cpu().numpy()) == hmac_want(ctx, fx, name), name
    assert ctx.L.ecamd_ctx_wipe_scratch(ctx.h) == 0
    cv.free()


def test_secret_scalar_mode(ctx, fx):
    """Streebog is refused with a reason by all three calls; another pair gives the bytes of the default mode"""
    curve = "BRAINPOOLP384R1"
    L = ctx.L
    cv = ctx.curve(curve)
    ql = cv.qlen
    ctx.set_secret_scalars(True)
    try:
        priv, st, sig, k = bytes([1] * ql), C.create_string_buffer(b"\x07", 1), C.create_string_buffer(2 * ql), C.create_string_buffer(ql)
        mac = C.create_string_buffer(64)
        for ht, hl in ((13, 32), (14, 64)):
            assert L.ec_hmac_slots_batch(ctx.h, ht, 1, M.slot(b"k", 8), 8, M.slot(b"m", 8), 8, mac) == -1
            assert b"Streebog" in L.ecamd_last_error() and b"secret" in L.ecamd_last_error()
            assert L.ec_rfc6979_nonce_ht_batch(ctx.h, cv.h, ht, 1, priv, bytes(hl), k, st) == -1
            assert b"Streebog" in L.ecamd_last_error()
            assert L.ec_decdsa_sign_ht_batch(ctx.h, cv.h, ht, 1, priv, bytes(hl), hl, 1, sig, st) == -1
            assert b"Streebog" in L.ecamd_last_error()
            assert L.ec_hmac_slots_batch_dev(ctx.h, ht, 0, None, 8, None, 8, None, None) == -1
            assert L.ec_rfc6979_nonce_ht_batch_dev(ctx.h, cv.h, ht, 0, None, None, None, None, None) == -1
            assert L.ec_decdsa_sign_ht_batch_dev(ctx.h, cv.h, ht, 0, None, None, hl, 1, None, None, None) == -1
        assert st.raw == b"\x07" and sig.raw == bytes(2 * ql) and mac.raw == bytes(64)
        for name in ("SHA3_512", "RIPEMD160"):
            privs, msgs, want, _ = pair_items(ctx, cv, fx, curve, name)
            got = sign_ht(ctx, cv, name, privs, msgs, True)
            assert got == want, name
            assert_all_verify(ctx, cv, curve, name, privs, msgs, got)
            keys, ks, mm, ms = hmac_case(name)
            assert ctx.hmac_slots(M.HASH_IDS[name], keys, ks, mm, ms) == hmac_want(ctx, fx, name)
    finally:
        ctx.set_secret_scalars(False)
    # and the default mode serves Streebog again
    privs, msgs, want, _ = pair_items(ctx, cv, fx, curve, "STREEBOG256")
    assert sign_ht(ctx, cv, "STREEBOG256", privs, msgs, True) == want
    cv.free()


def test_call_level_arguments(ctx):
    cv = ctx.curve("SECP256R1")
    L = ctx.L
    priv, dg = bytes([1] * 32), bytes(64)
    k, st, sig, mac = C.create_string_buffer(32), C.create_string_buffer(b"\x07", 1), C.create_string_buffer(64), C.create_string_buffer(64)
    ksl, msl = M.slot(b"key", 8), M.slot(b"msg", 8)
    # n = 0: nothing touched, NULL pointers welcome
    assert L.ec_hmac_slots_batch(ctx.h, 6, 0, None, 8, None, 8, None) == 0
    assert L.ec_hmac_slots_batch_dev(ctx.h, 6, 0, None, 8, None, 8, None, None) == 0
    assert L.ec_rfc6979_nonce_ht_batch(ctx.h, cv.h, 6, 0, None, None, None, None) == 0
    assert L.ec_decdsa_sign_ht_batch(ctx.h, cv.h, 6, 0, None, None, 32, 1, None, None) == 0
    assert L.ec_rfc6979_nonce_ht_batch_dev(ctx.h, cv.h, 6, 0, None, None, None, None, None) == 0
    assert L.ec_decdsa_sign_ht_batch_dev(ctx.h, cv.h, 6, 0, None, None, 8, 0, None, None, None) == 0
    for ht in M.NOT_SERVED:
        assert L.ec_hmac_slots_batch(ctx.h, ht, 1, ksl, 8, msl, 8, mac) == -1
        assert b"hash_type" in L.ecamd_last_error()
        assert L.ec_rfc6979_nonce_ht_batch(ctx.h, cv.h, ht, 1, priv, dg, k, st) == -1
        assert b"hash_type" in L.ecamd_last_error()
        assert L.ec_decdsa_sign_ht_batch(ctx.h, cv.h, ht, 1, priv, dg, 32, 1, sig, st) == -1
        assert L.ec_hmac_slots_batch_dev(ctx.h, ht, 0, None, 8, None, 8, None, None) == -1
        assert L.ec_rfc6979_nonce_ht_batch_dev(ctx.h, cv.h, ht, 0, None, None, None, None, None) == -1
        assert L.ec_decdsa_sign_ht_batch_dev(ctx.h, cv.h, ht, 0, None, None, 32, 1, None, None, None) == -1
    # NULL arguments with n > 0, NULL handles
    assert L.ec_hmac_slots_batch(ctx.h, 6, 1, None, 8, msl, 8, mac) == -1
    assert L.ec_hmac_slots_batch(ctx.h, 6, 1, ksl, 8, msl, 8, None) == -1
    assert L.ec_hmac_slots_batch(None, 6, 1, ksl, 8, msl, 8, mac) == -1
    assert L.ec_rfc6979_nonce_ht_batch(ctx.h, cv.h, 6, 1, None, dg, k, st) == -1
    assert L.ec_decdsa_sign_ht_batch(ctx.h, cv.h, 6, 1, priv, dg, 32, 1, sig, None) == -1
    assert L.ec_decdsa_sign_ht_batch(None, cv.h, 6, 1, priv, dg, 32, 1, sig, st) == -1
    assert L.ec_decdsa_sign_ht_batch(ctx.h, None, 6, 1, priv, dg, 32, 1, sig, st) == -1
    # strides
    for ks, ms in ((0, 8), (6, 8), (4100, 8), (8, 0), (8, 10), (8, 4100)):
        assert L.ec_hmac_slots_batch(ctx.h, 6, 1, ksl, ks, msl, ms, mac) == -1, (ks, ms)
        assert b"stride" in L.ecamd_last_error()
    for stride, dig in ((28, 1), (64, 1), (0, 1), (6, 0), (0, 0), (4100, 0), (32, 2)):
        assert L.ec_decdsa_sign_ht_batch(ctx.h, cv.h, 6, 1, priv, dg, stride, dig, sig, st) == -1, (stride, dig)
    assert L.ec_decdsa_sign_ht_batch(ctx.h, cv.h, 15, 1, priv, dg, 32, 1, sig, st) == -1       # RIPEMD-160's digests are 20 octets
    assert st.raw == b"\x07" and sig.raw == bytes(64) and mac.raw == bytes(64)
    assert L.ec_decdsa_sign_ht_batch(ctx.h, cv.h, 15, 1, priv, dg, 20, 1, sig, st) == 0 and st.raw == b"\x00"
    # the old names still refuse what they refused
    assert L.ec_rfc6979_nonce_batch(ctx.h, cv.h, 5, 1, priv, dg, k, st) == -1
    assert L.ec_decdsa_sign_batch(ctx.h, cv.h, 5, 1, priv, dg, 28, 1, sig, st) == -1
    assert b"hash_type" in L.ecamd_last_error()
    cv.free()
