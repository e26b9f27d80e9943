"""GPU tests of BIP0340 / ECFSDSA item by item (ec_schnorr_verify_batch[_dev], ec_schnorr_sign_batch[_dev]): every recorded item of
tests/golden/schnorr_items.json through the host form and the _dev form on every curve and on ecamd_curve_from_params handles, the
sign -> verify round trip signed on the device, signing with and without the public key, secret-scalar mode, chunking with bad and
exceptional-pair items on the chunk boundaries, small and empty batches, unusable slots, argument errors, and the arrays of
ec_schnorr_verify_msg_all_batch handed to the item call unchanged.

BIP0340 signing with k = 0, q - 1 and q cannot be recorded (the reference derives k from an aux value by a hash): those three
rest on the restatement of tests/schnorr_ref.py."""
import os

import numpy as np
import pytest

import oracles as O
import schnorr_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGS = sorted(S.SCHEMES.items())
HT = S.HASH_TYPE

_FIXTURE = []


def load(curve):
    if not _FIXTURE:
        _FIXTURE.append(S.load_fixture(os.path.join(ROOT, "tests", "golden", "schnorr_items.json")))
    return _FIXTURE[0][curve]


def to_dev(*arrays):
    import torch
    dev = torch.device("cuda:0")
    return [None if b is None else torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8).to(dev) for b in arrays]


def ptr(t):
    return None if t is None else t.data_ptr()


def verify_dev(cv, alg, ht, keys, fmt, sigs, slots, stride):
    import torch
    n = len(sigs) // (cv.schnorr_rlen(alg) + cv.qlen)
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    bufs = to_dev(keys, sigs, slots)
    keep = bufs[2].clone()
    res = torch.full((max(n, 1),), 0xAA, dtype=torch.uint8, device=bufs[0].device)
    torch.cuda.synchronize()
    cv.schnorr_verify_dev(alg, ht, n, ptr(bufs[0]), fmt, ptr(bufs[1]), ptr(bufs[2]), stride, ptr(res), stream.cuda_stream)
    stream.synchronize()   # the _dev form only enqueues
    assert torch.equal(keep, bufs[2]), "the caller's slots were modified"
    return bytes(res.cpu().numpy())[:n]


def sign_dev(cv, alg, ht, xs, pubs, ks, slots, stride):
    import torch
    n = len(xs) // cv.qlen
    sl = cv.schnorr_rlen(alg) + cv.qlen
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    bufs = to_dev(xs, pubs, ks, slots)
    keep = bufs[3].clone()
    sig = torch.full((max(sl * n, 1),), 0xAA, dtype=torch.uint8, device=bufs[0].device)
    st = torch.full((max(n, 1),), 0xAA, dtype=torch.uint8, device=bufs[0].device)
    torch.cuda.synchronize()
    cv.schnorr_sign_dev(alg, ht, n, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), stride, ptr(sig), ptr(st), stream.cuda_stream)
    stream.synchronize()
    assert torch.equal(keep, bufs[3]), "the caller's slots were modified"
    return bytes(sig.cpu().numpy())[:sl * n], bytes(st.cpu().numpy())[:n]


def vslots(curve, alg, h, sigs, msgs, stride=None, blank_fill=0):
    """verification slots in ec_schnorr_verify_msg_all_batch's format: the commitment field holds the signature's r"""
    cl = O.clen(curve)
    rl = S.r_len(alg, cl)
    stride = stride or S.stride_for(alg, h, cl, max([len(m) for m in msgs] + [0]))
    return b"".join(S.slot(alg, h, cl, m, stride, r=s[:rl], blank_fill=blank_fill) for s, m in zip(sigs, msgs)), stride


def sslots(curve, alg, h, msgs, stride=None):
    cl = O.clen(curve)
    stride = stride or S.stride_for(alg, h, cl, max([len(m) for m in msgs] + [0]))
    return b"".join(S.slot(alg, h, cl, m, stride) for m in msgs), stride


def groups(items, keys):
    out = {}
    for i in items:
        out.setdefault(tuple(i[k] for k in keys), []).append(i)
    return sorted(out.items())


def run_fixture(cv, curve, reps=(1,)):
    """every recorded item through the host and the _dev form; reps: the group repeated, so that larger batches take other paths"""
    fx = load(curve)
    q, ql, cl = O.CURVES[curve]["q"], O.qlen(curve), O.clen(curve)
    top = (1 << (8 * ql)) - 1
    for name, alg in ALGS:
        sl = S.r_len(alg, cl) + ql
        seen = 0
        for (h, fmt), group in groups(fx[name]["verify"], ("hash", "fmt")):
            keys = b"".join(bytes.fromhex(i["key"]) for i in group)
            sigs = [bytes.fromhex(i["r"] + i["s"]) for i in group]
            # the commitment field of the slot is overwritten by the device: garbage there must not matter
            slots, stride = vslots(curve, alg, h, sigs, [bytes.fromhex(i["msg"]) for i in group], blank_fill=0x5A)
            exp = bytes(0 if i["ret"] == 0 else 1 for i in group)
            for r in reps:
                got = cv.schnorr_verify(alg, HT[h], keys * r, fmt, b"".join(sigs) * r, slots * r, stride)
                assert got == exp * r, (curve, name, h, fmt, [(i["family"], g) for i, g, e in zip(group * r, got, exp * r) if g != e][:6])
                assert verify_dev(cv, alg, HT[h], keys * r, fmt, b"".join(sigs) * r, slots * r, stride) == exp * r, (curve, name, h, "dev")
            seen += len(group)
        assert seen == len(fx[name]["verify"])
        seen = 0
        for (h,), group in groups(fx[name]["sign"], ("hash",)):
            xi = [int(i["x"], 16) for i in group]
            # BIP0340 items whose key pair does not import have no derived k: any nonce must fail
            ki = [int(i.get("k", i["v"] if alg == S.ECFSDSA else "01"), 16) for i in group]
            assert max(xi + ki) <= top
            xs, ks = b"".join(x.to_bytes(ql, "big") for x in xi), b"".join(k.to_bytes(ql, "big") for k in ki)
            slots, stride = sslots(curve, alg, h, [bytes.fromhex(i["msg"]) for i in group])
            sigs = b"".join(bytes.fromhex(i["out"]) if i["ret"] == 0 else bytes(sl) for i in group)
            st = bytes(0 if i["ret"] == 0 else 1 for i in group)
            for r in reps:
                got = cv.schnorr_sign(alg, HT[h], xs * r, None, ks * r, slots * r, stride)
                assert got[1] == st * r, (curve, name, h, [(i["family"], g) for i, g in zip(group * r, got[1])])
                assert got[0] == sigs * r, (curve, name, h)
                assert sign_dev(cv, alg, HT[h], xs * r, None, ks * r, slots * r, stride) == (sigs * r, st * r), (curve, name, h, "dev")
            seen += len(group)
        assert seen == len(fx[name]["sign"])


@pytest.mark.parametrize("curve", S.CURVES)
def test_fixture_item_for_item(gpu_ctx, curve):
    cv = gpu_ctx.curve(curve)
    try:
        run_fixture(cv, curve)
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256K1", "WEI25519"])
def test_fixture_on_a_handle_from_params(gpu_ctx, curve):
    """a fresh ecamd_curve_from_params handle: first batches too small for a comb table of the generator, then batches that build it"""
    import libecc_amd
    cv = libecc_amd.Curve(gpu_ctx, params=O.CURVES[curve])
    try:
        run_fixture(cv, curve, reps=(1, 8))
    finally:
        cv.free()


def signed_batch(cv, curve, alg, h, n, seed, msg_len=24, with_pub=False):
    """n items signed ON THE DEVICE: (xs, pubs, sigs, msgs)"""
    q, ql, cl = O.CURVES[curve]["q"], O.qlen(curve), O.clen(curve)
    rng = np.random.default_rng(seed)
    xi = [1 + S.rand_int(rng, q - 1) for _ in range(n)]
    xs = b"".join(x.to_bytes(ql, "big") for x in xi)
    ks = b"".join((1 + S.rand_int(rng, q - 1)).to_bytes(ql, "big") for _ in range(n))
    msgs = [rng.integers(0, 256, size=msg_len, dtype=np.uint8).tobytes() for _ in range(n)]
    pubs, pst = cv.scalar_mult(xs)
    assert pst == bytes(n)
    slots, stride = sslots(curve, alg, h, msgs)
    sigs, st = cv.schnorr_sign(alg, HT[h], xs, pubs if with_pub else None, ks, slots, stride)
    assert st == bytes(n)
    return xs, ks, pubs, sigs, msgs


def split(b, w):
    return [b[i:i + w] for i in range(0, len(b), w)]


@pytest.mark.parametrize("curve", ["SECP256K1", "SECP256R1", "SECP521R1", "WEI25519"])
def test_sign_verify_round_trip_and_key_forms(gpu_ctx, curve):
    cv = gpu_ctx.curve(curve)
    try:
        ql, cl = O.qlen(curve), O.clen(curve)
        for name, alg in ALGS:
            for h in S.hashes_for(curve)[:2]:
                sl = S.r_len(alg, cl) + ql
                xs, ks, pubs, sigs, msgs = signed_batch(cv, curve, alg, h, 70, 31)
                slots, stride = vslots(curve, alg, h, split(sigs, sl), msgs)
                assert cv.schnorr_verify(alg, HT[h], pubs, S.AFF, sigs, slots, stride) == bytes(70), (curve, name, h)
                # projective keys X || Y || 1
                prj = b"".join(k + (1).to_bytes(cl, "big") for k in split(pubs, 2 * cl))
                assert cv.schnorr_verify(alg, HT[h], prj, S.PRJ, sigs, slots, stride) == bytes(70)
                # the key supplied gives the bytes the derived key gives; so does the _dev form
                ss, _ = sslots(curve, alg, h, msgs)
                assert cv.schnorr_sign(alg, HT[h], xs, pubs, ks, ss, stride) == (sigs, bytes(70))
                assert sign_dev(cv, alg, HT[h], xs, pubs, ks, ss, stride) == (sigs, bytes(70))
                # a supplied key that is not on the curve: status 1, zero bytes (BIP0340; ECFSDSA ignores the array)
                badp = bytearray(pubs)
                badp[2 * cl * 3 + cl] ^= 1
                badp[2 * cl * 69:2 * cl * 70] = b"\xff" * (2 * cl)
                got = cv.schnorr_sign(alg, HT[h], xs, bytes(badp), ks, ss, stride)
                if alg == S.BIP0340:
                    assert got[1] == bytes(1 if i in (3, 69) else 0 for i in range(70))
                    assert got[0][3 * sl:4 * sl] == bytes(sl) and got[0][:3 * sl] == sigs[:3 * sl]
                else:
                    assert got == (sigs, bytes(70))
                # one damaged signature, one damaged message, one foreign key
                bs = bytearray(sigs)
                bs[5 * sl + sl - 1] ^= 1
                bm = list(msgs)
                bm[9] = bytes([bm[9][0] ^ 1]) + bm[9][1:]
                bk = bytearray(pubs)
                bk[2 * cl * 20:2 * cl * 21] = pubs[2 * cl * 21:2 * cl * 22]
                slots2, _ = vslots(curve, alg, h, split(bytes(bs), sl), bm)
                exp = bytes(1 if i in (5, 9, 20) else 0 for i in range(70))
                assert cv.schnorr_verify(alg, HT[h], bytes(bk), S.AFF, bytes(bs), slots2, stride) == exp
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256K1", "SECP256R1"])
def test_secret_scalar_mode_gives_the_same_bytes(gpu_ctx, curve):
    cv = gpu_ctx.curve(curve)
    try:
        for name, alg in ALGS:
            plain = signed_batch(cv, curve, alg, "SHA256", 66, 41)
            gpu_ctx.set_secret_scalars(True)
            try:
                secret = signed_batch(cv, curve, alg, "SHA256", 66, 41)
                sl = S.r_len(alg, O.clen(curve)) + O.qlen(curve)
                slots, stride = vslots(curve, alg, "SHA256", split(secret[3], sl), secret[4])
                assert cv.schnorr_verify(alg, HT["SHA256"], secret[2], S.AFF, secret[3], slots, stride) == bytes(66)
            finally:
                gpu_ctx.set_secret_scalars(False)
            assert plain[3] == secret[3], (curve, name)
    finally:
        cv.free()


def mixed_batch(cv, curve, alg, n, seed):
    """n verification items on one key format (affine): signed ones, with the fixture's rejected and exceptional-pair items of SHA-256
    planted at `spots`: (keys, sigs, slots, stride, expected)"""
    h = "SHA256"
    ql, cl = O.qlen(curve), O.clen(curve)
    sl = S.r_len(alg, cl) + ql
    name = {v: k for k, v in S.SCHEMES.items()}[alg]
    xs, ks, pubs, sigs, msgs = signed_batch(cv, curve, alg, h, n, seed)
    keys, sg, exp = split(pubs, 2 * cl), split(sigs, sl), [0] * n
    pool = [i for i in load(curve)[name]["verify"] if i["hash"] == h and i["fmt"] == S.AFF and len(i["msg"]) // 2 <= 48]
    rejected = [i for i in pool if i["family"] in ("exceptional_pairs", "s_zero", "s_range", "r_range", "w_bad", "key_not_importable", "tampered")]
    accepted = [i for i in pool if i["family"] == "key_parity"]   # every parity of Y.y and R.y: items that MUST pass on a boundary too
    assert len(accepted) == 4 and all(i["ret"] == 0 for i in accepted)
    special = [v for j in range(len(rejected)) for v in ([rejected[j]] + ([accepted[j // 2]] if j % 2 == 0 and j // 2 < 4 else []))]
    spots = [0, 7, 8, 46, 47, 48, 49, 63, 64, 95, 96, 97, n - 2, n - 1]
    for j, at in enumerate(spots):
        it = special[j % len(special)] if j < len(spots) - 1 else [i for i in special if i["family"] == "exceptional_pairs"][0]
        keys[at], sg[at], msgs[at] = bytes.fromhex(it["key"]), bytes.fromhex(it["r"] + it["s"]), bytes.fromhex(it["msg"])
        exp[at] = 0 if it["ret"] == 0 else 1
    slots, stride = vslots(curve, alg, h, sg, msgs)
    return b"".join(keys), b"".join(sg), slots, stride, bytes(exp)


@pytest.mark.parametrize("curve", ["SECP256K1", "SECP256R1", "WEI25519"])
def test_chunks_with_bad_items_on_the_boundaries(gpu_ctx, curve):
    """max_chunk 48, n = 131: three chunks, the last partial, n a multiple of neither 8 nor 64; bad and exceptional-pair items on both
    sides of each boundary and in the last lane.  Equal to the call at the default chunk, and to what was planted."""
    cv = gpu_ctx.curve(curve)
    try:
        for name, alg in ALGS:
            keys, sigs, slots, stride, exp = mixed_batch(cv, curve, alg, 131, 51)
            whole = cv.schnorr_verify(alg, HT["SHA256"], keys, S.AFF, sigs, slots, stride)
            assert whole == exp, (curve, name, [i for i in range(131) if whole[i] != exp[i]])
            xs, ks, pubs, ssig, msgs = signed_batch(cv, curve, alg, "SHA256", 131, 52)
            gpu_ctx.set_max_chunk(48)
            try:
                assert cv.schnorr_verify(alg, HT["SHA256"], keys, S.AFF, sigs, slots, stride) == whole
                assert verify_dev(cv, alg, HT["SHA256"], keys, S.AFF, sigs, slots, stride) == whole
                assert signed_batch(cv, curve, alg, "SHA256", 131, 52)[3] == ssig
                ss, sst = sslots(curve, alg, "SHA256", msgs)
                assert sign_dev(cv, alg, HT["SHA256"], xs, None, ks, ss, sst) == (ssig, bytes(131))
            finally:
                gpu_ctx.set_max_chunk(1 << 20)
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256K1", "SECP384R1"])
def test_small_and_empty_batches(gpu_ctx, curve):
    cv = gpu_ctx.curve(curve)
    try:
        ql, cl = O.qlen(curve), O.clen(curve)
        for name, alg in ALGS:
            sl = S.r_len(alg, cl) + ql
            xs, ks, pubs, sigs, msgs = signed_batch(cv, curve, alg, "SHA256", 65, 61)
            for n in (1, 63, 65, 0):
                slots, stride = vslots(curve, alg, "SHA256", split(sigs, sl)[:n], msgs[:n], stride=S.stride_for(alg, "SHA256", cl, 24))
                assert cv.schnorr_verify(alg, HT["SHA256"], pubs[:2 * cl * n], S.AFF, sigs[:sl * n], slots, stride) == bytes(n)
                assert verify_dev(cv, alg, HT["SHA256"], pubs[:2 * cl * n], S.AFF, sigs[:sl * n], slots, stride) == bytes(n)
                ss, _ = sslots(curve, alg, "SHA256", msgs[:n], stride=stride)
                assert cv.schnorr_sign(alg, HT["SHA256"], xs[:ql * n], None, ks[:ql * n], ss, stride) == (sigs[:sl * n], bytes(n))
                assert sign_dev(cv, alg, HT["SHA256"], xs[:ql * n], None, ks[:ql * n], ss, stride) == (sigs[:sl * n], bytes(n))
    finally:
        cv.free()


def test_bip0340_nonce_edges_rest_on_the_restatement(gpu_ctx):
    curve, alg, h = "SECP256K1", S.BIP0340, "SHA256"
    q, ql, cl = O.CURVES[curve]["q"], O.qlen(curve), O.clen(curve)
    cv = gpu_ctx.curve(curve)
    try:
        x, msg = 0x1234567, b"nonce edges"
        ks = [0, 1, q - 1, q, (1 << 256) - 1]
        exp = [S.sign(curve, alg, h, x, k, msg) for k in ks]
        slots, stride = sslots(curve, alg, h, [msg] * len(ks))
        got = cv.schnorr_sign(alg, HT[h], x.to_bytes(ql, "big") * len(ks), None, b"".join(k.to_bytes(ql, "big") for k in ks), slots, stride)
        assert got == (b"".join(e[1] for e in exp), bytes(e[0] for e in exp)) and got[1] == bytes([1, 0, 0, 1, 1])
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256K1", "SECP521R1"])
def test_unusable_slots(gpu_ctx, curve):
    """a stride too small for the fixed fields rejects every item; a slot whose length does not hold the fixed fields or does not fit
    the stride rejects its item alone"""
    cv = gpu_ctx.curve(curve)
    try:
        ql, cl = O.qlen(curve), O.clen(curve)
        h = "SHA256"
        for name, alg in ALGS:
            sl = S.r_len(alg, cl) + ql
            n = 12
            xs, ks, pubs, sigs, msgs = signed_batch(cv, curve, alg, h, n, 71)
            slots, stride = vslots(curve, alg, h, split(sigs, sl), msgs)
            fl = S.fixed_len(alg, h, cl)
            small = (fl + 3) & ~3      # < 4 + fixed
            assert small < 4 + fl
            assert cv.schnorr_verify(alg, HT[h], pubs, S.AFF, sigs, bytes(small * n), small) == bytes([1]) * n
            assert cv.schnorr_sign(alg, HT[h], xs, None, ks, bytes(small * n), small) == (bytes(sl * n), bytes([1]) * n)
            assert verify_dev(cv, alg, HT[h], pubs, S.AFF, sigs, bytes(small * n), small) == bytes([1]) * n
            bad = {2: fl - 1, 5: stride - 3, 7: 0xFFFFFFFF, 11: 0}
            bs = bytearray(slots)
            for i, ln in bad.items():
                bs[i * stride:i * stride + 4] = ln.to_bytes(4, "little")
            exp = bytes(1 if i in bad else 0 for i in range(n))
            assert cv.schnorr_verify(alg, HT[h], pubs, S.AFF, sigs, bytes(bs), stride) == exp
            assert verify_dev(cv, alg, HT[h], pubs, S.AFF, sigs, bytes(bs), stride) == exp
            ss, _ = sslots(curve, alg, h, msgs)
            bss = bytearray(ss)
            for i, ln in bad.items():
                bss[i * stride:i * stride + 4] = ln.to_bytes(4, "little")
            gs, gst = cv.schnorr_sign(alg, HT[h], xs, None, ks, bytes(bss), stride)
            assert gst == exp
            for i in range(n):
                assert gs[i * sl:(i + 1) * sl] == (bytes(sl) if i in bad else sigs[i * sl:(i + 1) * sl])
    finally:
        cv.free()


@pytest.mark.parametrize("algo", ["straus", "bucket"])
@pytest.mark.parametrize("curve", ["SECP256K1", "SECP256R1"])
def test_same_arrays_as_the_whole_batch_call(gpu_ctx, curve, algo):
    """arrays that ec_schnorr_verify_msg_all_batch accepts (the multi-scalar evaluation chosen by $ECAMD_SCHNORR_MSM_ALGO at a few
    hundred items, as tests/test_gpu_schnorr_msm.py does) give all-zero results here; with one damaged item exactly that index is 1"""
    cv = gpu_ctx.curve(curve)
    old = os.environ.get("ECAMD_SCHNORR_MSM_ALGO")
    os.environ["ECAMD_SCHNORR_MSM_ALGO"] = algo
    try:
        ql, cl = O.qlen(curve), O.clen(curve)
        h, n = "SHA256", 300
        for name, alg in ALGS:
            r_fmt = 1 if alg == S.BIP0340 else 0
            if not cv.schnorr_msm_available(r_fmt):
                pytest.fail("the whole-batch form is not available on %s" % curve)
            sl = S.r_len(alg, cl) + ql
            xs, ks, pubs, sigs, msgs = signed_batch(cv, curve, alg, h, n, 81)
            slots, stride = vslots(curve, alg, h, split(sigs, sl), msgs)
            xo = 2 * S.HSIZE[h] + cl if alg == S.BIP0340 else 0xffffffff
            assert cv.schnorr_verify_msg_all(pubs, S.AFF, sigs, r_fmt, HT[h], slots, stride, xo)
            assert cv.schnorr_verify(alg, HT[h], pubs, S.AFF, sigs, slots, stride) == bytes(n)
            bs = bytearray(sigs)
            bs[123 * sl + sl - 2] ^= 0x10
            slots2, _ = vslots(curve, alg, h, split(bytes(bs), sl), msgs)
            assert not cv.schnorr_verify_msg_all(pubs, S.AFF, bytes(bs), r_fmt, HT[h], slots2, stride, xo)
            assert cv.schnorr_verify(alg, HT[h], pubs, S.AFF, bytes(bs), slots2, stride) == bytes(1 if i == 123 else 0 for i in range(n))
    finally:
        if old is None:
            os.environ.pop("ECAMD_SCHNORR_MSM_ALGO", None)
        else:
            os.environ["ECAMD_SCHNORR_MSM_ALGO"] = old
        cv.free()


def test_argument_errors(gpu_ctx):
    import libecc_amd
    cv = gpu_ctx.curve("SECP256K1")
    other = libecc_amd.Context(0)
    try:
        ql, cl = 32, 32
        xs, ks, pubs, sigs, msgs = signed_batch(cv, "SECP256K1", S.BIP0340, "SHA256", 2, 91)
        slots, stride = vslots("SECP256K1", S.BIP0340, "SHA256", split(sigs, 64), msgs)
        ok = (S.BIP0340, 2, pubs, S.AFF, sigs, slots, stride)
        assert cv.schnorr_verify(*ok) == bytes(2)

        def fails(*a):
            with pytest.raises(Exception):
                cv.schnorr_verify(*a)

        fails(3, 2, pubs, S.AFF, sigs, slots, stride)            # ECSDSA's number: not this call's
        fails(1, 2, pubs, S.AFF, sigs, slots, stride)
        fails(S.BIP0340, 0, pubs, S.AFF, sigs, slots, stride)    # hash_type
        fails(S.BIP0340, 5, pubs, S.AFF, sigs, slots, stride)
        fails(S.BIP0340, 2, pubs, 2, sigs, slots, stride)        # key_fmt
        fails(S.BIP0340, 2, pubs, S.AFF, sigs, slots, stride + 2)
        fails(S.BIP0340, 2, pubs, S.AFF, sigs, slots, 4100)
        fails(S.BIP0340, 2, None, S.AFF, sigs, slots, stride)    # NULL with n > 0
        ss, sst = sslots("SECP256K1", S.BIP0340, "SHA256", msgs)
        with pytest.raises(Exception):
            cv.schnorr_sign(7, 2, xs, None, ks, ss, sst)
        with pytest.raises(Exception):
            cv.schnorr_sign(S.BIP0340, 9, xs, None, ks, ss, sst)
        with pytest.raises(Exception):
            cv.schnorr_sign(S.BIP0340, 2, xs, None, ks, None, sst)
        # a handle of another context
        with pytest.raises(Exception):
            libecc_amd.api._chk(cv.L, cv.L.ec_schnorr_verify_batch(other.h, cv.h, S.BIP0340, 2, 2, pubs, S.AFF, sigs, slots, stride,
                                                                  bytes(2)), "ec_schnorr_verify_batch")
        assert cv.schnorr_verify(*ok) == bytes(2)
    finally:
        other.close()
        cv.free()
