"""GPU tests of batched ECSDSA / ECOSDSA / ECKCDSA (ec_sig_hashed_verify_batch / ec_sig_hashed_sign_batch and their _dev forms):
the recorded reference answers of tests/golden/sig_hashed.json item for item through both forms on every curve and scheme, the
same on an ecamd_curve_from_params handle, random batches against the reference at run time, the sign -> verify round trip
with every padding-boundary message length signed on the device, a chunked 2^20-item batch with edge items on the chunk
boundaries and mixed message lengths, redo items among ordinary ones (an ACCEPTED ECKCDSA item with e = 0 among them),
secret-scalar mode, signatures of ECDSA and ECGDSA offered under the three schemes, unusable slots, argument errors."""
import os

import numpy as np
import pytest

import oracles as O
import sigfam_ref as SF
import sighash_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGS = sorted(S.SCHEMES.items())
HT = O.HASH_IDS

_FIXTURE = []


def load(curve):
    if not _FIXTURE:
        _FIXTURE.append(S.load_fixture(os.path.join(ROOT, "tests", "golden", "sig_hashed.json")))
    return _FIXTURE[0][curve]


def inputs_for(curve, alg, h, pubs, msgs, stride=None):
    """(inputs, stride): the slots of the messages (one stride for the group), or ECKCDSA's digests"""
    if alg == S.ECKCDSA:
        return b"".join(S.kcdsa_h(curve, h, p, m) for p, m in zip(pubs, msgs)), S.HSIZE[h]
    stride = stride or S.stride_for(alg, O.clen(curve), max([len(m) for m in msgs] + [0]))
    return b"".join(S.slot(alg, O.clen(curve), m, stride) for m in msgs), stride


def key_of(curve, alg, x):
    """the public key the signer's h is made with (ECKCDSA): zeros where x has none"""
    q = O.CURVES[curve]["q"]
    return S.pt_bytes(curve, S.pub_point(curve, alg, x)) if 0 < x < q else bytes(2 * O.clen(curve))


def to_dev(*arrays):
    import torch
    dev = torch.device("cuda:0")
    return [torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8).to(dev) for b in arrays]


def verify_dev(cv, alg, ht, pubs, sigs, inp, stride):
    import torch
    n = len(pubs) // (2 * cv.clen)
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    bufs = to_dev(pubs, sigs, inp)
    keep = bufs[2].clone()
    res = torch.full((n,), 0xAA, dtype=torch.uint8, device=bufs[0].device)
    torch.cuda.synchronize()
    cv.sig_hashed_verify_dev(alg, ht, n, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), stride, res.data_ptr(), stream.cuda_stream)
    stream.synchronize()   # the _dev form only enqueues
    assert torch.equal(keep, bufs[2]), "the caller's slots were modified"
    return bytes(res.cpu().numpy())


def sign_dev(cv, alg, ht, xs, ks, inp, stride):
    import torch
    n = len(xs) // cv.qlen
    sl = cv.sig_hashed_rlen(alg, ht) + cv.qlen
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    bufs = to_dev(xs, ks, inp)
    keep = bufs[2].clone()
    sig = torch.full((sl * n,), 0xAA, dtype=torch.uint8, device=bufs[0].device)
    st = torch.full((n,), 0xAA, dtype=torch.uint8, device=bufs[0].device)
    torch.cuda.synchronize()
    cv.sig_hashed_sign_dev(alg, ht, n, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), stride, sig.data_ptr(), st.data_ptr(),
                           stream.cuda_stream)
    stream.synchronize()
    assert torch.equal(keep, bufs[2]), "the caller's slots were modified"
    return bytes(sig.cpu().numpy()), bytes(st.cpu().numpy())


def by_hash(items):
    groups = {}
    for i in items:
        groups.setdefault(i["hash"], []).append(i)
    return groups


def run_fixture(cv, curve, reps=(1,)):
    """every recorded item through the host and the _dev form; reps: the group repeated, so that larger batches take other paths"""
    fx = load(curve)
    ql = O.qlen(curve)
    top = (1 << (8 * ql)) - 1
    for name, alg in ALGS:
        seen = 0
        for h, group in sorted(by_hash(fx[name]["verify"]).items()):
            pubs = [bytes.fromhex(i["pub"]) for i in group]
            msgs = [bytes.fromhex(i["msg"]) for i in group]
            inp, stride = inputs_for(curve, alg, h, pubs, msgs)
            sigs = b"".join(bytes.fromhex(i["sig"]) for i in group)
            exp = bytes(0 if i["ret"] == 0 else 1 for i in group)
            for r in reps:
                got = cv.sig_hashed_verify(alg, HT[h], b"".join(pubs) * r, sigs * r, inp * r, stride)
                assert got == exp * r, (curve, name, h, [(i["family"], g) for i, g, e in zip(group * r, got, exp * r) if g != e][:6])
                assert verify_dev(cv, alg, HT[h], b"".join(pubs) * r, sigs * r, inp * r, stride) == exp * r, (curve, name, h, "dev")
            seen += len(group)
        assert seen == len(fx[name]["verify"])
        seen = 0
        for h, group in sorted(by_hash(fx[name]["sign"]).items()):
            # x and k that do not fit the qlen bytes of the interface (q + 1 where q is just below 2^(8 qlen)) are recorded as the
            # all-ones value by the generator already (min(top, q + 1)); the file holds qlen + 1 bytes of each
            xi, ki = [int(i["x"], 16) for i in group], [int(i["k"], 16) for i in group]
            assert max(xi + ki) <= top
            xs, ks = b"".join(x.to_bytes(ql, "big") for x in xi), b"".join(k.to_bytes(ql, "big") for k in ki)
            msgs = [bytes.fromhex(i["msg"]) for i in group]
            inp, stride = inputs_for(curve, alg, h, [key_of(curve, alg, x) for x in xi], msgs)
            sl = S.r_len(alg, h, ql) + ql
            sigs = b"".join(bytes.fromhex(i["out"]) if i["ret"] == 0 else bytes(sl) for i in group)
            st = bytes(0 if i["ret"] == 0 else 1 for i in group)
            for r in reps:
                assert cv.sig_hashed_sign(alg, HT[h], xs * r, ks * r, inp * r, stride) == (sigs * r, st * r), (curve, name, h)
                assert sign_dev(cv, alg, HT[h], xs * r, ks * r, inp * r, stride) == (sigs * r, st * r), (curve, name, h, "dev")
            seen += len(group)
        assert seen == len(fx[name]["sign"])


@pytest.mark.parametrize("curve", S.CURVES)
def test_fixture_item_for_item(gpu_ctx, curve):
    cv = gpu_ctx.curve(curve)
    try:
        run_fixture(cv, curve)
    finally:
        cv.free()


@pytest.mark.parametrize("curve", S.CURVES)
def test_fixture_on_a_handle_from_params(gpu_ctx, curve):
    """a fresh ecamd_curve_from_params handle: first batches too small for a comb table of the generator, then batches that build it"""
    import libecc_amd
    cv = libecc_amd.Curve(gpu_ctx, params=O.CURVES[curve])
    try:
        run_fixture(cv, curve, reps=(1, 8))
    finally:
        cv.free()


def random_signed(cv, curve, alg, h, n, seed, msg_lens=(24,)):
    """n random (x, k, message) signed on the device, the public keys from the device's own fixed-base multiplication:
    (pubs, sigs, status, inputs, stride, xb, kb, msgs)"""
    q, ql, cl = O.CURVES[curve]["q"], O.qlen(curve), O.clen(curve)
    rng = np.random.default_rng(seed)

    def scalars():
        raw = rng.integers(0, 256, size=(n, ql + 8), dtype=np.uint8)
        return [1 + int.from_bytes(row.tobytes(), "big") % (q - 1) for row in raw]
    xs, ks = scalars(), scalars()
    xb = b"".join(x.to_bytes(ql, "big") for x in xs)
    kb = b"".join(k.to_bytes(ql, "big") for k in ks)
    keysc = b"".join(pow(x, -1, q).to_bytes(ql, "big") for x in xs) if alg == S.ECKCDSA else xb
    pubs, st = cv.scalar_mult(keysc)
    assert st == bytes(n)
    msgs = [rng.integers(0, 256, size=msg_lens[i % len(msg_lens)], dtype=np.uint8).tobytes() for i in range(n)]
    inp, stride = inputs_for(curve, alg, h, [pubs[2 * cl * i:2 * cl * (i + 1)] for i in range(n)], msgs)
    sigs, sst = cv.sig_hashed_sign(alg, HT[h], xb, kb, inp, stride)
    return pubs, sigs, sst, inp, stride, xb, kb, msgs


@pytest.mark.parametrize("curve", S.CURVES)
def test_random_batch_against_the_reference(gpu_ctx, curve):
    """2^14 items (256-bit fields and below) or 2^11: half honest (made by ec_sig_hashed_sign_batch), a quarter with one bit of the
    signature changed, a quarter with random r and s; every verdict is the reference's, and a sample of the signatures is what the
    reference signs with the same nonce"""
    if not O.have_ref():
        pytest.skip("oracle/_ref/libecc_ref.so is not built here")
    cv = gpu_ctx.curve(curve)
    q, ql, cl = O.CURVES[curve]["q"], O.qlen(curve), O.clen(curve)
    n = 1 << 14 if O.CURVES[curve]["p"].bit_length() <= 256 else 1 << 11
    try:
        for name, alg in ALGS:
            for h in S.hashes_for(curve)[:2]:
                pubs, sigs, sst, inp, stride, xb, kb, msgs = random_signed(cv, curve, alg, h, n, 9700 + alg, msg_lens=(24, 0, 119, 56))
                assert sst == bytes(n), (curve, name, h)
                sl = S.r_len(alg, h, ql) + ql
                rng = np.random.default_rng(9800 + alg)
                sg = bytearray(sigs)
                for i in range(n // 2, 3 * n // 4):
                    sg[sl * i + int(rng.integers(0, sl))] ^= 1 << int(rng.integers(0, 8))
                for i in range(3 * n // 4, n):
                    sg[sl * i:sl * (i + 1)] = rng.integers(0, 256, size=sl - ql, dtype=np.uint8).tobytes() + \
                        (1 + SF.rand_int(rng, q - 1)).to_bytes(ql, "big")
                sg = bytes(sg)
                got = cv.sig_hashed_verify(alg, HT[h], pubs, sg, inp, stride)
                assert got[:n // 2] == bytes(n // 2), (curve, name, h, "an honest signature was rejected")
                ref = O.join_slices(O.in_slices(lambda lo, hi: bytes(
                    0 if S.ref_verify(curve, alg, h, pubs[2 * cl * i:2 * cl * (i + 1)], sg[sl * i:sl * (i + 1)], msgs[i]) == 0 else 1
                    for i in range(lo, hi)), n))
                assert got == ref, (curve, name, h, [i for i in range(n) if got[i] != ref[i]][:8])
                assert verify_dev(cv, alg, HT[h], pubs, sg, inp, stride) == ref, (curve, name, h, "dev")
                for i in range(0, n, n // 32):
                    ret, rsig = S.ref_sign(curve, alg, h, int.from_bytes(xb[ql * i:ql * (i + 1)], "big"),
                                           int.from_bytes(kb[ql * i:ql * (i + 1)], "big"), msgs[i])
                    assert (ret, rsig) == (0, sigs[sl * i:sl * (i + 1)]), (curve, name, h, i)
                print(curve, name, h, "accepted", got.count(0), "of", n)
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP256K1", "SECP384R1", "SECP224K1", "WEI25519"])
def test_sign_verify_round_trip(gpu_ctx, curve):
    """2^14 signatures per scheme and hash, over every padding-boundary message length, verify; with one message bit (ECKCDSA:
    one bit of h) changed none does.  Where the reference is built, the signatures at every length are its own."""
    cv = gpu_ctx.curve(curve)
    n = 1 << 14
    ql = O.qlen(curve)
    try:
        for name, alg in ALGS:
            for h in S.hashes_for(curve):
                pubs, sigs, sst, inp, stride, xb, kb, msgs = random_signed(cv, curve, alg, h, n, 9900 + alg, msg_lens=S.PAD_EDGES)
                assert sst == bytes(n), (curve, name, h)
                assert cv.sig_hashed_verify(alg, HT[h], pubs, sigs, inp, stride) == bytes(n), (curve, name, h)
                bad = bytearray(inp)
                for i in range(n):
                    bad[stride * i + (stride - 1 if alg == S.ECKCDSA else 4 + S.blank_len(alg, O.clen(curve)))] ^= 0x10
                # (a message of length 0 has no bit to change: its slot's padding byte is not hashed, the item still verifies)
                exp = bytes(0 if alg != S.ECKCDSA and len(msgs[i]) == 0 else 1 for i in range(n))
                assert cv.sig_hashed_verify(alg, HT[h], pubs, sigs, bytes(bad), stride) == exp, (curve, name, h)
                if O.have_ref():
                    sl = S.r_len(alg, h, ql) + ql
                    for i in range(len(S.PAD_EDGES)):
                        ret, rsig = S.ref_sign(curve, alg, h, int.from_bytes(xb[ql * i:ql * (i + 1)], "big"),
                                               int.from_bytes(kb[ql * i:ql * (i + 1)], "big"), msgs[i])
                        assert (ret, rsig) == (0, sigs[sl * i:sl * (i + 1)]), (curve, name, h, len(msgs[i]))
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP256K1"])
def test_large_batch_in_chunks(gpu_ctx, curve):
    """2^20 items with max_chunk below n: a signed 2^14-item block of mixed message lengths repeated, with the fixture's items
    of each hash (all but the one 4096-byte slot, which is asserted) laid over the chunk boundaries; signing the same batch in
    chunks gives the block's bytes"""
    cv = gpu_ctx.curve(curve)
    n, block, chunk = 1 << 20, 1 << 14, 300000
    cl, ql = O.clen(curve), O.qlen(curve)
    fx = load(curve)
    try:
        for name, alg in ALGS:
            for h in S.hashes_for(curve):
                pubs, sigs, sst, inp, stride, xb, kb, _ = random_signed(cv, curve, alg, h, block, 9300 + alg, msg_lens=(0, 1, 55, 56, 63, 64, 111, 120))
                assert sst == bytes(block)
                sl = S.r_len(alg, h, ql) + ql
                reps = n // block
                P, Sg, D, exp = bytearray(pubs * reps), bytearray(sigs * reps), bytearray(inp * reps), bytearray(n)
                # every recorded item of this hash but the one 4096-byte slot ("longest": a 2^20-item array of that stride is 4 GiB)
                items = [i for i in fx[name]["verify"] if i["hash"] == h and len(i["msg"]) // 2 <= 120]
                left_out = [i["family"] for i in fx[name]["verify"] if i["hash"] == h and len(i["msg"]) // 2 > 120]
                assert set(left_out) <= {"longest"} and len(left_out) <= 1, (curve, name, h, left_out)
                assert {i["family"] for i in items} >= {"honest", "r_zero_mod_q", "w_infinity", "equal_operands", "pad_edges"}
                if h == S.hashes_for(curve)[0]:
                    assert {i["family"] for i in items} >= {"tampered", "s_range", "key_not_importable", "foreign_scheme"}
                for b in range(1, 4):
                    for j, it in enumerate(items):
                        k = b * chunk - len(items) // 2 + j
                        pub, msg = bytes.fromhex(it["pub"]), bytes.fromhex(it["msg"])
                        P[2 * cl * k:2 * cl * (k + 1)] = pub
                        Sg[sl * k:sl * (k + 1)] = bytes.fromhex(it["sig"])
                        D[stride * k:stride * (k + 1)] = inputs_for(curve, alg, h, [pub], [msg], stride)[0]
                        exp[k] = 0 if it["ret"] == 0 else 1
                gpu_ctx.set_max_chunk(chunk)
                try:
                    got = cv.sig_hashed_verify(alg, HT[h], bytes(P), bytes(Sg), bytes(D), stride)
                    gdev = verify_dev(cv, alg, HT[h], bytes(P), bytes(Sg), bytes(D), stride)
                    ssig, sst2 = cv.sig_hashed_sign(alg, HT[h], xb * reps, kb * reps, inp * reps, stride)
                finally:
                    gpu_ctx.set_max_chunk(1 << 20)
                assert got == bytes(exp), (curve, name, [k for k in range(n) if got[k] != exp[k]][:8])
                assert gdev == bytes(exp), (curve, name, "dev")
                assert (ssig, sst2) == (sigs * reps, bytes(n)), (curve, name, "sign")
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP256K1", "SECP521R1"])
def test_redo_items_among_ordinary_ones(gpu_ctx, curve):
    """items that leave the shared-denominator path -- W' at infinity, a doubling, and ECKCDSA's e = 0 ([e]G at infinity), one of
    them ACCEPTED (h chosen to end in r: the entry point takes h from the caller) -- inside groups of ordinary items"""
    cv = gpu_ctx.curve(curve)
    cl, ql = O.clen(curve), O.qlen(curve)
    fx = load(curve)
    n = 256
    try:
        for name, alg in ALGS:
            for h in S.hashes_for(curve):
                pubs, sigs, sst, inp, stride, _, _, _ = random_signed(cv, curve, alg, h, n, 9400 + alg, msg_lens=(48,))
                assert sst == bytes(n)
                sl = S.r_len(alg, h, ql) + ql
                P, Sg, D, exp = bytearray(pubs), bytearray(sigs), bytearray(inp), bytearray(n)
                special = [(bytes.fromhex(i["pub"]), bytes.fromhex(i["sig"]),
                            inputs_for(curve, alg, h, [bytes.fromhex(i["pub"])], [bytes.fromhex(i["msg"])], stride)[0], 0 if i["ret"] == 0 else 1)
                           for i in fx[name]["verify"] if i["hash"] == h and i["family"] in ("w_infinity", "equal_operands", "e_zero")]
                assert len(special) >= 2
                if alg == S.ECKCDSA:
                    rng = np.random.default_rng(9450)
                    for _ in range(3):
                        pub, sig, hh = S.kcdsa_e_zero_accepted(curve, h, rng)
                        special.append((pub, sig, hh, 0))
                for j, (pub, sig, di, e) in enumerate(special):
                    k = 3 + 11 * j          # different positions within the groups of eight
                    P[2 * cl * k:2 * cl * (k + 1)], Sg[sl * k:sl * (k + 1)], D[stride * k:stride * (k + 1)], exp[k] = pub, sig, di, e
                got = cv.sig_hashed_verify(alg, HT[h], bytes(P), bytes(Sg), bytes(D), stride)
                assert got == bytes(exp), (curve, name, h, [k for k in range(n) if got[k] != exp[k]])
                assert verify_dev(cv, alg, HT[h], bytes(P), bytes(Sg), bytes(D), stride) == bytes(exp), (curve, name, h, "dev")
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP256K1", "SECP384R1"])
def test_secret_scalar_mode_gives_the_same_bytes(gpu_ctx, curve):
    cv = gpu_ctx.curve(curve)
    n = 1 << 11
    try:
        for name, alg in ALGS:
            for h in S.hashes_for(curve)[:2]:
                pubs, sigs, sst, inp, stride, xb, kb, _ = random_signed(cv, curve, alg, h, n, 9500 + alg)
                gpu_ctx.set_secret_scalars(True)
                try:
                    assert cv.sig_hashed_sign(alg, HT[h], xb, kb, inp, stride) == (sigs, sst), (curve, name, h)
                    assert cv.sig_hashed_verify(alg, HT[h], pubs, sigs, inp, stride) == bytes(n), (curve, name, h)
                finally:
                    gpu_ctx.set_secret_scalars(False)
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP256K1"])
def test_signatures_of_ecdsa_and_ecgdsa_are_no_signatures_here(gpu_ctx, curve):
    cv = gpu_ctx.curve(curve)
    q, ql, cl = O.CURVES[curve]["q"], O.qlen(curve), O.clen(curve)
    n = 512
    rng = np.random.default_rng(9600)
    try:
        xs = b"".join((1 + SF.rand_int(rng, q - 2)).to_bytes(ql, "big") for _ in range(n))
        ks = b"".join((1 + SF.rand_int(rng, q - 1)).to_bytes(ql, "big") for _ in range(n))
        msgs = [rng.integers(0, 256, size=24, dtype=np.uint8).tobytes() for _ in range(n)]
        dgs = b"".join(S.H("SHA256", m) for m in msgs)
        pubs, st = cv.scalar_mult(xs)
        assert st == bytes(n)
        esig, est = cv.ecdsa_sign(xs, ks, dgs, 32)
        gsig, gst = cv.sig_sign(SF.ECGDSA, xs, ks, dgs, 32)
        assert est == bytes(n) and gst == bytes(n) and cv.ecdsa_verify(pubs, esig, dgs, 32) == bytes(n)
        for name, alg in ALGS:
            inp, stride = inputs_for(curve, alg, "SHA256", [pubs[2 * cl * i:2 * cl * (i + 1)] for i in range(n)], msgs)
            for sigs in (esig, gsig):   # hsize = qlen = 32: the sizes agree
                assert cv.sig_hashed_verify(alg, HT["SHA256"], pubs, sigs, inp, stride) == b"\1" * n, (curve, name)
    finally:
        cv.free()


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP521R1"])
def test_unusable_slots(gpu_ctx, curve):
    """a length word shorter than the blank, or one that does not fit the stride, is result / status 1 (with zero signature
    bytes); its neighbours are untouched.  A stride that cannot hold the blank rejects every item."""
    cv = gpu_ctx.curve(curve)
    cl, ql = O.clen(curve), O.qlen(curve)
    n = 64
    try:
        for name, alg in ALGS:
            if alg == S.ECKCDSA:
                continue
            h = "SHA256"
            pubs, sigs, sst, inp, stride, xb, kb, _ = random_signed(cv, curve, alg, h, n, 9650 + alg)
            bl = S.blank_len(alg, cl)
            sl = S.r_len(alg, h, ql) + ql
            D, exp, esig = bytearray(inp), bytearray(n), bytearray(sigs)
            for k, ln in ((5, bl - 1), (6, 0), (17, stride - 3), (18, 0xFFFFFFFF), (40, stride)):
                D[stride * k:stride * k + 4] = ln.to_bytes(4, "little")
                exp[k] = 1
                esig[sl * k:sl * (k + 1)] = bytes(sl)
            D[stride * 7:stride * 7 + 4] = bl.to_bytes(4, "little")      # the empty message: usable, but another message
            got = cv.sig_hashed_verify(alg, HT[h], pubs, sigs, bytes(D), stride)
            assert got[7] == 1 and got[:7] + got[8:] == bytes(exp[:7] + exp[8:]), (curve, name)
            ssig, sst2 = cv.sig_hashed_sign(alg, HT[h], xb, kb, bytes(D), stride)
            assert sst2[:7] + sst2[8:] == bytes(exp[:7] + exp[8:]) and sst2[7] == 0, (curve, name)
            assert ssig[:sl * 7] + ssig[sl * 8:] == bytes(esig[:sl * 7] + esig[sl * 8:]), (curve, name)
            small = (4 + bl - 4) & ~3
            assert cv.sig_hashed_verify(alg, HT[h], pubs, sigs, bytes(small * n), small) == b"\1" * n
            assert cv.sig_hashed_sign(alg, HT[h], xb, kb, bytes(small * n), small) == (bytes(sl * n), b"\1" * n)
    finally:
        cv.free()


def test_argument_errors_and_empty_batches(gpu_ctx):
    import libecc_amd
    cv = gpu_ctx.curve("SECP256R1")
    try:
        for alg in (S.ECKCDSA, S.ECSDSA, S.ECOSDSA):
            stride = 32 if alg == S.ECKCDSA else 128
            assert cv.sig_hashed_verify(alg, 2, b"", b"", b"", stride) == b""
            assert cv.sig_hashed_sign(alg, 2, b"", b"", b"", stride) == (b"", b"")
            for ht in (0, 5, 6, 12):   # SHA-3 and the others have no kernel here
                with pytest.raises(libecc_amd.EcamdError):
                    cv.sig_hashed_verify(alg, ht, bytes(64), bytes(64), bytes(stride), stride)
                with pytest.raises(libecc_amd.EcamdError):
                    cv.sig_hashed_sign(alg, ht, bytes(32), bytes(32), bytes(stride), stride)
            for bad in ((130, 4100, 0) if alg != S.ECKCDSA else (28, 64, 0)):
                with pytest.raises(libecc_amd.EcamdError):
                    cv.sig_hashed_verify(alg, 2, bytes(64), bytes(64), bytes(4200), bad)
                with pytest.raises(libecc_amd.EcamdError):
                    cv.sig_hashed_sign(alg, 2, bytes(32), bytes(32), bytes(4200), bad)
        for alg in (0, 1, 5, 6, 7, 8, 9):   # ECDSA and the ECDSA-shaped schemes have their own entry points
            with pytest.raises(libecc_amd.EcamdError):
                cv.sig_hashed_verify(alg, 2, bytes(64), bytes(64), bytes(128), 128)
            with pytest.raises(libecc_amd.EcamdError):
                cv.sig_hashed_sign(alg, 2, bytes(32), bytes(32), bytes(128), 128)
        # NULL arguments with n > 0, a NULL context or curve, and a curve handle of another context: -1 before anything is launched,
        # in the host and the _dev forms (the non-NULL "device pointers" below are never dereferenced)
        L, ch, vh = cv.L, cv.ctx.h, cv.h
        other = libecc_amd.Context(0)
        try:
            ov = other.curve("SECP256R1")
            try:
                for alg, stride in ((S.ECKCDSA, 32), (S.ECSDSA, 128)):
                    good_v = [bytes(64), bytes(96), bytes(128), bytes(1)]
                    good_s = [bytes(32), bytes(32), bytes(128), bytes(96), bytes(1)]
                    for hole in range(4):
                        a = list(good_v)
                        a[hole] = None
                        assert L.ec_sig_hashed_verify_batch(ch, vh, alg, 2, 1, a[0], a[1], a[2], stride, a[3]) == -1, (alg, hole)
                        d = [None if k == hole else 4096 for k in range(4)]
                        assert L.ec_sig_hashed_verify_batch_dev(ch, vh, alg, 2, 1, d[0], d[1], d[2], stride, d[3], None) == -1, (alg, hole)
                    for hole in range(5):
                        a = list(good_s)
                        a[hole] = None
                        assert L.ec_sig_hashed_sign_batch(ch, vh, alg, 2, 1, a[0], a[1], a[2], stride, a[3], a[4]) == -1, (alg, hole)
                        d = [None if k == hole else 4096 for k in range(5)]
                        assert L.ec_sig_hashed_sign_batch_dev(ch, vh, alg, 2, 1, d[0], d[1], d[2], stride, d[3], d[4], None) == -1, (alg, hole)
                    for c, v in ((None, vh), (ch, None), (ch, ov.h), (other.h, vh)):
                        assert L.ec_sig_hashed_verify_batch(c, v, alg, 2, 1, *good_v[:3], stride, good_v[3]) == -1
                        assert L.ec_sig_hashed_sign_batch(c, v, alg, 2, 1, *good_s[:3], stride, *good_s[3:]) == -1
                        assert L.ec_sig_hashed_verify_batch_dev(c, v, alg, 2, 1, 4096, 4096, 4096, stride, 4096, None) == -1
                        assert L.ec_sig_hashed_sign_batch_dev(c, v, alg, 2, 1, 4096, 4096, 4096, stride, 4096, 4096, None) == -1
                    assert L.ecamd_last_error()
                    # the _dev forms refuse a bad alg, hash_type and stride as the host forms do; n = 0 is no work with any pointers
                    for al, ht, st_ in ((9, 2, stride), (alg, 5, stride), (alg, 2, 130), (alg, 2, 0)):
                        assert L.ec_sig_hashed_verify_batch_dev(ch, vh, al, ht, 1, 4096, 4096, 4096, st_, 4096, None) == -1
                        assert L.ec_sig_hashed_sign_batch_dev(ch, vh, al, ht, 1, 4096, 4096, 4096, st_, 4096, 4096, None) == -1
                    assert L.ec_sig_hashed_verify_batch_dev(ch, vh, alg, 2, 0, None, None, None, stride, None, None) == 0
                    assert L.ec_sig_hashed_sign_batch_dev(ch, vh, alg, 2, 0, None, None, None, stride, None, None, None) == 0
            finally:
                ov.free()
        finally:
            other.close()
    finally:
        cv.free()
