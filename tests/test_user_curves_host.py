"""The chain of references for user-defined curves, proven without a GPU: tests/golden/user_curves.json is sound (primes, the
generator, the orders), and on every batch of tests/user_curves.py the Python integers (a), the restatement oracle (b) and the
recorded answers of the unmodified reference (c, bitlen(p) <= 521) say the same."""
import pytest

import oracles as O
import user_curves as U

CURVES = U.load()
NAMES = sorted(CURVES)
# the field sizes this work exists for, and the two extreme primes
WANTED = {160, 161, 200, 233, 257, 300, 350, 400, 480, 513, 521, 544, 256, 512}


def _slices(buf, width, idx):
    return [buf[width * i:width * (i + 1)] for i in idx]


def test_fixture_covers_the_sizes():
    assert {U.pbits(cv) for cv in CURVES.values()} >= WANTED
    assert {U.words(cv) for cv in CURVES.values()} == set(U.WIDTHS)
    for cv in CURVES.values():
        # the reference's answers are recorded exactly where its default build holds the curve
        assert (cv["ref"] is not None) == (U.pbits(cv) <= 521), cv["name"]
    big = CURVES["U544A"]
    assert big["p"] > (1 << 543) + (1 << 542)
    assert CURVES["X256A"]["p"] >> 200 == 1 << 55 and (CURVES["X512A"]["p"] >> 200) + 1 == 1 << 312
    assert CURVES["U521B"]["p"] != (1 << 521) - 1
    assert (U.clen(CURVES["U257A"]), U.qlen(CURVES["U257A"])) == (33, 32)
    assert CURVES["U513A"]["q"].bit_length() == 511
    assert CURVES["U200B"]["p"] % 8 == 5 and CURVES["U300B"]["p"] % 8 == 1


@pytest.mark.parametrize("name", NAMES)
def test_curve_is_what_it_claims(name):
    cv = CURVES[name]
    p, q, h = cv["p"], cv["q"], cv["h"]
    assert U.is_prime(p) and U.is_prime(q)
    assert cv["order"] == h * q == p + 1
    if cv["family"] == "A":
        assert h == 4 and p % 4 == 3 and cv["b"] == 0 and 0 < cv["a"] < p       # supersingular: #E = p + 1
    else:
        assert h == 6 and p % 3 == 2 and cv["a"] == 0 and 0 < cv["b"] < p
    G = (cv["gx"], cv["gy"])
    assert U.on_curve(G, cv) and U.mul(q, G, cv) is None
    S = U.special_points(cv)
    assert all(U.on_curve(P, cv) and U.mul(q, P, cv) is None for P in S["sub"])
    assert U.on_curve(S["full"], cv) and U.mul(q, S["full"], cv) is not None and U.mul(h * q, S["full"], cv) is None
    assert S["two"][1] == 0 and U.on_curve(S["two"], cv)
    # the batches are the ones the reference answered
    if cv["ref"] is not None:
        assert U.batch_hashes(cv) == cv["sha256"]


@pytest.mark.parametrize("name", NAMES)
def test_scalar_mult_references_agree(name):
    cv = CURVES[name]
    o = O.Oracle(cv)
    for label, slen, sc, pts in U.smul_batches(cv):
        out, st = o.scalar_mult(sc, pts, slen=slen)
        n = len(st)
        if cv["ref"] is not None:
            assert U.pack(U.ref_items(cv, label), st, out) == cv["ref"]["smul"][label], label
        idx = U.sample(n, 4 if label.startswith("fixed") else 6)
        cl = U.clen(cv)
        items = [(int.from_bytes(sc[slen * i:slen * (i + 1)], "big"), None if pts is None else pts[2 * cl * i:2 * cl * (i + 1)]) for i in idx]
        pout, pst = U.py_smul(cv, items)
        assert (pout, pst) == (b"".join(_slices(out, 2 * cl, idx)), bytes(st[i] for i in idx)), label
    # every kind of answer is in the variable-base batch: a point, the reference's -1, infinity
    st = o.scalar_mult(*[(b[2], b[3]) for b in U.smul_batches(cv) if b[0] == "var/q"][0])[1]
    assert set(st) == {0, 1, 2}


@pytest.mark.parametrize("name", NAMES)
def test_point_add_references_agree(name):
    cv = CURVES[name]
    o = O.Oracle(cv)
    A, B, exc = U.add_batch(cv)
    cl = U.clen(cv)
    n = len(A) // (2 * cl)
    for key, res in (("add", o.pt_add(A, B)), ("dbl", o.pt_add(A))):
        if cv["ref"] is not None:
            assert U.pack(U.ref_items(cv, key), res[1], res[0]) == cv["ref"][key], key
        pairs = list(zip(_slices(A, 2 * cl, range(n)), _slices(B, 2 * cl, range(n))))
        assert U.py_add(cv, pairs, dbl=(key == "dbl")) == res, key       # no scalar multiplication here: the whole batch
    st = o.pt_add(A, B)[1]
    # the point of order two T is an operand like any other (T + T: infinity); Q = P + T makes P - Q of order two, the
    # reference's "exceptional pair"
    assert st[exc:exc + 4] == b"\x00\x00\x00\x02" and st[exc + 4:exc + 9] == b"\x01" * 5 and set(st[exc + 9:]) == {1}
    assert set(st[:exc]) == {0, 2}


@pytest.mark.parametrize("name", NAMES)
def test_ecdsa_references_agree(name):
    cv = CURVES[name]
    o = O.Oracle(cv)
    ql, cl, hl = U.qlen(cv), U.clen(cv), U.hash_of(cv)().digest_size
    privs, nonces, _, _, digests = U.sign_batch(cv)
    sigs, st = o.ecdsa_sign(privs, nonces, digests, hl)
    n = len(st)
    sigs = b"".join(sigs[2 * ql * i:2 * ql * (i + 1)] if st[i] == 0 else bytes(2 * ql) for i in range(n))
    assert st == bytes(16) + b"\x01" * 4       # the last four: a private key or a nonce that is 0 or not below q
    if cv["ref"] is not None:
        assert U.pack(U.ref_items(cv, "sign"), st, sigs) == cv["ref"]["sign"]
    idx = U.sample(n, 10)
    items = [(int.from_bytes(privs[ql * i:ql * (i + 1)], "big"), int.from_bytes(nonces[ql * i:ql * (i + 1)], "big"),
              digests[hl * i:hl * (i + 1)]) for i in idx]
    assert U.py_sign(cv, items) == (b"".join(_slices(sigs, 2 * ql, idx)), bytes(st[i] for i in idx))

    pubs, vs, _, _, vd, by_msg = U.verify_batch(cv)
    res = o.ecdsa_verify(pubs, vs, vd, hl)
    n = len(res)
    tail = 0 if 8 * hl > cv["q"].bit_length() else 1       # the digest's last bit is shifted out of e where the digest is longer than q
    assert res[:6] == bytes(6) and res[10] == tail and set(res[6:10] + res[11:]) == {1}
    if cv["ref"] is not None:
        rec = bytes.fromhex(cv["ref"]["verify"])
        assert [rec[i] for i in range(n) if by_msg[i]] == [res[i] for i in range(n) if by_msg[i]]
    idx = sorted(set(U.sample(n, 8)) | {i for i in range(n) if not by_msg[i]})
    items = [(pubs[2 * cl * i:2 * cl * (i + 1)], vs[2 * ql * i:2 * ql * (i + 1)], vd[hl * i:hl * (i + 1)]) for i in idx]
    assert U.py_verify(cv, items) == bytes(res[i] for i in idx)


@pytest.mark.parametrize("name", NAMES)
def test_y_from_x_references_agree(name):
    cv = CURVES[name]
    xs = U.yfx_batch(cv)
    cl = U.clen(cv)
    y1, y2, st = O.Oracle(cv).y_from_x(xs)
    if cv["ref"] is not None:
        assert U.pack(U.ref_items(cv, "yfx"), st, y1, y2) == cv["ref"]["yfx"]
    py = U.py_y_from_x(cv, xs)
    assert set(st) == {0, 1}
    for i, roots in enumerate(py):
        assert (st[i] == 0) == (roots is not None), i
        if roots is not None:
            assert {int.from_bytes(y1[cl * i:cl * (i + 1)], "big"), int.from_bytes(y2[cl * i:cl * (i + 1)], "big")} == roots, i


@pytest.mark.parametrize("name", NAMES)
def test_field_references_agree(name):
    cv = CURVES[name]
    A, B = U.field_batch(cv)
    assert len(A) == len(B) <= 512 and max(A + B) < cv["p"]
    o = O.Oracle(cv)
    for op in range(5):
        assert o.fp_op(op, A, B) == U.py_field(cv, op, A, B), op


def test_top_carry_branch_is_reached_on_the_544_bit_curve():
    """p fills its 17 words, so t = (a b + m p) / R can pass R = 2^544: only the carry word then tells the Montgomery product's
    final step to subtract.  At least a quarter of the batch's products take that branch; a curve with spare bits never does."""
    cv = CURVES["U544A"]
    A, B = U.field_batch(cv)
    assert 4 * U.top_carry_count(cv, A, B) >= len(A)
    other = CURVES["U513A"]
    assert U.top_carry_count(other, *U.field_batch(other)) == 0
