"""secp256r1's own radix-2^29 unit (ecamd_u29.h, ecamd_p256.h) as the DEVICE compiles it: tests/u29_device_shim.hip built with
the product's flags (-DU29_ASM_MAD) on the vectors of tests/u29_vectors.py, in the manner of tests/test_gpu_u29g_units.py: per
operation all records in one launch, the extreme ones on lane 0, lane 63, the first lane of the second wave and in the last,
partial wave; (a) residues and flags of Python integers and (b) the bound-class assertions of the host test, both by replaying the
generators on the device's outputs; (c) limb-for-limb equality with the g++ build of the same entry point."""
import ctypes as C
import os
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import u29_device as D  # noqa: E402
import u29_vectors as V  # noqa: E402

pytestmark = pytest.mark.gpu


def test_secp256r1_unit_on_the_device():
    t0 = time.time()
    host = V.host_lib()
    dev = C.CDLL(D.build()["p256"])     # built beforehand as a rule; built here when missing or stale; a failure to build fails
    assert dev.gd_flags() == 1 | (D.FLAVOUR_ID["p256"] << 8)    # the asm branches: a build on the portable ones cannot pass
    consts = (C.c_uint32 * 49)()
    assert dev.gd_p256_consts(consts) == 0
    V.check_consts(list(consts))
    assert list(consts) == V.call(host.t_consts, n_out=49)[0]
    done = {n: V.drive(g(), host) for n, g in V.GENERATORS}
    counts = V.check_counts(done)
    groups = {}
    for n, d in done.items():
        for j, (rec, out, r) in enumerate(d):
            groups.setdefault((rec.op, rec.arg), []).append((n, j))
    dev_done = {n: [None] * len(d) for n, d in done.items()}
    t1 = time.time()
    for (op, arg), where in groups.items():
        members = [done[n][j] for n, j in where]
        lanes = D.place([rec.edge for rec, _, _ in members])
        assert len(lanes) > 64 and len(lanes) % 64 != 0
        outs, flags = D.run_p(dev, op, arg, [members[i][0].ins for i in lanes], V.N_OUT[op])
        for lane, i in enumerate(lanes):
            rec, hout, hr = members[i]
            assert outs[lane] == hout, (op, arg, "lane", lane, "record", i, "device", outs[lane], "host", hout)
            if op in V.FLAGGED:
                assert flags[lane] == hr, (op, arg, "lane", lane, "record", i, flags[lane], hr)
            n, j = where[i]
            dev_done[n][j] = (rec, outs[lane], flags[lane] if op in V.FLAGGED else 0)
    # oracles (a) and (b): the generators' own assertions on the device's outputs
    for n, g in V.GENERATORS:
        V.replay(g(), dev_done[n])
    # the multiplication at one lane, one short of a wave, a full wave, one over
    muls = [m for m in done["mul_sqr"] if m[0].op == "mul"]
    muls = muls[300:] + muls[:300]        # the extreme pairs first
    for n in (1, 63, 64, 65):
        outs, _ = D.run_p(dev, "mul", None, [muls[i][0].ins for i in range(n)], 9)
        for i in range(n):
            assert outs[i] == muls[i][1], ("mul", "n", n, "lane", i)
            lx, ly = muls[i][0].ins
            assert V.val(outs[i]) % V.p == V.val(lx) * V.val(ly) * V.Rinv % V.p
    t2 = time.time()
    print("\nsecp256r1 unit: %.2f s in all, %.2f s of it launches, comparisons and replay; records per operation %s"
          % (t2 - t0, t2 - t1, dict(sorted(counts.items()))))
