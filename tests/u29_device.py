"""Build helper of the device shims (tests/u29g_device_shim.hip, tests/u29_device_shim.hip): one shared
object per flag set of the product's radix-2^29 units in tests/_build/, compiled with the compiler, the
flags and the per-unit -D flags of libecc_amd/build.py itself (HIPCC, FLAGS, _jobs()), so that a shim can
never be built differently from the product.  -DG29_PB / -DG29_WAVES belong to the kernel file only and
are dropped.  An object is rebuilt only when it is missing or older than the shim or a header; at most
eight compilers run at a time, as in build.py.

Cold build of all nine objects, eight compilers in parallel: 74 s of wall time measured where this was written
(the dense object with its ten sizes is the longest single compile); the product build takes two to three minutes."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from libecc_amd import build as B  # noqa: E402

TESTS = os.path.join(ROOT, "tests")
BUILD = os.path.join(TESTS, "_build")
G_SHIM = os.path.join(TESTS, "u29g_device_shim.hip")
P_SHIM = os.path.join(TESTS, "u29_device_shim.hip")
G_HEADERS = ["ecamd_madchain.h", "ecamd_u29g.h", "ecamd_jacg.h", "ecamd_rcbg.h"]
P_HEADERS = ["ecamd_madchain.h", "ecamd_u29.h", "ecamd_p256.h"]
KERNEL_ONLY = ("-DG29_PB=", "-DG29_WAVES=")
# gd_flags(): bit 0 = U29_ASM_MAD, bits 8.. = the flavour the object was compiled as
FLAVOUR_ID = {"dense": 0, "521m": 1, "255c": 2, "384n": 3, "256k": 4, "448g": 5, "224s": 6, "192s": 7, "p256": 8}
G_OPS = ["mul", "mulword", "canon", "neg", "inv", "add", "dbl", "madd", "dblt", "rcb", "liftx", "info", "infot"]
P_OPS = ["mul", "sqr", "mul_loose", "fold", "inv", "canonical_words", "from_words", "is_zero", "dbl", "add", "madd", "consts"]


def units():
    """{tag: (field sizes, flags)}: "dense" with every size of G29_SIZES, then one entry per flavoured unit of build._jobs()"""
    out = {"dense": (list(B.G29_SIZES), [])}
    for src, obj, extra in B._jobs():
        flav = [f for f in extra if not f.startswith(KERNEL_ONLY)]
        if src != "ecamd_g29_kernel.hip" or not flav or "-DG29_DISPATCH" in flav:
            continue
        pb = next(int(f.split("=")[1]) for f in extra if f.startswith("-DG29_PB="))
        tag = obj[len("ecamd_g29_"):-len(".o")]
        out[tag] = ([pb], flav + [f"-DSHIM_ONLY_{pb}"])
    return out


def so_path(tag):
    return os.path.join(BUILD, f"u29g_dev_{tag}.so" if tag != "p256" else "u29_dev_p256.so")


def symbols(tag):
    """every gd_* entry point the GPU tests may call on this object"""
    if tag == "p256":
        return ["gd_flags"] + [f"gd_p256_{op}" for op in P_OPS]
    return ["gd_flags"] + [f"gd_{op}_{pb}" for pb in units()[tag][0] for op in G_OPS]


def _jobs():
    jobs = [(tag, G_SHIM, G_HEADERS, flags) for tag, (_, flags) in units().items()]
    jobs.append(("p256", P_SHIM, P_HEADERS, []))
    return jobs


def build(force=False):
    """build what is missing or stale; returns {tag: path}.  Raises (never skips) when an object cannot be built."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(BUILD, exist_ok=True)
    todo, paths = [], {}
    for tag, shim, headers, flags in _jobs():
        so = paths[tag] = so_path(tag)
        cmd = [B.HIPCC] + B.FLAGS + flags + ["-x", "hip", shim, "-shared", "-o", so]
        try:
            same_cmd = open(so + ".cmd").read() == " ".join(cmd)
        except OSError:
            same_cmd = False
        if force or not same_cmd or B._stale(so, [shim] + [os.path.join(B.CSRC, h) for h in headers]):
            todo.append(cmd)

    def run(cmd):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("device shim does not build: %s\n%s" % (" ".join(cmd), r.stdout[-4000:]))
        with open(cmd[-1] + ".cmd", "w") as f:
            f.write(" ".join(cmd))

    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as ex:
        list(ex.map(run, todo))
    return paths


def load(tag):
    """the built object of a unit as a ctypes library (the HIP runtime comes with it: load it after torch)"""
    return C.CDLL(build()[tag])


def place(edges):
    """lane -> record index for one launch of len(edges) records (edges[i]: record i sits at the edge of its class).  More than two
    waves, the last one partial; the c edge records fill lanes [0, c), (63 - c, 63], [64, 64 + c) and the last c lanes, rotated so
    that the first four of them land on lane 0, lane 63, the first lane of the second wave and the last lane, and every one of them
    in each of the four places; every record sits at least once in the lanes between."""
    m = len(edges)
    E = [i for i, e in enumerate(edges) if e][:31] or [0]
    c = len(E)
    n = max(m + 4 * c, 130)
    n += 1 if n % 64 == 0 else 0
    lanes = [None] * n
    for t in range(c):
        for r, pos in enumerate((t, 63 - t, 64 + t, n - 1 - t)):
            lanes[pos] = E[(t + r) % c]
    free = [i for i in range(n) if lanes[i] is None]
    assert len(free) >= m
    for j, i in enumerate(free):
        lanes[i] = j % m
    return lanes


def _u32(rows):
    import numpy as np
    a = np.ascontiguousarray(np.array(rows, dtype=np.uint64).astype(np.uint32))
    return a, a.ctypes.data_as(C.POINTER(C.c_uint32))


def run_g(lib, f, op, arg, items):
    """one launch of a generic unit's kernel `op` on the curve image of the Field f: items = [operand limb lists] per lane.
    Returns ([output limbs] per lane, [flag word] per lane); the hipError_t of the call must be 0."""
    import numpy as np
    n, nl = len(items), f.nl
    n_out = {"mul": 1, "mulword": 1, "canon": 1, "neg": 1, "inv": 1, "add": 3, "dbl": 3, "madd": 3, "dblt": 3, "rcb": 3, "liftx": 2}[op] * nl
    ins = []
    for k in range(len(items[0])):
        a, ptr = _u32([it[k] for it in items])
        assert a.shape == (n, len(items[0][k]))
        ins.append((a, ptr))
    out = np.zeros((n, n_out), dtype=np.uint32)
    flag = np.zeros(n, dtype=np.uint32)
    po, pf = out.ctypes.data_as(C.POINTER(C.c_uint32)), flag.ctypes.data_as(C.POINTER(C.c_uint32))
    fn = getattr(lib, f"gd_{op}_{f.pb}")
    p = [x[1] for x in ins]
    if op == "mul":
        e = fn(f.k, p[0], p[1], po, arg, n)
    elif op == "mulword":
        e = fn(p[0], po, n)
    elif op in ("add", "liftx"):
        e = fn(f.k, *p, po, pf, n)
    elif op == "rcb":
        e = fn(f.k, p[0], p[1], po, pf, arg, n)
    else:
        e = fn(f.k, *p, po, n)
    assert e == 0, (op, f.pb, "hipError_t", e)
    return [[int(v) for v in row] for row in out], [int(v) for v in flag]


def run_p(lib, op, arg, items, n_out):
    """one launch of secp256r1's kernel `op`: items = [operand word lists] per lane, n_out result words per lane (0: the
    operation only answers with its flag word).  Returns ([output words] per lane, [flag word] per lane)."""
    import numpy as np
    n = len(items)
    ins = []
    for k in range(len(items[0])):
        a, ptr = _u32([it[k] for it in items])
        assert a.shape == (n, len(items[0][k]))
        ins.append((a, ptr))
    out = np.zeros((n, max(n_out, 1)), dtype=np.uint32)
    flag = np.zeros(n, dtype=np.uint32)
    po, pf = out.ctypes.data_as(C.POINTER(C.c_uint32)), flag.ctypes.data_as(C.POINTER(C.c_uint32))
    fn = getattr(lib, f"gd_p256_{op}")
    p = [x[1] for x in ins]
    if op == "is_zero":
        e = fn(p[0], pf, n)
    elif op == "add":
        e = fn(p[0], p[1], po, pf, n)
    elif op == "madd":
        e = fn(p[0], p[1], po, pf, arg, n)
    else:
        e = fn(*p, po, n)
    assert e == 0, (op, "hipError_t", e)
    return [[int(v) for v in row[:n_out]] for row in out], [int(v) for v in flag]


if __name__ == "__main__":
    import time
    t0 = time.time()
    for tag, path in build(force="--force" in sys.argv).items():
        print(tag, path)
    print("%.1f s" % (time.time() - t0))
