"""The main index's sort called on its own, and what it must return.

TEST INFRASTRUCTURE ONLY. tests/index_sort_probe.hip is compiled together with
the product's own sort.hip and kernels.hip (the compiler and flags of
rna_clique_amd/build.py, so the kernels under test are the product's) into
tests/_build/libindexsortprobe.so. The two product sources are compiled through
index_sort_probe_sort.hip and index_sort_probe_kernels.hip, which include them
unchanged; the first adds the host accessors of the index sort's geometry. The
library is never linked into librcgpu.so and never imported by rna_clique_amd.

The host references restate the contract in integer-exact numpy; neither calls
the kernels:

  entries  the keys sorted stably on the bits [32, 64)
  bucket   bucket[x] = first sorted entry whose top `bits` bits are >= x,
           x = 0 .. 2^bits (so bucket[2^bits] = n)
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

try:
    import numpy as np
except ImportError:   # build_probe() needs no numpy
    np = None

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "index_sort_probe.hip")
LIB = os.path.join(HERE, "_build", "libindexsortprobe.so")
PRODUCT_SOURCES = ["sort.hip", "kernels.hip"]
WRAPPERS = [os.path.join(HERE, "index_sort_probe_sort.hip"), os.path.join(HERE, "index_sort_probe_kernels.hip")]
W16 = 16   # index word, bases


def _product():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from rna_clique_amd import build
    return build


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    csrc = _product().CSRC
    deps = [SRC] + WRAPPERS + [os.path.join(csrc, s) for s in PRODUCT_SOURCES + ["device.h", "launch.h"]]
    return any(os.path.getmtime(d) > t for d in deps)


def build_probe(force=False):
    """Compile the probe and the product's sort.hip and kernels.hip (one object
    each, the product's compiler, flags and working directory) and link them
    into LIB."""
    if not force and not _stale():
        return LIB
    from concurrent.futures import ThreadPoolExecutor
    import tempfile
    b = _product()
    extra = os.environ.get("RC_EXTRA_FLAGS", "").split()
    cflags = [f for f in b.FLAGS if f != "-shared"] + extra
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="indexsortprobe_") as tmp:
        jobs = [(s, os.path.join(tmp, os.path.basename(s) + ".o")) for s in WRAPPERS + [SRC]]

        def one(job):
            src, obj = job
            cmd = [b.HIPCC, *cflags, "-I", b.CSRC, "-c", "-o", obj, src]
            return cmd, subprocess.run(cmd, cwd=b.CSRC, capture_output=True, text=True)

        with ThreadPoolExecutor(len(jobs)) as ex:
            results = list(ex.map(one, jobs))
        for cmd, res in results:
            if res.returncode != 0:
                raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{res.stderr[-8000:]}")
        cmd = [b.HIPCC, "--offload-arch=gfx950", "-shared", "-pthread", "-o", LIB + ".tmp", *[j[1] for j in jobs]]
        res = subprocess.run(cmd, cwd=b.CSRC, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"link failed:\n{' '.join(cmd)}\n{res.stderr[-8000:]}")
    os.replace(LIB + ".tmp", LIB)
    return LIB


_lib = None


def lib():
    """The probe library, built first when it is missing or older than its sources."""
    global _lib
    if _lib is None:
        build_probe()
        # torch's HIP runtime first, the order rna_clique_amd/_native.py keeps
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except Exception:
            pass
        L = ctypes.CDLL(LIB)
        P, u64, u32, i32, vp = ctypes.POINTER, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p
        L.isp_create.restype = vp
        L.isp_create.argtypes = []
        L.isp_destroy.restype = None
        L.isp_destroy.argtypes = [vp]
        L.isp_error.restype = ctypes.c_char_p
        L.isp_error.argtypes = [vp]
        L.isp_geometry.restype = None
        L.isp_geometry.argtypes = [P(i32), P(i32), P(i32), P(i32)]
        L.isp_choice.restype = None
        L.isp_choice.argtypes = [u64, u32, P(i32), P(i32)]
        L.isp_epoch.restype = u32
        L.isp_epoch.argtypes = [vp]
        L.isp_sort.restype = i32
        L.isp_sort.argtypes = [vp, vp, u64, i32, i32, u32, vp, vp, vp]
        L.isp_index.restype = i32
        L.isp_index.argtypes = [vp, vp, u64, vp, vp, u32, i32, u32, vp, u64, P(u64), vp, i32, P(i32), P(i32), vp]
        _lib = L
    return _lib


def geometry():
    """(keys per global-pass tile, range-local capacity, oversized-list length,
    most global bits) of the compiled kernels (host only: no GPU needed)."""
    v = [ctypes.c_int() for _ in range(4)]
    lib().isp_geometry(*[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v)


def choice(n, cap=0):
    """(bucket bits, G) the engine picks for an index of n entries (host only)."""
    bits, G = ctypes.c_int(), ctypes.c_int()
    lib().isp_choice(n, cap, ctypes.byref(bits), ctypes.byref(G))
    return bits.value, G.value


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


class Probe:
    """One probe handle: a stream plus the sort's scratch, status table and
    epoch, all kept from call to call."""

    def __init__(self):
        self._L = lib()
        self._h = self._L.isp_create()
        if not self._h:
            raise RuntimeError("isp_create: " + self._L.isp_error(None).decode())

    def close(self):
        if self._h:
            self._L.isp_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {rc}: {self._L.isp_error(self._h).decode()}")

    def sort(self, keys, G, bits, cap=0):
        """(entries, bucket, info) of os_index_sort; info = dict(ranges, keys,
        whole): what took the oversized-range fallbacks."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        ent = np.full(keys.shape[0], 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        bucket = np.full((1 << bits) + 1, 0xDEADBEEF, dtype=np.uint32)
        info = np.zeros(3, dtype=np.uint64)
        self._chk(self._L.isp_sort(self._h, _ptr(keys), keys.shape[0], G, bits, cap, _ptr(ent), _ptr(bucket),
                                   _ptr(info)), "isp_sort")
        return ent, bucket, dict(ranges=int(info[0]), keys=int(info[1]), whole=bool(info[2]))

    def index(self, seq, tx_start, tx_len, amb, cap=0):
        """(entries, bucket, bits, G, info) of the index of the transcripts, built the engine's way."""
        seq = np.ascontiguousarray(np.frombuffer(bytes(seq), dtype=np.uint8) if isinstance(seq, (bytes, bytearray))
                                   else seq, dtype=np.uint8)
        tx_start = np.ascontiguousarray(tx_start, dtype=np.uint64)
        tx_len = np.ascontiguousarray(tx_len, dtype=np.uint32)
        room = int(np.maximum(tx_len.astype(np.int64) - (W16 - 1), 0).sum())
        bits_cap = choice(room)[0]
        ent = np.full(max(room, 1), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        bucket = np.full((1 << bits_cap) + 1, 0xDEADBEEF, dtype=np.uint32)
        info = np.zeros(3, dtype=np.uint64)
        n, bits, G = ctypes.c_uint64(0), ctypes.c_int(0), ctypes.c_int(0)
        self._chk(self._L.isp_index(self._h, _ptr(seq), seq.shape[0], _ptr(tx_start), _ptr(tx_len), tx_len.shape[0],
                                    int(amb), cap, _ptr(ent), room, ctypes.byref(n), _ptr(bucket), bits_cap,
                                    ctypes.byref(bits), ctypes.byref(G), _ptr(info)), "isp_index")
        return (ent[:n.value].copy(), bucket[:(1 << bits.value) + 1].copy(), bits.value, G.value,
                dict(ranges=int(info[0]), keys=int(info[1]), whole=bool(info[2])))


# ------------------------------------------------------------------------
# host references
# ------------------------------------------------------------------------

def ref_entries(keys):
    """keys sorted stably on the bits [32, 64)."""
    keys = np.asarray(keys, dtype=np.uint64)
    return keys[np.argsort(keys >> np.uint64(32), kind="stable")]


def ref_bucket(sorted_entries, bits):
    """bucket[x] = first entry whose top `bits` bits are >= x, x = 0 .. 2^bits."""
    top = np.asarray(sorted_entries, dtype=np.uint64) >> np.uint64(64 - bits)
    x = np.arange((1 << bits) + 1, dtype=np.uint64)
    return np.searchsorted(top, x, side="left").astype(np.uint32)


def assert_same(got, want, what=""):
    """Whole-array equality (np.array_equal), with the first difference in the message."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype == want.dtype and np.array_equal(got, want):
        return
    if got.dtype != want.dtype:
        raise AssertionError(f"{what}: dtype {got.dtype}, expected {want.dtype}")
    if got.shape != want.shape:
        raise AssertionError(f"{what}: shape {got.shape}, expected {want.shape}")
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    raise AssertionError(f"{what}: {bad.shape[0]} of {got.shape[0]} differ, first at {i}: "
                         f"got {int(got[i]):#x}, expected {int(want[i]):#x}")
