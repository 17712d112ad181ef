"""The seed index kernels called one by one, and what each must return.

TEST INFRASTRUCTURE ONLY. oracle/index_probe.hip is compiled together with the
product's own sort.hip and kernels.hip (the compiler and flags of
rna_clique_amd/build.py, so the kernels under test are the product's) into
oracle/_build/libindexprobe.so. The two product sources are compiled through
index_probe_sort.hip and index_probe_kernels.hip, which include them unchanged
and add the host accessors of their geometry: the product sources stay
untouched. The library is never linked into librcgpu.so and never imported by
rna_clique_amd.

The host references below restate the contract from the kernels' comments in
integer-exact numpy; none of them calls the kernels:

  sort     stable sort of u64 keys on the bits [bb, 64)
  entries  (k-mer << 32 | position) of every 16-base window, sorted
  bucket   bucket[x] = first sorted entry whose top `bits` bits are >= x
  pack     2-bit forward / reverse-complement words and their ambiguity masks
"""
from __future__ import annotations

import ctypes
import os
import subprocess

try:
    import numpy as np
except ImportError:   # `make -C oracle` runs build_probe() under whatever python3 is: the build needs no numpy
    np = None

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "index_probe.hip")
LIB = os.path.join(HERE, "_build", "libindexprobe.so")
PRODUCT_SOURCES = ["sort.hip", "kernels.hip"]
# each product source through a unit that includes it and adds geometry accessors
WRAPPERS = [os.path.join(HERE, "index_probe_sort.hip"), os.path.join(HERE, "index_probe_kernels.hip")]
SYMBOLS = ["ip_create", "ip_destroy", "ip_error", "ip_geometry", "ip_pack_words", "ip_epoch", "ip_sort",
           "ip_bucket", "ip_pack", "ip_index"]
W16 = 16   # index word, bases


# ------------------------------------------------------------------------
# build
# ------------------------------------------------------------------------

def _product():
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from rna_clique_amd import build
    return build


def _deps():
    csrc = _product().CSRC
    return [SRC] + WRAPPERS + [os.path.join(csrc, s) for s in PRODUCT_SOURCES + ["device.h", "launch.h"]]


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in _deps())


def build_probe(force=False):
    """Compile the probe and the product's sort.hip and kernels.hip (one object
    each, the product's compiler, flags and working directory; the product
    sources are included by the wrapper units) and link them into LIB."""
    if not force and not _stale():
        return LIB
    from concurrent.futures import ThreadPoolExecutor
    import tempfile
    b = _product()
    extra = os.environ.get("RC_EXTRA_FLAGS", "").split()
    cflags = [f for f in b.FLAGS if f != "-shared"] + extra
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="indexprobe_") as tmp:
        jobs = [(s, os.path.join(tmp, os.path.basename(s) + ".o"), ["-I", b.CSRC]) for s in WRAPPERS + [SRC]]

        def one(job):
            src, obj, inc = job
            cmd = [b.HIPCC, *cflags, *inc, "-c", "-o", obj, src]
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


# ------------------------------------------------------------------------
# ctypes front end
# ------------------------------------------------------------------------

_lib = None


def lib():
    """The probe library, built first when it is missing or older than its sources."""
    global _lib
    if _lib is None:
        build_probe()
        # torch bundles its own HIP runtime, and tests that use it share the
        # process: bring torch's up before this library's is loaded, the order
        # rna_clique_amd/_native.py keeps (the other order found no device)
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except Exception:
            pass
        L = ctypes.CDLL(LIB)
        P, u64, u32, i32, vp = ctypes.POINTER, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p
        L.ip_create.restype = vp
        L.ip_create.argtypes = []
        L.ip_destroy.restype = None
        L.ip_destroy.argtypes = [vp]
        L.ip_error.restype = ctypes.c_char_p
        L.ip_error.argtypes = [vp]
        L.ip_geometry.restype = None
        L.ip_geometry.argtypes = [P(i32), P(i32), P(i32)]
        L.ip_pack_words.restype = u64
        L.ip_pack_words.argtypes = [u64]
        L.ip_epoch.restype = u32
        L.ip_epoch.argtypes = [vp]
        L.ip_sort.restype = i32
        L.ip_sort.argtypes = [vp, vp, u64, i32, vp]
        L.ip_bucket.restype = i32
        L.ip_bucket.argtypes = [vp, vp, u64, i32, vp]
        L.ip_pack.restype = i32
        L.ip_pack.argtypes = [vp, vp, u64, vp, vp, vp, vp]
        L.ip_index.restype = i32
        L.ip_index.argtypes = [vp, vp, u64, vp, vp, u32, i32, vp, u64, P(u64)]
        _lib = L
    return _lib


def geometry():
    """(OS_TILE, OS_SEG, BF_PER) of the compiled kernels (host only: no GPU needed)."""
    t, s, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib().ip_geometry(ctypes.byref(t), ctypes.byref(s), ctypes.byref(b))
    return t.value, s.value, b.value


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _bytes(seq):
    if isinstance(seq, (bytes, bytearray)):
        seq = np.frombuffer(bytes(seq), dtype=np.uint8)
    return np.ascontiguousarray(seq, dtype=np.uint8)


class Probe:
    """One probe handle: a stream plus the sort's scratch, status table and
    epoch, all kept from call to call."""

    def __init__(self):
        self._L = lib()
        self._h = self._L.ip_create()
        if not self._h:
            raise RuntimeError("ip_create: " + self._L.ip_error(None).decode())

    def close(self):
        if self._h:
            self._L.ip_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {rc}: {self._L.ip_error(self._h).decode()}")

    @property
    def epoch(self):
        return self._L.ip_epoch(self._h)

    def sort(self, keys, bb):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.full(keys.shape[0], 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        self._chk(self._L.ip_sort(self._h, _ptr(keys), keys.shape[0], bb, _ptr(out)), "ip_sort")
        return out

    def bucket(self, sorted_entries, bits):
        ent = np.ascontiguousarray(sorted_entries, dtype=np.uint64)
        out = np.full((1 << bits) + 1, 0xDEADBEEF, dtype=np.uint32)
        self._chk(self._L.ip_bucket(self._h, _ptr(ent), ent.shape[0], bits, _ptr(out)), "ip_bucket")
        return out

    def pack(self, seq):
        seq = _bytes(seq)
        nw = self._L.ip_pack_words(seq.shape[0])
        out = [np.full(nw, 0xDEADBEEFDEADBEEF, dtype=np.uint64) for _ in range(4)]
        self._chk(self._L.ip_pack(self._h, _ptr(seq), seq.shape[0], *[_ptr(o) for o in out]), "ip_pack")
        return tuple(out)   # F, AF, RC, ARC

    def index(self, seq, tx_start, tx_len, path):
        seq = _bytes(seq)
        tx_start = np.ascontiguousarray(tx_start, dtype=np.uint64)
        tx_len = np.ascontiguousarray(tx_len, dtype=np.uint32)
        cap = int(np.maximum(tx_len.astype(np.int64) - (W16 - 1), 0).sum())
        out = np.full(max(cap, 1), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        n = ctypes.c_uint64(0)
        self._chk(self._L.ip_index(self._h, _ptr(seq), seq.shape[0], _ptr(tx_start), _ptr(tx_len), tx_len.shape[0],
                                   path, _ptr(out), cap, ctypes.byref(n)), "ip_index")
        return out[:n.value].copy()


# ------------------------------------------------------------------------
# host references
# ------------------------------------------------------------------------

# A C G T in either case -> 0..3; every other byte is ambiguous (4)
def _code_lut():
    lut = np.full(256, 4, dtype=np.uint8)
    for i, c in enumerate(b"ACGT"):
        lut[c] = lut[c | 0x20] = i
    return lut


CODE = _code_lut() if np is not None else None


def ref_sort(keys, bb):
    """keys sorted stably on the bits [bb, 64)."""
    keys = np.asarray(keys, dtype=np.uint64)
    if bb == 0:
        return np.sort(keys)   # all 64 bits: equal keys are indistinguishable
    return keys[np.argsort(keys >> np.uint64(bb), kind="stable")]


def ref_entries(seq, tx_start, tx_len, amb=False):
    """The sorted index of the transcripts: for every transcript in order and
    every offset o with o + 16 <= len the entry (key << 32 | start + o), key =
    sum of code(seq[start + o + i]) << 2i over i < 16. amb: windows holding a
    byte outside ACGTacgt are left out (the paths without ambiguity handling
    are only defined on ACGT input). Fill order is position order and the sort
    is stable, so the result is np.sort of all entries."""
    seq = _bytes(seq)
    code = CODE[seq]
    bad = code > 3
    if bad.any() and not amb:
        raise ValueError("ambiguous bytes need amb=True")
    code = np.where(bad, 0, code).astype(np.uint64)
    # key of the window at every position, and whether it holds an ambiguous byte
    nwin = max(seq.shape[0] - W16 + 1, 0)
    key = np.zeros(nwin, dtype=np.uint64)
    anyb = np.zeros(nwin, dtype=bool)
    for i in range(W16):
        key |= code[i:i + nwin] << np.uint64(2 * i)
        anyb |= bad[i:i + nwin]
    parts = []
    for s, ln in zip(np.asarray(tx_start, dtype=np.int64), np.asarray(tx_len, dtype=np.int64)):
        if ln < W16:
            continue
        pos = np.arange(s, s + ln - W16 + 1, dtype=np.int64)
        if amb:
            pos = pos[~anyb[pos]]
        parts.append((key[pos] << np.uint64(32)) | pos.astype(np.uint64))
    if not parts:
        return np.zeros(0, dtype=np.uint64)
    return np.sort(np.concatenate(parts))


def ref_bucket(sorted_entries, bits):
    """bucket[x] = first entry whose top `bits` bits are >= x, x = 0 .. 2^bits."""
    top = np.asarray(sorted_entries, dtype=np.uint64) >> np.uint64(64 - bits)
    x = np.arange((1 << bits) + 1, dtype=np.uint64)
    return np.searchsorted(top, x, side="left").astype(np.uint32)


def _to_words(codes, nwords):
    """2-bit codes (one per base, base i of a word at bits 2i..2i+1) -> u64 words."""
    c = np.zeros(nwords * 32, dtype=np.uint64)
    c[:codes.shape[0]] = codes
    sh = (np.arange(32, dtype=np.uint64) * np.uint64(2))[None, :]
    return np.bitwise_or.reduce(c.reshape(nwords, 32) << sh, axis=1)


def pack_words(total):
    """Words per packed array: the bases plus the engine's two spare words."""
    return (total + 31) // 32 + 2


def ref_pack(seq):
    """(F, AF, RC, ARC) of seq, pack_words(len) words each.
    F: base i of a word at bits 2i..2i+1; an ambiguous base codes as 0.
    AF: 3 at ambiguous bases, 0 elsewhere. Bits past the end are 0 in both.
    RC: base q is the complement (3 - code) of forward base total - 1 - q, so
    word w is the reverse complement of the forward window ending at
    total - 32 w; past the end it complements nothing: all ones.
    ARC: AF in the same reversed order, 0 past the end."""
    seq = _bytes(seq)
    total = seq.shape[0]
    nw = pack_words(total)
    code = CODE[seq]
    bad = code > 3
    f = np.where(bad, 0, code).astype(np.uint64)
    a = np.where(bad, 3, 0).astype(np.uint64)
    rc = np.full(nw * 32, 3, dtype=np.uint64)
    rc[:total] = np.uint64(3) - f[::-1]
    return _to_words(f, nw), _to_words(a, nw), _to_words(rc, nw), _to_words(a[::-1], nw)


# ------------------------------------------------------------------------
# the comparison of the GPU tests
# ------------------------------------------------------------------------

def assert_same(got, want, what=""):
    """Whole-array equality (np.array_equal), with the first difference in the
    message. Not a sortedness or checksum property: one wrong element fails."""
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
