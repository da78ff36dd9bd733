"""Query and result files of the primal's entries (csrc/host/primal.c).

A query file holds one `k i j` or `k i j v` per line: block, row and column 1-based as in .dat-s, v a reference value (every line
carries one or none does).  `lorads file.dat-s --entriesFile IN --entriesOut OUT` answers it with a file of the form

    lorads-entries 1
    count N
    src uv|rr
    refs 0|1
    rmse .. / mae .. / maxabs .. / refnorm ..     (with refs)
    k i j x [v]                                   (per query, in the query file's order)

every double printed with %.17g, so that reading it back gives the bits."""
from collections import namedtuple

import numpy as np

Entries = namedtuple("Entries", "count src refs stats blk row col val ref")


def write_queries(path, blk, row, col, ref=None):
    """blk, row, col: 1-based integer vectors; ref: a value per query or None"""
    blk, row, col = (np.asarray(a, dtype=np.int64) for a in (blk, row, col))
    with open(path, "w") as f:
        for e in range(len(blk)):
            if ref is None:
                f.write("%d %d %d\n" % (blk[e], row[e], col[e]))
            else:
                f.write("%d %d %d %.17g\n" % (blk[e], row[e], col[e], float(ref[e])))


def read_entries(path):
    """the output file: Entries(count, src, refs, stats, blk, row, col, val, ref) with 1-based indices; stats is a dict of rmse, mae,
    maxabs and refnorm with refs, else None"""
    with open(path) as f:
        lines = [ln.split() for ln in f.read().splitlines() if ln.strip()]
    if lines[0] != ["lorads-entries", "1"]:
        raise ValueError("%s: not a lorads-entries 1 file" % path)
    head = {}
    at = 1
    while at < len(lines) and not lines[at][0].lstrip("-").isdigit():
        head[lines[at][0]] = lines[at][1]
        at += 1
    count, refs = int(head["count"]), int(head["refs"]) == 1
    body = lines[at:]
    if len(body) != count or any(len(b) != (5 if refs else 4) for b in body):
        raise ValueError("%s: %d entry lines for count %d" % (path, len(body), count))
    blk = np.array([int(b[0]) for b in body], dtype=np.int64)
    row = np.array([int(b[1]) for b in body], dtype=np.int64)
    col = np.array([int(b[2]) for b in body], dtype=np.int64)
    val = np.array([float(b[3]) for b in body], dtype=np.float64)
    ref = np.array([float(b[4]) for b in body], dtype=np.float64) if refs else None
    stats = {k: float(head[k]) for k in ("rmse", "mae", "maxabs", "refnorm")} if refs else None
    return Entries(count, head["src"], refs, stats, blk, row, col, val, ref)


# ---- the C host's reader, grouping and writer (what the command line uses), for callers that want the same files from Python
import ctypes as C  # noqa: E402

_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)


class EntriesStruct(C.Structure):
    """lrd_entries (csrc/host/lorads_host.h)"""
    _fields_ = [("count", C.c_int64), ("has_ref", C.c_int), ("src", C.c_int), ("blk", _ip), ("row", _ip), ("col", _ip),
                ("ref", _dp), ("val", _dp), ("stats", C.c_double * 4)]


def _lib():
    from lorads_amd import host
    lib = host.host_lib()
    lib.lrd_entries_read.argtypes = [C.c_char_p, C.POINTER(C.POINTER(EntriesStruct)), _ip]
    lib.lrd_entries_write.argtypes = [C.c_char_p, C.POINTER(EntriesStruct)]
    lib.lrd_entries_free.argtypes = [C.POINTER(EntriesStruct)]
    lib.lrd_entries_group.argtypes = [C.POINTER(EntriesStruct), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    return lib


def read_queries(path):
    """a query file through the C reader: (blk, row, col, ref-or-None), 1-based; ValueError names the malformed line"""
    import os
    lib, ptr, bad = _lib(), C.POINTER(EntriesStruct)(), C.c_int(0)
    rc = lib.lrd_entries_read(os.fsencode(str(path)), C.byref(ptr), C.byref(bad))
    if rc == 1:
        raise OSError("cannot read %s" % path)
    if rc:
        raise ValueError("%s: line %d is malformed" % (path, bad.value))
    try:
        q, n = ptr.contents, ptr.contents.count
        get = lambda p, t: np.array([p[e] for e in range(n)], dtype=t)  # noqa: E731
        return get(q.blk, np.int64) + 1, get(q.row, np.int64) + 1, get(q.col, np.int64) + 1, (get(q.ref, np.float64) if q.has_ref else None)
    finally:
        lib.lrd_entries_free(ptr)


def _struct(blk, row, col, val=None, ref=None, src=1, stats=None):
    blk, row, col = (np.ascontiguousarray(np.asarray(a) - 1, dtype=np.int32) for a in (blk, row, col))
    val = np.ascontiguousarray(val if val is not None else np.zeros(len(blk)), dtype=np.float64)
    ref = None if ref is None else np.ascontiguousarray(ref, dtype=np.float64)
    q = EntriesStruct(len(blk), int(ref is not None), int(src), blk.ctypes.data_as(_ip), row.ctypes.data_as(_ip), col.ctypes.data_as(_ip),
                      ref.ctypes.data_as(_dp) if ref is not None else None, val.ctypes.data_as(_dp),
                      (C.c_double * 4)(*(stats if stats is not None else (0.0, 0.0, 0.0, 0.0))))
    return q, (blk, row, col, val, ref)   # (the arrays live as long as the caller holds them)


def write_entries(path, blk, row, col, val, ref=None, src="uv", stats=None):
    """the output file through the C writer; indices 1-based, stats the four sums {sum d^2, sum |d|, max |d|, sum ref^2}"""
    import os
    q, keep = _struct(blk, row, col, val, ref, 1 if src == "uv" else 0, stats)
    if _lib().lrd_entries_write(os.fsencode(str(path)), C.byref(q)):
        raise OSError("cannot write %s" % path)
    del keep


def group_queries(blk, nblk):
    """the C host's per-block grouping of queries with 1-based blocks blk: (perm, start) -- perm[start[k]:start[k + 1]] are the indices
    of block k's queries in file order"""
    q, keep = _struct(blk, np.ones(len(blk)), np.ones(len(blk)))
    perm = np.zeros(max(len(blk), 1), dtype=np.int64)
    start = np.zeros(nblk + 1, dtype=np.int64)
    if _lib().lrd_entries_group(C.byref(q), nblk, perm.ctypes.data_as(C.POINTER(C.c_int64)), start.ctypes.data_as(C.POINTER(C.c_int64))):
        raise ValueError("a query names a block outside 1..%d" % nblk)
    del keep
    return perm[:len(blk)], start
