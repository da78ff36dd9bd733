"""Query and result files of the top-k search per row of the primal (csrc/host/topk.c).

A query file holds one `blk row lo hi [skip ...]` per line: block and row 1-based as in .dat-s, the window of candidate columns
lo..hi inclusive, then the columns to skip.  `lorads file.dat-s --topkFile IN --topkCount k [--topkOut OUT] [--topkSmallest]
[--topkDiag] [--topkSkipConstrained]` answers it with a file of the form

    lorads-topk 1
    count N
    k K
    src uv|rr
    order largest|smallest
    blk row found            (per query, in the query file's order)
    col value                (found lines)

every double printed with %.17g, so that reading it back gives the bits."""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

Topk = namedtuple("Topk", "count k src order blk row found idx val")

_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)


def write_queries(path, blk, row, lo, hi, skip=None):
    """blk, row, lo, hi: 1-based integer vectors (the window lo..hi inclusive); skip: a list of 1-based column lists or None"""
    blk, row, lo, hi = (np.asarray(a, dtype=np.int64) for a in (blk, row, lo, hi))
    with open(path, "w") as f:
        for e in range(len(blk)):
            extra = "" if skip is None else "".join(" %d" % c for c in skip[e])
            f.write("%d %d %d %d%s\n" % (blk[e], row[e], lo[e], hi[e], extra))


def read_topk(path):
    """the output file: Topk(count, k, src, order, blk, row, found, idx, val) with 1-based blk, row and idx; idx [count, k] holds 0
    and val 0.0 past found"""
    with open(path) as f:
        lines = [ln.split() for ln in f.read().splitlines() if ln.strip()]
    if lines[0] != ["lorads-topk", "1"]:
        raise ValueError("%s: not a lorads-topk 1 file" % path)
    head = {ln[0]: ln[1] for ln in lines[1:5]}
    count, k = int(head["count"]), int(head["k"])
    blk, row, found = (np.zeros(count, dtype=np.int64) for _ in range(3))
    idx, val = np.zeros((count, k), dtype=np.int64), np.zeros((count, k))
    at = 5
    for e in range(count):
        blk[e], row[e], found[e] = (int(x) for x in lines[at])
        if len(lines[at]) != 3 or not 0 <= found[e] <= k:
            raise ValueError("%s: query %d: bad header line" % (path, e + 1))
        for j in range(found[e]):
            idx[e, j], val[e, j] = int(lines[at + 1 + j][0]), float(lines[at + 1 + j][1])
        at += 1 + found[e]
    if at != len(lines):
        raise ValueError("%s: %d lines beyond the last query" % (path, len(lines) - at))
    return Topk(count, k, head["src"], head["order"], blk, row, found, idx, val)


# ---- the C host's reader and writer (what the command line uses), for callers that want the same files from Python
class TopkStruct(C.Structure):
    """lrd_topk (csrc/host/lorads_host.h)"""
    _fields_ = [("count", C.c_int), ("k", C.c_int), ("src", C.c_int), ("smallest", C.c_int), ("include_diag", C.c_int),
                ("skip_constrained", C.c_int), ("blk", _ip), ("row", _ip), ("lo", _ip), ("hi", _ip), ("skip_ptr", C.POINTER(C.c_int64)),
                ("skip_col", _ip), ("found", _ip), ("idx", _ip), ("val", _dp)]


def _lib():
    from lorads_amd import host
    lib = host.host_lib()
    lib.lrd_topk_read.argtypes = [C.c_char_p, C.POINTER(C.POINTER(TopkStruct)), _ip]
    lib.lrd_topk_write.argtypes = [C.c_char_p, C.POINTER(TopkStruct)]
    lib.lrd_topk_free.argtypes = [C.POINTER(TopkStruct)]
    lib.lrd_topk_free.restype = None
    return lib


def read_queries(path):
    """a query file through the C reader: (blk, row, lo, hi, skip), 1-based, the window lo..hi inclusive, skip a list of arrays;
    ValueError names the malformed line"""
    lib, ptr, bad = _lib(), C.POINTER(TopkStruct)(), C.c_int(0)
    rc = lib.lrd_topk_read(os.fsencode(str(path)), C.byref(ptr), C.byref(bad))
    if rc == 1:
        raise OSError("cannot read %s" % path)
    if rc:
        raise ValueError("%s: line %d is malformed" % (path, bad.value))
    try:
        q, n = ptr.contents, ptr.contents.count
        get = lambda p, off: np.array([p[e] for e in range(n)], dtype=np.int64) + off  # noqa: E731
        skip = [np.array([q.skip_col[x] + 1 for x in range(q.skip_ptr[e], q.skip_ptr[e + 1])], dtype=np.int64) for e in range(n)]
        return get(q.blk, 1), get(q.row, 1), get(q.lo, 1), get(q.hi, 0), skip
    finally:
        lib.lrd_topk_free(ptr)


def write_topk(path, blk, row, found, idx, val, k, src="uv", smallest=False):
    """the output file through the C writer; blk, row and idx 1-based, idx and val [count, k]"""
    blk, row = (np.ascontiguousarray(np.asarray(a) - 1, dtype=np.int32) for a in (blk, row))
    found = np.ascontiguousarray(found, dtype=np.int32)
    idx = np.ascontiguousarray(np.asarray(idx).reshape(len(blk), k) - 1, dtype=np.int32)
    val = np.ascontiguousarray(np.asarray(val).reshape(len(blk), k), dtype=np.float64)
    q = TopkStruct(len(blk), int(k), 1 if src == "uv" else 0, int(bool(smallest)), 0, 0, blk.ctypes.data_as(_ip), row.ctypes.data_as(_ip),
                   None, None, None, None, found.ctypes.data_as(_ip), idx.ctypes.data_as(_ip), val.ctypes.data_as(_dp))
    if _lib().lrd_topk_write(os.fsencode(str(path)), C.byref(q)):
        raise OSError("cannot write %s" % path)
