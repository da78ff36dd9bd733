"""What the results of the four roundings (rounding.py, kcut.py, stable.py, bisection.py) share: the ctypes mirror of the head of
their C structs, the scalar keys of their files, and the reader and the filler of those scalars."""
import ctypes as C

import numpy as np

INT_KEYS = ("trials", "seed", "max_rounds", "rounds", "src", "best", "best0")
FLOAT_KEYS = ("scale", "f_best", "f_best0", "by", "bound", "gap", "tol")
# the integer keys a feature's file adds to the head's, by the name of the member of the feature's own struct that holds them
OWN = {"parts": "parts", "lp_columns": "nlp", "lp_negative": "lp_neg"}


class RoundHeadStruct(C.Structure):
    """lrd_round_head (csrc/host/lorads_host.h): the first member, `head`, of lrd_rounding, lrd_kcut, lrd_stable and lrd_bisection"""
    _fields_ = [("trials", C.c_int), ("max_rounds", C.c_int), ("rounds", C.c_int), ("src", C.c_int), ("seed", C.c_uint64),
                ("scale", C.c_double), ("best", C.c_int), ("best0", C.c_int), ("f_best", C.c_double), ("f_best0", C.c_double),
                ("obj", C.POINTER(C.c_double)), ("obj0", C.POINTER(C.c_double)),
                ("by", C.c_double), ("bound", C.c_double), ("gap", C.c_double), ("tol", C.c_double)]


def _arr(ptr, n, dtype=np.float64):
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n > 0 and ptr else np.zeros(0, dtype=dtype)


def head_of(st, keys):
    """(obj, obj0, the scalars `keys` as a dict) of a result struct"""
    h = st.head
    sc = {k: getattr(st, OWN[k]) if k in OWN else getattr(h, k) for k in keys}
    return _arr(h.obj, h.trials), _arr(h.obj0, h.trials), sc


def fill_head(st, result, keys):
    """the scalars `keys` of a result object into its struct (what a file holds: the writers read nothing else of the head)"""
    for k in keys:
        setattr(st if k in OWN else st.head, OWN.get(k, k), getattr(result, k))


def read_head(path, magic, what, int_keys):
    """the lines of a result file, the position behind its scalars, and the scalars (int_keys, then FLOAT_KEYS, one per line)"""
    with open(path) as f:
        lines = f.read().split("\n")
    if lines[0] != magic:
        raise ValueError("%s: not a lorads %s file" % (path, what))
    pos = 1
    sc = {}
    for key in int_keys + FLOAT_KEYS:
        t = lines[pos].split()
        pos += 1
        if len(t) != 2 or t[0] != key:
            raise ValueError("%s: expected %s, found %r" % (path, key, t))
        sc[key] = int(t[1]) if key in int_keys else float(t[1])
    return lines, pos, sc
