"""The solution file written by the C writer (lrd_solution_write) reads back bit for bit (no GPU)."""
import ctypes as C

import numpy as np
import pytest

from lorads_amd import host
from lorads_amd.solution import CERT_KEYS, SolutionConeStruct, SolutionStruct, read_solution


def _ptr(a, ct=C.c_double):
    return a.ctypes.data_as(C.POINTER(ct))


def _write(path, m, cones, seed=0):
    """cones: list of (n, rank) for SDP cones, (n, None) for the LP block; returns (y, [R or x], head)"""
    rng = np.random.default_rng(seed)
    keep = []
    y = rng.standard_normal(m) * 10.0 ** rng.integers(-300, 300, size=m) if m else np.zeros(1)
    keep.append(y)
    arr = (SolutionConeStruct * max(len(cones), 1))()
    want = []
    for k, (n, r) in enumerate(cones):
        q = arr[k]
        q.n, q.is_lp = n, int(r is None)
        if r is None:
            q.rank = 1
            x = rng.random(n) ** 3
            keep.append(x)
            q.x = _ptr(x)
            want.append(x)
        else:
            q.rank = r
            R = rng.standard_normal((n, r)) / 3.0
            cm = np.ascontiguousarray(R.T).ravel()  # column-major n x r
            keep.append(cm)
            q.R = _ptr(cm)
            want.append(R)
    st = SolutionStruct()
    st.m, st.nblk, st.status = m, len(cones), 2
    st.pobj, st.dobj = -123.45678901234567, 1e-310
    head = dict(zip(CERT_KEYS, [1.0 / 3.0, 2.5e-17, 0.0, 0.0, float("nan"), -7.0e-9, 0.1]))
    for k, v in head.items():
        setattr(st, k, v)
    st.y = _ptr(y)
    st.cone = arr
    lib = host.host_lib()
    lib.lrd_solution_write.argtypes = [C.c_char_p, C.POINTER(SolutionStruct)]
    assert lib.lrd_solution_write(str(path).encode(), C.byref(st)) == 0
    return y[:m], want, head, st


@pytest.mark.parametrize("m,cones", [
    (7, [(5, 3)]),                    # odd rank
    (4, [(6, 2), (3, 1), (9, None)]),  # several cones and the LP block
    (0, [(4, 2)]),                    # m = 0
])
def test_roundtrip_bit_equal(tmp_path, m, cones):
    path = tmp_path / "sol.txt"
    y, want, head, st = _write(path, m, cones, seed=m)
    sol = read_solution(path)
    assert sol.status == 2
    assert sol.pobj == st.pobj and sol.dobj == st.dobj
    for k, v in head.items():
        got = sol.certificate[k]
        assert (np.isnan(v) and np.isnan(got)) or got == v, k
    assert sol.y.shape == (m,)
    assert np.array_equal(sol.y.view(np.uint64), y.view(np.uint64))
    assert len(sol.cones) == len(cones)
    for (n, r), c, w in zip(cones, sol.cones, want):
        if r is None:
            assert c.is_lp and c.x.shape == (n,) and np.array_equal(c.x, w)
        else:
            assert not c.is_lp and c.R.shape == (n, r) and np.array_equal(c.R, w)


def test_layout(tmp_path):
    path = tmp_path / "sol.txt"
    _write(path, 2, [(3, 3), (2, None)])
    lines = path.read_text().split("\n")
    assert lines[0] == "lorads-solution 1"
    assert [ln.split()[0] for ln in lines[1:11]] == ["status", "pobj", "dobj"] + list(CERT_KEYS)
    assert lines[11] == "y 2"
    assert lines[14] == "sdp 1 3 3" and all(len(lines[15 + i].split()) == 3 for i in range(3))
    assert lines[18] == "lp 2 2" and len(lines[19].split()) == 1 and len(lines[20].split()) == 1
    assert lines[21] == "" and len(lines) == 22


def test_oracle_backend_refuses():
    from tests import common
    s = common.oracle_session(common.instance_path("maxcut100"))
    try:
        with pytest.raises(NotImplementedError):
            s.solution()
    finally:
        s.close()
