"""The numpy model of the top-k search per row of the primal (tests/topk_model.py) against a brute-force sorted(); the query and result
files through the C reader and writer; the table slot and what the command line refuses before it creates a backend.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from lorads_amd import host, topk
from tests import common
from tests import topk_model as tm


def _brute(F, p, lo, hi, k, smallest, include_diag, skip):
    """sorted() over python floats (the cases are exact in float64)"""
    cand = []
    for q in range(lo, hi):
        x = math.fsum(float(a) * float(b) for a, b in zip(F[p], F[q]))
        if x != x or (q == p and not include_diag) or q in skip:
            continue
        cand.append((x if smallest else -x, q))   # (-0.0 == 0.0 in a tuple comparison: the column decides)
    cand.sort()
    return [q for _, q in cand[:k]], [(x if smallest else -x) + 0.0 for x, _ in cand[:k]]


CASES = {
    "ints": np.array([[1, 2], [2, 1], [-1, 0], [0, 0], [3, -3], [1, 2], [-2, -1], [0, 1]], dtype=np.float64),
    "ties": np.ones((7, 3)),
    "zeros": np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [-0.0, 0.0, -0.0]]),
    "one": np.array([[2.0]]),
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("smallest", [False, True])
def test_model_against_brute_force(name, smallest):
    F = CASES[name]
    n = len(F)
    rows = list(range(n)) + [0]
    for lo, hi in {(0, n), (n // 3, max(n - 1, n // 3)), (0, 0), (n - 1, n)}:
        for k in (1, 3, 128):
            for diag in (False, True):
                for skip in (None, [[p, (p + 1) % n, (p + 1) % n, n - 1] for p in rows]):
                    idx, val, found = tm.model_topk(F, rows, lo, hi, k, smallest, diag, skip)
                    for i, p in enumerate(rows):
                        bq, bx = _brute(F, p, lo, hi, k, smallest, diag, set(skip[i]) if skip else set())
                        assert found[i] == len(bq)
                        assert idx[i, :found[i]].tolist() == bq, (name, lo, hi, k, diag, p)
                        assert val[i, :found[i]].tolist() == bx
                        assert (idx[i, found[i]:] == -1).all() and (val[i, found[i]:] == 0).all()
                    tm.check_against_model(F, rows, lo, hi, k, smallest, diag, skip, idx, val, found, name)


def test_zero_of_either_sign_ties_by_column():
    F = CASES["zeros"]
    for smallest in (False, True):
        idx, val, found = tm.model_topk(F, [6], 0, 8, 8, smallest)
        assert idx[0].tolist() == [0, 1, 2, 3, 4, 5, 7, -1] and found[0] == 7 and not np.signbit(val).any()
    idx, _, _ = tm.model_topk(F, [0], 0, 8, 3)
    assert idx[0].tolist() == [2, 3, 4]          # (X_00 is no candidate; the zeros of either sign by column; -1 last)
    idx, _, _ = tm.model_topk(F, [0], 0, 8, 3, smallest=True)
    assert idx[0].tolist() == [1, 2, 3]


def test_check_rejects_wrong_lists():
    rng = np.random.default_rng(0)
    F = rng.standard_normal((20, 3))
    rows = [3, 4]
    idx, val, found = tm.model_topk(F, rows, 0, 20, 5)
    tm.check_against_model(F, rows, 0, 20, 5, False, False, None, idx, val, found)
    for spoil in ("swap", "value", "found", "diag"):
        i2, v2, f2 = idx.copy(), val.copy(), found.copy()
        if spoil == "swap":
            i2[0, [0, 1]] = i2[0, [1, 0]]
            v2[0, [0, 1]] = v2[0, [1, 0]]
        elif spoil == "value":
            v2[1, 2] *= 1 + 1e-12
        elif spoil == "found":
            f2[0] = 4
        else:
            i2[0, 4] = 3
        with pytest.raises(AssertionError):
            tm.check_against_model(F, rows, 0, 20, 5, False, False, None, i2, v2, f2)


def test_files_round_trip_through_the_c_reader_and_writer(tmp_path):
    qf, of = tmp_path / "q.txt", tmp_path / "o.txt"
    blk, row, lo, hi = [1, 2, 1], [3, 1, 60], [1, 5, 31], [60, 5, 60]
    skip = [[4, 4, 9], [], [2147483647]]
    topk.write_queries(qf, blk, row, lo, hi, skip)
    with open(qf, "a") as f:
        f.write("\n* a comment\n  # another\n1 7 2 3 5   \n")
    b, r, l, h, s = topk.read_queries(qf)
    assert b.tolist() == blk + [1] and r.tolist() == row + [7] and l.tolist() == lo + [2] and h.tolist() == hi + [3]
    assert [x.tolist() for x in s] == skip + [[5]]
    k = 3
    found = [3, 0, 1]
    idx = np.array([[5, 2, 9], [0, 0, 0], [31, 0, 0]])
    val = np.array([[1 / 3, -0.0, -1e-300], [0, 0, 0], [np.inf, 0, 0]])
    for smallest, src in ((False, "uv"), (True, "rr")):
        topk.write_topk(of, blk, row, found, idx, val, k, src=src, smallest=smallest)
        got = topk.read_topk(of)
        assert (got.count, got.k, got.src, got.order) == (3, k, src, "smallest" if smallest else "largest")
        assert got.blk.tolist() == blk and got.row.tolist() == row and got.found.tolist() == found
        assert np.array_equal(got.idx, idx)
        assert got.val.tobytes() == val.tobytes()   # (%.17g: the bits, the sign of zero included)
    text = of.read_text().splitlines()
    assert text[:5] == ["lorads-topk 1", "count 3", "k 3", "src rr", "order smallest"]
    assert text[5] == "1 3 3" and text[6] == "5 %.17g" % (1 / 3) and text[9] == "2 1 0" and text[10] == "1 60 1"


@pytest.mark.parametrize("line", ["1 2 3", "1 2", "0 1 1 5", "1 0 1 5", "1 1 0 5", "1 1 6 5", "1 1 1 5 x", "1 1 1 5 0", "1 1 1 5 -3",
                                  "1 1 1 5 2.5", "a", "1 1 1 99999999999", "1,1,1,5"])
def test_malformed_lines_are_named(tmp_path, line):
    qf = tmp_path / "q.txt"
    qf.write_text("1 1 1 5\n\n%s\n1 1 1 5\n" % line)
    with pytest.raises(ValueError, match="line 3"):
        topk.read_queries(qf)
    with pytest.raises(OSError):
        topk.read_queries(tmp_path / "none.txt")


def test_oracle_backend_refuses_and_table_mirror():
    s = common.oracle_session(common.instance_path("theta30"))
    try:
        assert not s.be.has_primal_topk()
        with pytest.raises(NotImplementedError):
            s.primal_topk(0, [0], 5)
    finally:
        s.close()
    names = [f[0] for f in host.BackendStruct._fields_]
    assert names.index("primal_apply") + 1 == names.index("primal_topk") == names.index("triangle_cuts") - 1
    assert names[-2:] == ["spectrum", "compress_rank"]
    lib = host.host_lib()
    lib.lrd_backend_sizeof.restype = C.c_size_t
    assert lib.lrd_backend_sizeof() == C.sizeof(host.BackendStruct)
    assert C.sizeof(topk.TopkStruct) == 96
    hip = C.CDLL(os.path.join(host.LIB_DIR, "liblorads_hip.so"))
    assert hasattr(hip, "lorads_hip_primal_topk")


@pytest.mark.parametrize("args,say", [
    (["--topkCount", "5"], "--topkCount needs --topkFile"), (["--topkSmallest"], "--topkSmallest needs --topkFile"),
    (["--topkDiag"], "needs --topkFile"), (["--topkSkipConstrained"], "needs --topkFile"), (["--topkOut", "x"], "--topkOut needs --topkFile"),
    (["--topkFile", "Q", "--topkCount", "0"], "bad value 0 of --topkCount"), (["--topkFile", "Q", "--topkCount", "129"], "bad value"),
    (["--topkFile", "Q", "--topkCount", "-1"], "bad value"), (["--topkFile", "Q", "--topkCount", "3x"], "bad value"),
    (["--topkFile", "Q"], "--topkFile needs --topkCount"), (["--topkFile", "NONE", "--topkCount", "3"], "cannot read"),
    (["--topkFile", "BAD", "--topkCount", "3"], "line 2"), (["--topkFile", "OUT", "--topkCount", "3"], "query 2"),
    (["--topkFile", "LP", "--topkCount", "3"], "query 1"),
])
def test_command_line_refuses_before_the_backend(tmp_path, args, say):
    """bad values, --topk* without --topkFile, unreadable, malformed and out-of-problem query files: exit code 2 and nothing solved
    (sdplp40: cone 1 of 40 rows, block 2 the LP block)"""
    files = {"Q": "1 1 1 40\n", "BAD": "1 1 1 40\n1 1 5 4\n", "OUT": "1 1 1 40\n1 41 1 40\n", "LP": "2 1 1 1\n"}
    for name, text in files.items():
        (tmp_path / name).write_text(text)
    args = [str(tmp_path / a) if a in files or a == "NONE" else a for a in args]
    exe = os.path.join(host.LIB_DIR, "lorads")
    pr = subprocess.run([exe, common.instance_path("sdplp40")] + args, capture_output=True, text=True, timeout=120)
    assert pr.returncode == 2, (pr.returncode, pr.stderr)
    assert say in pr.stderr, pr.stderr
    assert "End Program" not in pr.stdout
