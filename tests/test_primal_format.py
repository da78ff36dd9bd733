"""Query and result files of the primal's entries, the per-block grouping and the table's mirror (DESIGN.md section 13;
lorads_amd/csrc/host/primal.c, lorads_amd/primal.py): no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lorads_amd import host, primal
from tests import common


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _queries(n, seed):
    rng = np.random.default_rng(seed)
    blk = rng.integers(1, 4, n)
    row = rng.integers(1, 1000, n)
    col = rng.integers(1, 1000, n)
    # doubles whose shortest decimal form is long, a denormal, a negative zero, the largest double
    ref = rng.standard_normal(n) * 10.0 ** rng.integers(-300, 150, n)
    ref[:4] = [5e-324, -0.0, np.finfo(float).max, 1.0 / 3.0]
    return blk, row, col, ref


@pytest.mark.parametrize("with_ref", [False, True])
def test_query_and_output_files_round_trip_bit_exact(built, tmp_path, with_ref):
    blk, row, col, ref = _queries(257, 1)
    qf, of = tmp_path / "q.txt", tmp_path / "o.txt"
    primal.write_queries(qf, blk, row, col, ref if with_ref else None)
    b2, r2, c2, f2 = primal.read_queries(qf)
    assert np.array_equal(b2, blk) and np.array_equal(r2, row) and np.array_equal(c2, col)
    assert (f2 is None) == (not with_ref)
    if with_ref:
        assert np.array_equal(_bits(f2), _bits(ref))
    val = np.random.default_rng(2).standard_normal(257) * 1e-7
    with np.errstate(over="ignore"):   # (the largest double among the refs: two of the sums are inf, and inf round-trips too)
        d = val - ref
        stats = (float(np.sum(d * d)), float(np.sum(np.abs(d))), float(np.max(np.abs(d))), float(np.sum(ref * ref))) if with_ref else None
    primal.write_entries(of, b2, r2, c2, val, f2, "uv", stats)
    text = open(of).read().splitlines()
    assert text[:4] == ["lorads-entries 1", "count 257", "src uv", "refs %d" % with_ref]
    got = primal.read_entries(of)
    assert got.count == 257 and got.src == "uv" and got.refs == with_ref
    assert np.array_equal(got.blk, blk) and np.array_equal(got.row, row) and np.array_equal(got.col, col)
    assert np.array_equal(_bits(got.val), _bits(val))
    if with_ref:
        assert np.array_equal(_bits(got.ref), _bits(ref))
        assert [ln.split()[0] for ln in text[4:8]] == ["rmse", "mae", "maxabs", "refnorm"]
        want = dict(rmse=np.sqrt(stats[0] / 257), mae=stats[1] / 257, maxabs=stats[2], refnorm=np.sqrt(stats[3]))
        for k, v in want.items():
            assert _bits(got.stats[k]) == _bits(v), k
    else:
        assert got.stats is None and len(text) == 4 + 257


def test_comments_and_blank_lines_are_skipped(built, tmp_path):
    qf = tmp_path / "q.txt"
    qf.write_text('* a title\n\n# a remark\n"quoted"\n  1 2 3\n\t2 5 4  \n   \n1 1 1\n')
    blk, row, col, ref = primal.read_queries(qf)
    assert ref is None and list(blk) == [1, 2, 1] and list(row) == [2, 5, 1] and list(col) == [3, 4, 1]
    qf.write_text("")
    blk, row, col, ref = primal.read_queries(qf)
    assert len(blk) == 0 and ref is None


@pytest.mark.parametrize("body,line", [
    ("1 2 3\n1 2\n", 2),                 # a field short
    ("1 2 3 0.5\n1 2 3\n", 2),           # v on the first line only
    ("1 2 3\n1 2 3 0.5\n", 2),           # v on a later line only
    ("1 0 3\n", 1),                      # 1-based: no index 0
    ("1 2 -3\n", 1),
    ("# c\n\n1 2 3\nx 2 3\n", 4),        # comments and blank lines count as lines
    ("1 2.5 3\n", 1),
    ("1 2 3 0.5 7\n", 1),                # a fifth field
    ("1 2 3 abc\n", 1),
    ("1 2 3 nan\n", 1),
    ("1 2 99999999999\n", 1),
])
def test_malformed_lines_are_refused_with_their_number(built, tmp_path, body, line):
    qf = tmp_path / "q.txt"
    qf.write_text(body)
    with pytest.raises(ValueError, match="line %d " % line):
        primal.read_queries(qf)


def test_grouping_restores_the_file_order(built):
    rng = np.random.default_rng(3)
    blk = rng.integers(1, 6, 1000)
    blk[blk == 4] = 5   # (a block without queries)
    perm, start = primal.group_queries(blk, 5)
    assert start[0] == 0 and start[-1] == 1000 and sorted(perm) == list(range(1000))
    for k in range(5):
        run = perm[start[k]:start[k + 1]]
        assert np.all(blk[run] == k + 1) and np.all(np.diff(run) > 0)   # the block's queries, in file order
    assert start[4] == start[3]
    # values dealt per block and put back through perm stand in the file order
    val = np.zeros(1000)
    for k in range(5):
        run = perm[start[k]:start[k + 1]]
        val[run] = 1000.0 * (k + 1) + np.arange(len(run))
    seen = {}
    for e in range(1000):
        assert val[e] == 1000.0 * blk[e] + seen.get(blk[e], 0)
        seen[blk[e]] = seen.get(blk[e], 0) + 1
    with pytest.raises(ValueError):
        primal.group_queries([1, 7], 5)


def test_oracle_session_cannot_query_the_primal(oracle_lib):
    s = common.oracle_session(common.instance_path("theta30"))
    try:
        assert not s.be.has_primal()
        with pytest.raises(NotImplementedError):
            s.primal_entries(0, [0], [0])
        with pytest.raises(NotImplementedError):
            s.primal_apply(0, np.ones(30))
        with pytest.raises(NotImplementedError):
            s.primal_diag(0)
    finally:
        s.close()


def test_table_mirror_has_the_primal_pair(built):
    names = [f[0] for f in host.BackendStruct._fields_]
    assert "primal_entries" in names and names.index("primal_apply") == names.index("primal_entries") + 1
    lib = host.host_lib()
    lib.lrd_backend_sizeof.restype = C.c_size_t
    assert lib.lrd_backend_sizeof() == C.sizeof(host.BackendStruct)
    hip = C.CDLL(os.path.join(host.LIB_DIR, "liblorads_hip.so"))
    assert hasattr(hip, "lorads_hip_primal_entries") and hasattr(hip, "lorads_hip_primal_apply")


@pytest.mark.parametrize("body", ["1 2\n", "1 2 3\n1 2 3 4\n", "1 1 31\n", "2 1 1\n"])
def test_cli_refuses_a_bad_query_file_before_the_backend(built, tmp_path, body):
    """malformed, mixed, a position outside the cone, a block outside the problem: exit code 2 and nothing solved"""
    qf = tmp_path / "q.txt"
    qf.write_text(body)
    exe = os.path.join(host.LIB_DIR, "lorads")
    r = subprocess.run([exe, common.instance_path("theta30"), "--entriesFile", str(qf)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "query" in r.stderr and "HIP backend" not in r.stderr
    r = subprocess.run([exe, common.instance_path("theta30"), "--entriesOut", str(qf)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--entriesFile" in r.stderr
