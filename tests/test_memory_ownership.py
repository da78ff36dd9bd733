"""Every device and pinned allocation of the HIP backend has one owner (DevPool, csrc/hip/dev_pool.inc): what a context, its
plans and its scratch hold is counted by lorads_hip_memory_stats and is gone, to the byte, when the context is.  The counters
are exact integers of this process, so every comparison is `==`."""
import pytest

from lorads_amd import host
from tests import common
from tests.test_hip_abi_edges import Ctx, _i, lib  # noqa: F401  (`lib`: the fixture with the raw C ABI bound)

pytestmark = pytest.mark.gpu

# one golden instance of each image kind
KINDS = [
    "maxcut100",    # Max-Cut type, one-launch iteration, rounding
    "blk4x60",      # merged cone, lockstep sweep
    "densec40",     # dense objective (Wd, Wpart)
    "densea40",     # dense constraint matrices (Wj)
    "sdplp40",      # LP block
    "matcomp60",    # single-entry cone, bipartite entry graph
    "rand120",      # constraint-wise operator, one-kernel front
    "coupled3x70",  # coupled cones: no merged view
]


def mem():
    d = host.Session.hip_memory_stats()
    return (d["device_allocations"], d["device_bytes"], d["pinned_allocations"], d["pinned_bytes"])


def _alm_steps(s, iters=3, rho=0.7):
    be = s.be
    be.init_constr(host.PAIR_RR)
    be.alm_cal_grad(rho)
    front = be.alm_front(rho, 0)
    for it in range(iters):
        tau, _ = common.linesearch_tau(front[2])
        out = be.alm_step(rho, tau, it + 1)
        front = (out[2], out[3], out[4])


def _admm_steps(s, iters=3, rho=1.0):
    log = []
    for _ in range(iters):
        log.append(s.be.admm_step(rho, 1e-8, 800))
        s.be.update_dual_var(rho)
    return log


def _walk(s, name):
    """a few steps of both phases, the solution export (and the rounding), then a rank growth, more steps and the dual
    infeasibility.  The growth goes straight to the backend's table, so what follows it keeps to calls whose buffers are not
    sized by the host's own record of the ranks."""
    _alm_steps(s)
    s.be.alm_to_admm()
    s.be.init_constr(host.PAIR_UV)
    _admm_steps(s)
    s.solution()
    if name == "maxcut100":
        s.round_pm1(trials=128)
        s.round_pm1(trials=512)  # (the trial buffers grow: the old ones are replaced)
    ranks = [s.block_shape(k)[1] for k in range(s.nblk)]
    s.be.resize_rank([r if r == 1 else r + 1 for r in ranks])  # (rank 1: the LP block, which has no factor width to grow)
    s.be.init_constr(host.PAIR_UV)
    _admm_steps(s)
    s.hip_dual_infeasibility(tol=1e-6)


@pytest.mark.parametrize("name", KINDS)
def test_a_closed_context_leaves_nothing_behind(built, name):
    before = mem()
    s = common.hip_session(common.instance_path(name), phase1Tol=1e-2)
    try:
        opened = mem()
        assert opened[0] > before[0] and opened[1] > before[1] and opened[2] > before[2] and opened[3] > before[3], (before, opened)
        _walk(s, name)
        now = mem()
        assert now[1] > before[1] and now[0] > before[0], (before, now)
    finally:
        s.close()
    assert mem() == before, (name, before, mem())


def test_two_contexts_side_by_side(built):
    path = common.instance_path("rand120")

    def solve(s):
        _alm_steps(s)
        s.be.alm_to_admm()
        s.be.init_constr(host.PAIR_UV)
        return _admm_steps(s, iters=5)

    with common.hip_session(path, phase1Tol=1e-2) as alone:
        want = solve(alone)
    before = mem()
    first = common.hip_session(common.instance_path("maxcut100"), phase1Tol=1e-2)
    try:
        with_first = mem()
        added = tuple(a - b for a, b in zip(with_first, before))
        assert min(added) > 0, added
        second = common.hip_session(path, phase1Tol=1e-2)
        try:
            both = mem()
            first.close()
            assert mem() == tuple(a - b for a, b in zip(both, added)), (both, added, mem())
            got = solve(second)
            assert [x[:2] for x in got] == [x[:2] for x in want], (got, want)  # (CG count and objective of every iteration)
        finally:
            second.close()
    finally:
        first.close()
    assert mem() == before, (before, mem())


def test_refusals_leave_nothing_behind(lib):  # noqa: F811
    """the refused creates of test_malformed_input_is_refused and refused rank changes: error codes of the library's own input
    checks, each taken at a different depth of the set-up"""
    before = mem()
    for cones in ([(3, 2, [0], [[(0, 2, 1.0)]], [])],    # row < col: not lower-triangular
                  [(3, 2, [5], [[(1, 1, 1.0)]], [])],    # constraint index >= m
                  [(3, 2, [0], [[(3, 0, 1.0)]], [])],    # row >= n
                  [(3, 600, [0], [[(1, 1, 1.0)]], [])]):  # rank beyond the row kernels
        cx = Ctx(lib, 1, [1.0], cones)
        assert cx.rc != 0 and not cx.h
        assert mem() == before, (cones, before, mem())
    # ... the same where earlier cones of the context have been built already
    cx = Ctx(lib, 2, [1.0, 1.0], [(3, 2, [0], [[(1, 1, 1.0)]], []), (3, 2, [1], [[(0, 2, 1.0)]], [])])
    assert cx.rc != 0 and b"lower-triangular" in lib.lorads_hip_last_error()
    assert mem() == before, (before, mem())
    cx = Ctx(lib, 2, [1.0, 0.5], [(4, 3, [0], [[(1, 1, 1.0)]], [(2, 0, -1.0)]), (3, 2, [1], [[(2, 1, 1.0)]], [])])
    try:
        assert cx.rc == 0, lib.lorads_hip_last_error()
        held = mem()
        assert held[1] > before[1]
        low, high, grown = _i([2, 2]), _i([3, 600]), _i([4, 3])
        assert lib.lorads_hip_resize_rank(cx.h, low[1]) != 0  # below the current rank
        assert b"resize_rank:" in lib.lorads_hip_last_error()
        assert mem() == held
        assert lib.lorads_hip_resize_rank(cx.h, high[1]) != 0
        assert b"resize_rank:" in lib.lorads_hip_last_error()
        assert mem() == held
        assert lib.lorads_hip_resize_rank(cx.h, grown[1]) == 0  # (and the context is still whole)
    finally:
        cx.close()
    assert mem() == before, (before, mem())
