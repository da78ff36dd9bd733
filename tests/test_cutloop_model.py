"""The cut-tightened +-1 structure without a GPU: the appending writer (lrd_session_write_tightened_keep) against
the model's (tests/cutloop_model.py), the host recogniser (Session.present_cuts) on what the writer makes, on scaled rows and on
every malformed file, through the oracle library's session as test_triangle_model.py does."""
import numpy as np
import pytest

from lorads_amd import host, instances
from lorads_amd.cuts import Cuts, read_sdpa, read_tightened
from tests import common
from tests import cutloop_model as cm
from tests import triangle_model as tm


def _cuts(lst):
    a = np.array(lst, dtype=np.int64).reshape(-1, 5)
    return Cuts(np.zeros(int(a[:, 0].max()) + 1 if len(a) else 1, dtype=np.int64), a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], np.zeros(len(a)))


def _open(path):
    return host.Session.open(path, lib=common.load_oracle())


def _random_cuts(prob, count, seed):
    """`count` different (cone, p, q, s, cls) of the problem's cones"""
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < count:
        k = int(rng.integers(0, len(prob["blocks"])))
        p, q, s_ = sorted(rng.choice(prob["blocks"][k], 3, replace=False).tolist())
        c = (k, p, q, s_, int(rng.integers(0, 4)))
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def _same_file(got_path, want):
    gm, gblocks, gb, gent = read_sdpa(got_path)
    assert (gm, gblocks) == (want["m"], list(want["blocks"]))
    assert np.array_equal(gb, np.asarray(want["b"], dtype=np.float64))
    assert sorted(gent) == sorted((int(a), int(b), int(c), int(d), float(v)) for a, b, c, d, v in want["entries"])


def _tightened_file(tmp_path, name, ncut, seed=0):
    """(the generator dict, its path, the cuts) of instance `name` tightened with ncut random cuts by the C writer"""
    prob = instances.NAMED[name]()
    cuts = _random_cuts(prob, ncut, seed or len(name))
    path = str(tmp_path / (name + "_t.dat-s"))
    s = _open(common.generated_instance(name))
    try:
        assert s.present_cuts() == []
        s.write_tightened(path, _cuts(cuts))
    finally:
        s.close()
    return prob, path, cuts


@pytest.mark.parametrize("name", ["maxcut100", "blk4x60", "scaledpm1_120"])
def test_appending_writer_against_model_writer(tmp_path, name):
    prob = instances.NAMED[name]()
    all_cuts = _random_cuts(prob, 70, len(name))
    first, more = all_cuts[:40], all_cuts[40:]
    one, two, none = (str(tmp_path / f) for f in ("one.dat-s", "two.dat-s", "none.dat-s"))
    s = _open(common.generated_instance(name))
    try:
        assert s.present_cuts() == []
        s.write_tightened(one, _cuts(first))
        s.write_tightened(none, None, keep=[])
        with pytest.raises(ValueError):
            s.write_tightened(str(tmp_path / "bad.dat-s"), _cuts(first), keep=[True])   # (a mask for a problem without cuts)
    finally:
        s.close()
    # an untightened problem: what today's writer gives (test_triangle_model.py compares the same two)
    want1 = tm.tightened(prob, first)
    _same_file(one, want1)
    _same_file(none, tm.tightened(prob, []))
    assert read_tightened(one, prob["m"]) == first
    present = cm.first_present(prob, first)
    keep = np.random.default_rng(7).random(40) >= 1 / 3
    assert 8 <= int((~keep).sum()) <= 20
    s = _open(one)
    try:
        got = s.present_cuts()
        assert got == present and all(c.scale == 1.0 for c in got)
        assert s.write_tightened(two, _cuts(more), keep=keep) == int((~keep).sum())
        same = str(tmp_path / "same.dat-s")
        assert s.write_tightened(same, None, keep=np.ones(40, dtype=bool)) == 0   # nothing new, nothing dropped: the problem itself
        _same_file(same, want1)
        with pytest.raises(ValueError, match="already in the problem"):
            s.write_tightened(str(tmp_path / "dup.dat-s"), _cuts(more[:3] + [first[5]]))
        s.write_tightened(str(tmp_path / "readded.dat-s"), _cuts([first[int(np.nonzero(~keep)[0][0])]]), keep=keep)   # (a dropped cut may return)
        with pytest.raises(ValueError, match="already in the problem"):
            s.write_tightened(str(tmp_path / "dup.dat-s"), _cuts([more[0], more[1], more[0]]))
        with pytest.raises(ValueError):
            s.write_tightened(str(tmp_path / "bad.dat-s"), _cuts(more), keep=keep[:-1])
        with pytest.raises(ValueError):
            s.write_tightened(str(tmp_path / "bad.dat-s"), _cuts([(len(prob["blocks"]), 0, 1, 2, 0)]))   # (the slack block is no cone)
    finally:
        s.close()
    want2, now = cm.appended(want1, present, keep, more)
    _same_file(two, want2)
    assert want2["m"] == prob["m"] + int(keep.sum()) + 30 and want2["blocks"][-1] == -(int(keep.sum()) + 30)
    s = _open(two)
    try:
        assert s.present_cuts() == now
    finally:
        s.close()


def test_recogniser_refuses_each_malformed_file_and_names_the_place(tmp_path):
    for name in ("maxcut100", "blk4x60"):
        prob, path, cuts = _tightened_file(tmp_path, name, 6)
        tight = tm.tightened(prob, cuts)
        cases = cm.malformed(tight, prob["m"])
        assert ("two_cones" in cases) == (name == "blk4x60") and len(cases) >= 6
        for case, (bad, needle) in cases.items():
            bad_path = str(tmp_path / ("%s_%s.dat-s" % (name, case)))
            instances.write_sdpa(bad, bad_path)
            s = _open(bad_path)
            try:
                with pytest.raises(ValueError) as e:
                    s.present_cuts()
                why = str(e.value)
                print("%s / %s: %s" % (name, case, why))
                assert why.startswith("block %d is an LP block" % len(tight["blocks"])) and needle in why + " ", (case, why)
                with pytest.raises(ValueError) as e2:   # the writer refuses the same file for the same reason
                    s.write_tightened(str(tmp_path / "x.dat-s"), _cuts([(0, 0, 1, 2, 0)]))
                assert why in str(e2.value)
            finally:
                s.close()


def test_recogniser_refuses_an_lp_block_of_another_kind():
    s = _open(common.instance_path("sdplp40"))
    try:
        with pytest.raises(ValueError, match="LP block"):
            s.present_cuts()
    finally:
        s.close()


@pytest.mark.parametrize("factor", [3.0, 0.5])
def test_recogniser_accepts_positive_multiples_of_a_row(tmp_path, factor):
    prob, path, cuts = _tightened_file(tmp_path, "scaledpm1_120", 6)
    row = prob["m"] + 3
    sc_path = str(tmp_path / "scaled.dat-s")
    instances.write_sdpa(cm.scaled(tm.tightened(prob, cuts), row, factor), sc_path)
    s = _open(sc_path)
    try:
        got = s.present_cuts()
    finally:
        s.close()
    assert got == cm.first_present(prob, cuts)
    assert all(c.scale == 1.0 for c in got)   # (b / -c is the row's own: a multiple of the whole row leaves it)
    # the slack column's coefficient alone scaled: the slack is counted in other units, scale = -b / c = 1 / factor
    tight = tm.tightened(prob, cuts)
    tight["entries"] = [(mat, blk, i, j, v * factor if mat == row and blk == len(tight["blocks"]) else v) for mat, blk, i, j, v in tight["entries"]]
    instances.write_sdpa(tight, sc_path)
    s = _open(sc_path)
    try:
        got = s.present_cuts()
    finally:
        s.close()
    assert got == cm.first_present(prob, cuts)
    assert [c.scale for c in got] == [1.0 / factor if c.row == row - 1 else 1.0 for c in got]


def test_struct_mirrors_and_entry_points():
    import ctypes as C
    from lorads_amd.cuts import PresentStruct
    from lorads_amd.rounding import RoundingStruct
    lib = host.host_lib()
    for f in ("lrd_session_present_cuts", "lrd_present_free", "lrd_cuts_why", "lrd_session_write_tightened_keep",
              "lrd_session_write_tightened_drop", "lrd_session_write_tightened"):
        assert hasattr(lib, f)
    assert C.sizeof(PresentStruct) == 8 + 9 * C.sizeof(C.c_void_p)
    assert [f[0] for f in RoundingStruct._fields_][-3:] == ["nlp", "lp_neg", "lp_upper"]
