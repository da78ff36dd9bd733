"""The bytes of the extended problem files without a GPU: the tightened files of DESIGN.md sections 14 and 20 and the bounded files of
section 15, written through the oracle library's session as test_cutloop_model.py does, against the SHA-256 digests recorded in
tests/golden/extended_files.json (names and digests only).  The model writers pin what the files mean; this pins every byte."""
import hashlib
import json
import os

import numpy as np
import pytest

from lorads_amd import instances
from tests import common
from tests.test_bounds_model import _bounds
from tests.test_cutloop_model import _cuts, _open, _random_cuts

BOUND_CUTS = [(0, 1, 2, 0, 0.0), (0, 3, 7, 1, 0.5), (0, 0, 29, 1, 0.3)]   # (cone, p, q, cls, bound)


def _digest(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _write_all(tmp):
    """the eight files, {name: path}"""
    out = {}

    def done(tag, path):
        out[tag] = path

    for name in ("maxcut100", "blk4x60", "scaledpm1_120"):
        prob = instances.NAMED[name]()
        all_cuts = _random_cuts(prob, 70, len(name))
        first, more = all_cuts[:40], all_cuts[40:]
        one = os.path.join(tmp, name + "_first40.dat-s")
        s = _open(common.generated_instance(name))
        try:
            s.write_tightened(one, _cuts(first))
        finally:
            s.close()
        done(name + "_first40", one)
        if name != "maxcut100":
            continue
        keep = np.random.default_rng(7).random(40) >= 1 / 3
        two, same = os.path.join(tmp, name + "_keep_more30.dat-s"), os.path.join(tmp, name + "_keep_all.dat-s")
        s = _open(one)
        try:
            assert s.write_tightened(two, _cuts(more), keep=keep) == int((~keep).sum())
            assert s.write_tightened(same, None, keep=np.ones(40, dtype=bool)) == 0
        finally:
            s.close()
        done(name + "_keep_more30", two)
        done(name + "_keep_all", same)
    for name, nblk in (("theta30", 1), ("sdplp40", 2)):
        path = os.path.join(tmp, name + "_bounded3.dat-s")
        s = _open(common.instance_path(name))
        try:
            s.write_bounded(path, _bounds(BOUND_CUTS, nblk))
            if name == "sdplp40":
                as_read = os.path.join(tmp, name + "_as_read.dat-s")
                s.write_bounded(as_read, None)
                done(name + "_as_read", as_read)
        finally:
            s.close()
        done(name + "_bounded3", path)
    return out


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    return _write_all(str(tmp_path_factory.mktemp("extended")))


def _recorded():
    with open(os.path.join(common.GOLD, "extended_files.json")) as f:
        return json.load(f)


def test_the_eight_files_are_recorded(written):
    assert sorted(written) == sorted(_recorded()) and len(written) == 8


@pytest.mark.parametrize("tag", ["maxcut100_first40", "maxcut100_keep_more30", "maxcut100_keep_all", "blk4x60_first40",
                                 "scaledpm1_120_first40", "theta30_bounded3", "sdplp40_bounded3", "sdplp40_as_read"])
def test_bytes_of_the_written_file(written, tag):
    assert _digest(written[tag]) == _recorded()[tag]


def test_nothing_new_and_nothing_dropped_is_the_problem_itself(written):
    """cuts=None and an all-true mask on the tightened file: its header and its entry lines, in another order (so the digests differ): the
    first writing prints every cut's slack entry behind the cut's cone entries, the second finds the slacks in the LP block of the
    problem as it was read and prints that block behind the cones, as it does every block."""
    with open(written["maxcut100_first40"]) as f, open(written["maxcut100_keep_all"]) as g:
        one, same = f.read().split("\n"), g.read().split("\n")
    assert same[:4] == one[:4] and sorted(same[4:]) == sorted(one[4:])


if __name__ == "__main__":   # records the digests of the library as it is built now
    import tempfile
    with tempfile.TemporaryDirectory() as d, open(os.path.join(common.GOLD, "extended_files.json"), "w") as f:
        json.dump({tag: _digest(path) for tag, path in _write_all(d).items()}, f, indent=1, sort_keys=True)
        f.write("\n")
