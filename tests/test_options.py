"""The HIP backend's environment switches (lorads_amd/csrc/hip/options.inc): every name, its parse rule and its default.

tests/options_probe.cpp includes options.inc, calls read_options() and the accessors of the switches that are read after a context
is created, and prints one `field=value` line per switch.  It is compiled with the host C++ compiler (options.inc has no HIP header)
and run as a child process under chosen environments.  The expectations are literal and written from the rules, which are those the
library followed while ctx_init and build.inc read each name themselves:

  on unless the value starts with '0' (unset and the empty string: on); off unless it starts with '1'; on when the variable is
  there with any value ("0" and the empty string included: LORADS_NO_ELL=0 switches the lists OFF); integers with a clamp each;
  GRAPH, LBFGS_GRAM, PERSIST_MAP, OP_CW, ROW_DEAL and HIP_VERBOSE with values of their own.

No GPU is needed."""
import os
import re
import subprocess

import pytest

from tests import common

HIP_DIR = os.path.join(common.ROOT, "lorads_amd", "csrc", "hip")

# every switch unset
DEFAULTS = dict(
    pad_rank=1, dev_presolve=1, presolve_check=0, dev_presolve_min=32768,
    dense_a=1, ell=1, slot_ell=1, merge=1, op_cw=-1,
    graph=1, graph_batched=0, graph_forced=0,
    persist=1, shared_gpu=0, persist_carry=1, persist_l2=1, persist_rows=0, persist_linear=0,
    lbfgs_team=1, alm_sval_direct=1, alm_fold_cv=1, alm_fused_tail=1, gram=1, gram_single=0,
    entry_bip=1, fuse_dir=1, cw_quad=1, fuse_eval=1, dense_rem=1, dense_cache=1, front_diag=1, eval_diag=1,
    fold_avg=1, tile_update=1, front_lds=1, front_cw=1, fuse_cg0=1,
    row_deal=-1, pretend_cus=0, wt_stores=27, front_chain=3,
    spec_front=1, handover_on_front=1, spec_window=4, exact_refresh=0, split_front=0, lazy_scalars=1,
    seg_carry_init=1, seg_virt=1, seg_carry_dual=1, seg_carry_restart=1, seg_carry=1,
    trial_chunk=0, bisect_lds=1,
    no_batch=0, common_rank=1, lanczos_threads_of_4=4, lbfgs_team_np=0, handover_timeout_s=300, verbose=0)

# name -> the probe's field, by rule (the helper the name's line of read_options() calls)
ON_UNLESS_0 = dict(
    PAD_ODD_RANK="pad_rank", DEV_PRESOLVE="dev_presolve", LAZY_SCALARS="lazy_scalars", FUSE_DIR="fuse_dir", ENTRY_BIP="entry_bip",
    SEG_CARRY="seg_carry", SEG_CARRY_INIT="seg_carry_init", SEG_VIRT="seg_virt", SEG_CARRY_DUAL="seg_carry_dual",
    SEG_CARRY_RESTART="seg_carry_restart", CW_QUAD="cw_quad", FRONT_CW="front_cw", FUSE_CG0="fuse_cg0", FRONT_LDS="front_lds",
    SPEC_FRONT="spec_front", HANDOVER_ON_FRONT="handover_on_front", FOLD_AVG="fold_avg", TILE_UPDATE="tile_update",
    EVAL_DIAG="eval_diag", FRONT_DIAG="front_diag", DENSE_CACHE="dense_cache", BISECT_LDS="bisect_lds", FUSE_EVAL="fuse_eval",
    DENSE_REM="dense_rem", PERSIST="persist", PERSIST_L2="persist_l2", PERSIST_CARRY="persist_carry", LBFGS_TEAM="lbfgs_team",
    ALM_FUSED_TAIL="alm_fused_tail", ALM_FOLD_CV="alm_fold_cv", ALM_SVAL_DIRECT="alm_sval_direct", COMMON_RANK="common_rank")
OFF_UNLESS_1 = dict(PRESOLVE_CHECK="presolve_check", EXACT_REFRESH="exact_refresh", SPLIT_FRONT="split_front", SHARED_GPU="shared_gpu")
# present with any value; the field's value when the variable is there (the NO_* names switch their field off)
PRESENT = dict(NO_DENSE_A=("dense_a", 0), NO_ELL=("ell", 0), NO_SLOT_ELL=("slot_ell", 0), NO_MERGE=("merge", 0), NO_BATCH=("no_batch", 1))

VALUES = (None, "", "0", "00", "1", "2", "x")  # (None: unset)

# switches of DESIGN.md 8a that are not this library's: the host library's and bench.py's
NOT_THIS_LIBRARY = {"LORADS_SEPARABLE", "LORADS_BENCH_NO_PHASE1_RERUN", "LORADS_AR_TORCH", "LORADS_ALLREDUCE_SYNC", "LORADS_NO_PIN",
                    "LORADS_FORCE_DIST", "LORADS_DIST_BACKEND", "LORADS_FORCE_DEVICE"}
RETIRED = ("LORADS_NO_PUBLISH", "LORADS_AR_PLAIN", "LORADS_NO_OP_ENTRY", "LORADS_NO_ENTRY_BIP_DATA", "LORADS_NO_FRONT_CW_DATA")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("options") / "options_probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Werror", "-I", HIP_DIR,
                           os.path.join(common.ROOT, "tests", "options_probe.cpp"), "-o", exe])

    def run(env):
        base = {k: v for k, v in os.environ.items() if not k.startswith("LORADS_")}
        base.update(env)
        out = subprocess.run([exe], env=base, check=True, capture_output=True, text=True).stdout
        got = {}
        for line in out.splitlines():
            k, v = line.split("=")
            got[k] = float(v)
        return got
    return run


def _check(run, env, **changed):
    want = dict(DEFAULTS, **changed)
    got = run(env)
    assert set(got) == set(want), set(got) ^ set(want)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, (env, diff)


def test_nothing_set_gives_every_default(probe):
    _check(probe, {})


@pytest.mark.parametrize("name", sorted(ON_UNLESS_0))
def test_each_on_unless_0_name_alone_switches_its_own_field(probe, name):
    _check(probe, {"LORADS_" + name: "0"}, **{ON_UNLESS_0[name]: 0})


@pytest.mark.parametrize("name", sorted(OFF_UNLESS_1))
def test_each_off_unless_1_name_alone_switches_its_own_field(probe, name):
    _check(probe, {"LORADS_" + name: "1"}, **{OFF_UNLESS_1[name]: 1})


@pytest.mark.parametrize("name", sorted(PRESENT))
def test_each_present_name_alone_switches_its_own_field(probe, name):
    _check(probe, {"LORADS_" + name: "0"}, **{PRESENT[name][0]: PRESENT[name][1]})


@pytest.mark.parametrize("name", ["PAD_ODD_RANK", "FRONT_CW", "PERSIST", "COMMON_RANK"])
@pytest.mark.parametrize("value", VALUES)
def test_on_unless_the_value_starts_with_0(probe, name, value):
    on = 0 if value in ("0", "00") else 1
    _check(probe, {} if value is None else {"LORADS_" + name: value}, **{ON_UNLESS_0[name]: on})


@pytest.mark.parametrize("name", ["PRESOLVE_CHECK", "SHARED_GPU"])
@pytest.mark.parametrize("value", VALUES)
def test_off_unless_the_value_starts_with_1(probe, name, value):
    _check(probe, {} if value is None else {"LORADS_" + name: value}, **{OFF_UNLESS_1[name]: 1 if value == "1" else 0})


@pytest.mark.parametrize("name", ["NO_ELL", "NO_BATCH"])
@pytest.mark.parametrize("value", VALUES)
def test_present_with_any_value(probe, name, value):
    field, there = PRESENT[name]
    _check(probe, {} if value is None else {"LORADS_" + name: value}, **({} if value is None else {field: there}))


@pytest.mark.parametrize("value,want", [(None, 0), ("", 0), ("0", 0), ("00", 0), ("1", 1), ("2", 2), ("x", 0)])
def test_integer_with_clamp(probe, value, want):
    """LORADS_TRIAL_CHUNK: max(0, atoi)"""
    _check(probe, {} if value is None else {"LORADS_TRIAL_CHUNK": value}, trial_chunk=want)


def test_every_name_of_the_three_flag_rules(probe):
    """all names of a rule at once, at the value that flips them, and at a value that does not"""
    flip = {"LORADS_" + n: "0" for n in ON_UNLESS_0}
    flip.update({"LORADS_" + n: "1" for n in OFF_UNLESS_1})
    flip.update({"LORADS_" + n: "" for n in PRESENT})
    changed = {f: 0 for f in ON_UNLESS_0.values()}
    changed.update({f: 1 for f in OFF_UNLESS_1.values()})
    changed.update({f: v for f, v in PRESENT.values()})
    _check(probe, flip, **changed)
    keep = {"LORADS_" + n: "1" for n in ON_UNLESS_0}
    keep.update({"LORADS_" + n: "0" for n in OFF_UNLESS_1})
    _check(probe, keep)


def test_no_ell_0_switches_the_lists_off(probe):
    _check(probe, {"LORADS_NO_ELL": "0"}, ell=0)


@pytest.mark.parametrize("value,want", [("", 0), ("0", 0), ("1", 1), ("10", 1)])
def test_op_cw_forces_the_operator_choice(probe, value, want):
    _check(probe, {"LORADS_OP_CW": value}, op_cw=want)


@pytest.mark.parametrize("value,want", [("auto", -1), ("", -1), ("-3", 0), ("7", 7), ("40", 32)])
def test_row_deal(probe, value, want):
    _check(probe, {"LORADS_ROW_DEAL": value}, row_deal=want)


@pytest.mark.parametrize("value,want", [("0", 1), ("-5", 1), ("", 1), ("304", 304)])
def test_row_deal_cus(probe, value, want):
    """max(1, atoi) when set; unset (0 in Options): the device's own count"""
    _check(probe, {"LORADS_ROW_DEAL_CUS": value}, pretend_cus=want)


@pytest.mark.parametrize("value,want", [("", 27), ("0", 0), ("5", 5), ("255", 63)])
def test_wt_stores(probe, value, want):
    _check(probe, {"LORADS_WT_STORES": value}, wt_stores=want)


@pytest.mark.parametrize("value,want", [("7", 3), ("", 3), ("0", 0), ("2", 2)])
def test_front_chain(probe, value, want):
    _check(probe, {"LORADS_FRONT_CHAIN": value}, front_chain=want)


@pytest.mark.parametrize("value,want", [("0", 1), ("99", 8), ("1", 1), ("", 1)])
def test_spec_window(probe, value, want):
    _check(probe, {"LORADS_SPEC_WINDOW": value}, spec_window=want)


@pytest.mark.parametrize("value,want", [("0", (0, 0, 0)), ("1", (1, 0, 1)), ("2", (1, 1, 1)), ("", (1, 0, 0))])
def test_graph(probe, value, want):
    _check(probe, {"LORADS_GRAPH": value}, graph=want[0], graph_batched=want[1], graph_forced=want[2])


@pytest.mark.parametrize("value,want", [("0", (0, 0)), ("2", (1, 1)), ("1", (1, 0))])
def test_lbfgs_gram(probe, value, want):
    _check(probe, {"LORADS_LBFGS_GRAM": value}, gram=want[0], gram_single=want[1])


def test_persist_map_and_rows(probe):
    _check(probe, {"LORADS_PERSIST_MAP": "linear"}, persist_linear=1)
    _check(probe, {"LORADS_PERSIST_MAP": "xcd"})
    _check(probe, {"LORADS_PERSIST_ROWS": "4"}, persist_rows=4)
    _check(probe, {"LORADS_PERSIST_ROWS": "-1"}, persist_rows=-1)  # (raw atoi)


def test_dev_presolve_min(probe):
    _check(probe, {"LORADS_DEV_PRESOLVE_MIN": "-4"}, dev_presolve_min=0)
    _check(probe, {"LORADS_DEV_PRESOLVE_MIN": "5000000000"}, dev_presolve_min=5000000000)


@pytest.mark.parametrize("value,want", [("0", 1), ("2", 2), ("", 1), ("1", 1)])
def test_hip_verbose(probe, value, want):
    """present with any value: the messages; a leading '2': the stage times too"""
    _check(probe, {"LORADS_HIP_VERBOSE": value}, verbose=want)


def test_switches_read_after_creation(probe):
    _check(probe, {"LORADS_LANCZOS_THREADS": "0"}, lanczos_threads_of_4=1)
    _check(probe, {"LORADS_LANCZOS_THREADS": "3"}, lanczos_threads_of_4=3)
    _check(probe, {"LORADS_LANCZOS_THREADS": "9"}, lanczos_threads_of_4=4)
    _check(probe, {"LORADS_HANDOVER_TIMEOUT_S": "2.5"}, handover_timeout_s=2.5)
    _check(probe, {"LORADS_LBFGS_TEAM_NP": "6"}, lbfgs_team_np=6)


def _literals(path):
    """the string literals of a source file that are exactly a switch's name: what getenv is given (a message that speaks of a
    switch is a longer literal and is not meant)"""
    with open(path) as f:
        return re.findall(r'"(LORADS_[A-Z0-9_]+)"', f.read())


def test_options_inc_is_the_list():
    """every switch of the library stands in options.inc once and in the table of DESIGN.md 8a; no other source file of the library
    calls getenv or holds a string literal that is a switch's name (error messages may speak of a switch); the retired names
    are no string literal anywhere"""
    lits = _literals(os.path.join(HIP_DIR, "options.inc"))
    assert len(lits) == len(set(lits)), sorted(n for n in set(lits) if lits.count(n) > 1)
    with open(os.path.join(common.ROOT, "DESIGN.md")) as f:
        design = f.read()
    sec = design[design.index("\n## 8a."):design.index("\n## 9.")]
    sec = "\n".join(par for par in sec.split("\n\n") if not par.startswith("Retired"))
    table = set(re.findall(r"LORADS_[A-Z0-9_]*[A-Z0-9]", sec)) - NOT_THIS_LIBRARY
    assert set(lits) == table, (sorted(set(lits) - table), sorted(table - set(lits)))
    # the rule tables of this file name what options.inc reads by those rules (the rest have tests of their own above)
    for n in list(ON_UNLESS_0) + list(OFF_UNLESS_1) + list(PRESENT):
        assert "LORADS_" + n in lits, n
    for name in sorted(os.listdir(HIP_DIR)):
        with open(os.path.join(HIP_DIR, name)) as f:
            text = f.read()
        for r in RETIRED:
            assert '"%s"' % r not in text, (name, r)
        if name != "options.inc":
            assert "getenv" not in text, name
            assert not _literals(os.path.join(HIP_DIR, name)), (name, _literals(os.path.join(HIP_DIR, name)))
    for r in RETIRED:
        assert r not in table and r in design, r
