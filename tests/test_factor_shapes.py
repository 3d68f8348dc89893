"""Host-only companions of tests/test_gpu_factor_schedules.py: the facts of the analysis its six problems rely on (a change of
the ordering or of the tail selection fails here instead of quietly moving the GPU cases off the kernels' edges), what the
replay of the dense-tail plan's K-segment rule gives for the settings of the GPU cases, and the coverage of the schedule
switches: every SCILMM_* name `read_tuning()` (csrc/dev.h) reads is set by a case of a GPU module or exempted with a reason."""
import importlib
import os
import re

import numpy as np
import pytest

from scilmm_amd.factor import Symbolic
from tests import factor_shapes as FS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SYMS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_problems():
    yield
    _SYMS.clear()
    FS.release()


def _sym(pid):
    if pid not in _SYMS:
        p = FS.problem(pid)
        _SYMS[pid] = Symbolic(p["mats"], upload=False, **p["opts"])
    return _SYMS[pid]


@pytest.mark.parametrize("pid", ["R37", "R50", "R100", "R128", "P10"])
def test_the_problems_have_the_fronts_the_gpu_cases_are_about(pid):
    sym, want = _sym(pid), FS.PROBLEMS[pid][1]
    info = sym.info()
    start = sym.get("sn_start").astype(np.int64)
    rowptr = sym.get("sn_rowptr").astype(np.int64)
    level = sym.get("sn_level")
    assert (info.n, info.nsuper, info.dense_first) == (want["n"], want["nsuper"], want["dense_first"])
    assert np.diff(start)[info.dense_first:].tolist() == want["tail"]
    # a tail front stores every later row, and the tail fronts lie on a chain: one per level, in order
    for f in range(info.dense_first, info.nsuper):
        assert rowptr[f + 1] - rowptr[f] == info.n - start[f], f
    assert np.all(np.diff(level[info.dense_first:]) > 0)
    # tiles of 128 rows; a dense item takes a pair of them
    tb = sym.get("tile_base").astype(np.int64)
    assert np.array_equal(np.diff(tb)[info.dense_first:info.nsuper], (info.n - start[info.dense_first:info.nsuper] + FS.TM - 1) // FS.TM)


def test_ragged_widths_meet_every_edge_of_the_dense_kernels():
    """What the widths mean for k_dense_b (B chunks of 64 k-rows, k-steps of 4, two target columns per lane)."""
    w = {pid: FS.PROBLEMS[pid][1]["tail"] for pid in ("R37", "R50", "R100", "R128")}
    assert w["R37"][0] % 2 == 1 and w["R37"][0] % 4 != 0 and w["R37"][0] < 64 and w["R37"][-1] == 3      # odd target, klast re-read
    assert w["R50"][0] % 4 == 2 and w["R50"][0] < 64                                                       # one short chunk
    assert w["R100"][0] == 64 + 36                                                                         # a full and a short chunk
    assert w["R128"][0] == 2 * 64 and w["R128"][-1] == 8                                                   # full chunks only


def test_p10_prelude_reaches_the_tail_in_groups_of_identical_rows():
    sym, want = _sym("P10"), FS.PROBLEMS["P10"][1]["outside"]
    got = FS.outside_groups(sym)
    assert {k: got[k] for k in want} == want, got
    assert got["max_members"] == 3 and got["first_panels"] == len(FS.PROBLEMS["P10"][1]["tail"])
    # the chunk rule: what SCILMM_OUTSIDE_CHUNKS = 1 / 3 / 32 give
    assert [FS.outside_chunks(got["per_panel"], k) for k in (1, 3, 32)] == [1, 3, 10]


def test_p20_is_the_moved_tail():
    sym, want = _sym("P20"), FS.PROBLEMS["P20"][1]
    info = sym.info()
    width = np.diff(sym.get("sn_start").astype(np.int64))[info.dense_first:]
    assert (width.size, int(width.sum()), int(width[0])) == (want["nsuper_tail"], want["tail_columns"], want["first_width"])
    got = FS.outside_groups(sym)
    assert {k: got[k] for k in want["outside"]} == want["outside"], got
    assert got["first_panels"] == 24
    # 1688 items in 32 chunks would be 53 per chunk, more than thirteen of the panels start: asked for at least as many chunks
    # as there are first panels, the plan cuts at every panel
    assert min(got["per_panel"]) < -(-got["pairs"] // 32) and [FS.outside_chunks(got["per_panel"], k) for k in (1, 3, 32)] == [1, 3, 24]
    bp = sym.get("tail_blk_ptr")
    assert sym.get("tail_blk").size < (bp.size - 1) * (bp.size - 2) // 2   # padding-only blocks: the tail was moved


# (early items, longest early K segment in descendants) per setting: dense_items, dense_fill, taper
REPLAY = {
    "R37": {(128, 256, False): (12182, 2), (64, 256, False): (7225, 3), (64, 256, True): (8102, 3), (128, 0, False): (8943, 3)},
    "R128": {(128, 256, False): (4750, 1), (64, 256, False): (3333, 2), (64, 256, True): (3703, 2), (128, 0, False): (3947, 2)},
    "R50": {(128, 256, False): (88, 1), (64, 256, False): (88, 1), (64, 256, True): (88, 1), (128, 0, False): (88, 1)},
    "R100": {(128, 256, False): (13, 1), (64, 256, False): (13, 1), (64, 256, True): (13, 1), (128, 0, False): (13, 1)},
}


@pytest.mark.parametrize("pid", sorted(REPLAY))
def test_k_segments_of_the_dense_cases(pid):
    """The replay of plan_dense_level's K-segment rule on a dense matrix (one active run per target, every tile pair on): with
    64 items per launch R37 and R128 have early items over two or three descendants, the taper adds items there, and with
    the default 128 no item of R128 spans two descendants.  (The GPU cases compare the plan's own count with this replay.)"""
    sym = _sym(pid)
    np_on = FS.tail_pairs(sym)
    single = FS.single_descendant_early_items(sym)
    for (items, fill, taper), want in REPLAY[pid].items():
        assert FS.replay_early_items(np_on, items, fill, taper) == want, (items, fill, taper)
    r = REPLAY[pid]
    if pid in ("R37", "R128"):
        assert single == {"R37": 13588, "R128": 4750}[pid]
        assert r[64, 256, False][0] < single and r[64, 256, False][1] >= 2
        assert r[64, 256, True][0] > r[64, 256, False][0]
        assert r[128, 0, False][0] < single
    else:
        assert all(v == (single, 1) for v in r.values())      # nothing for the item count or the taper to change
    if pid == "R128":
        assert r[128, 256, False] == (single, 1)


def test_k_segment_replay_covers_every_descendant_once():
    for total in (1, 2, 3, 7, 37, 64, 65, 200):
        for np_on in (1, 3, 12, 20):
            for items in (64, 128, 1024):
                for fill in (0, 256):
                    for taper in (False, True):
                        segs = FS.k_segments(total, np_on, items, fill, taper)
                        assert segs[0][0] == 0 and segs[-1][1] == total and len(segs) <= 64 + 4
                        assert all(a < b for a, b in segs) and all(segs[i][1] == segs[i + 1][0] for i in range(len(segs) - 1))


# ---- coverage of the schedule switches

# switch -> why no case of tests/test_gpu_factor_schedules.py or of test_gpu_parity's schedule table sets it.  An entry
# that names a module is checked: the module's text has to name the switch.
EXEMPT = {
    "SCILMM_TUNING": "the gate: every case sets it",
    "SCILMM_RESERVE_CUS": "a CU mask moves work between CUs: no arithmetic and no item structure changes",
    "SCILMM_DIST_GROUP": "multi-rank handles: tests/test_zz_gpu_dist.py",
    "SCILMM_DIST_NOSPLIT": "multi-rank handles: tests/test_zz_gpu_dist.py",
    "SCILMM_CHAIN_PIPE": "chain sweeps: tests/test_gpu_chain_pipeline.py",
    "SCILMM_CHAIN_STAGGER": "chain sweeps: tests/test_gpu_chain_pipeline.py",
    "SCILMM_SINV_GENERIC": "selected inverse: tests/test_gpu_selected_inverse.py",
    "SCILMM_SINV_REVERSE": "selected inverse, deterministic mode: tests/test_gpu_sinv_deterministic.py",
    "SCILMM_SINV_CC_TILES": "selected inverse, deterministic mode: tests/test_gpu_sinv_deterministic.py",
}


def _switches_read_by_read_tuning():
    src = open(os.path.join(ROOT, "scilmm_amd", "csrc", "dev.h")).read()
    body = src[src.index("inline Tuning read_tuning()"):]
    body = body[:body.index("\n}\n")]
    return sorted(set(re.findall(r'"(SCILMM_[A-Z0-9_]+)"', body)))


def _covered_switches():
    """switch -> the case tables that set it: the tables of test_gpu_factor_schedules and the parametrized environments of
    test_gpu_parity.test_alternative_schedules_agree_with_oracle."""
    sched = importlib.import_module("tests.test_gpu_factor_schedules")
    parity = importlib.import_module("tests.test_gpu_parity")
    covered = {}
    for name, cases in sched.TABLES.items():
        for _, env in cases:
            for k in env:
                covered.setdefault(k, set()).add("test_gpu_factor_schedules." + name)
    marks = [m for m in parity.test_alternative_schedules_agree_with_oracle.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "env"
    for env in marks[0].args[1]:
        for k in env:
            covered.setdefault(k, set()).add("test_gpu_parity.test_alternative_schedules_agree_with_oracle")
    return covered


def test_every_schedule_switch_is_covered_or_exempt():
    """csrc/dev.h says of the switches of `Tuning` that every value gives the same factor to rounding, parity-tested: a switch
    that `read_tuning()` reads and no case sets fails here, by name."""
    names = _switches_read_by_read_tuning()
    assert len(names) > 30 and "SCILMM_DENSE_TAPER" in names and "SCILMM_TUNING" in names
    covered = _covered_switches()
    missing = [s for s in names if s not in covered and s not in EXEMPT]
    assert not missing, "no GPU case sets %s (add a case, or an entry of EXEMPT with the reason)" % ", ".join(missing)
    stale = [s for s in EXEMPT if s not in names]
    assert not stale, "EXEMPT names switches read_tuning() does not read: %s" % stale
    for s, why in EXEMPT.items():
        for mod in re.findall(r"tests/(\w+)\.py", why):
            assert s in open(os.path.join(ROOT, "tests", mod + ".py")).read(), (s, mod)
    # the switches the issue of this module is about stay in its own tables
    own = {k for k, v in covered.items() if any(t.startswith("test_gpu_factor_schedules.") for t in v)}
    for s in ("SCILMM_TRSM_LITE", "SCILMM_SHADOW", "SCILMM_NO_SPLITK", "SCILMM_TARGET_ITEMS", "SCILMM_MIN_ITEM", "SCILMM_MAX_ITEM",
              "SCILMM_DENSE_ITEMS", "SCILMM_DENSE_FILL", "SCILMM_DENSE_TAPER", "SCILMM_OUTSIDE_CHUNKS", "SCILMM_OUTSIDE_MERGE",
              "SCILMM_OUTSIDE_PRIO", "SCILMM_SIDE_STREAMS"):
        assert s in own, s


def test_the_documents_name_the_covering_module():
    """INTEGRATION.md section 3 and the comment on `Tuning` point at the modules that hold the parity cases."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 3."):doc.index("## 4.")]
    dev = open(os.path.join(ROOT, "scilmm_amd", "csrc", "dev.h")).read()
    for text in (sec, dev[:dev.index("inline Tuning read_tuning()")]):
        assert "test_gpu_factor_schedules" in text and "test_factor_shapes" in text
