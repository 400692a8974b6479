"""The half-step planner (naima_amd/csrc/nh_hs_plan.h) without a GPU: a stand-alone program
(tests/plan_shape_host.cpp), built host-only under the address and undefined-behaviour sanitizers,
replays the sizes of every case of tests/golden/plan_shapes.json -- recorded on an MI355X through
the library's own entry points (plan_shape_cases.py) -- and must decide what the library decided
there: threads, blocks, split, LDS bytes and the synchrotron form of every plan; threads,
LDS bytes, the log-domain form with its piece size and count, tables in registers, workgroups per
walker and the row split of the resident loop (its grid and the two-walkers-in-flight instance
follow from the runtime's occupancy answer: test_gpu_plan_shapes.py).  A refusal on record that
the planner itself makes must come back with the same message; the one the occupancy decides
("more walkers per half-step than resident workgroups") is the GPU test's.

Every branch of the planner has to occur in some case: split 1 / 2 / 4 / 8, the row split, register-
resident tables, 256 / 512 / 1024 threads, the log-domain form on and off, s2_own on and off,
tcompact, segscale > 1 (cfg3 at 8 and at 128 walkers per half-step: coarser items before fewer
workgroups).  The recorded cases reach all but one, which synthetic sizes drive and properties
check (lds_core <= 150 KB, the item count within its cap, every block of the layout inside the
LDS asked for):
  split = 4       cfg3's sizes at 64 walkers per half-step"""
import copy
import os
import shutil
import subprocess

import pytest

import plan_shape_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

PLAN_KEYS = ("threads", "blocks", "split", "lds_bytes", "syn_form")
RUN_KEYS = ("threads", "lds_bytes", "syn_log_domain", "syn_nodes_per_piece", "syn_pieces",
            "tables_in_registers", "workgroups_per_walker", "rows_split")
OCCUPANCY_REFUSAL = "more walkers per half-step than resident workgroups"


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_shape") / "plan_shape_host")
    subprocess.run([HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-g",
                    "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "plan_shape_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)

    def run(rec, want_resident=True):
        """the program's lines for a case's record -> ([plan dicts], run dict or None)"""
        tok = [rec["ncu"], rec["knobs"]["run_rt"], int(want_resident), len(rec["plans"])]
        for p in rec["plans"]:
            d = p["in"]
            tok += [d["ns"], d["ndim"], d["lo"], d["nloc"], d["kind"], d["do_accept"],
                    d["write_weights"], d["send_width"], d["has_lp"], d["nE"], d["nterms"]]
            tok.append(len(d["grids"]))
            for g in d["grids"]:
                tok += [g["nG"], repr(g["unit_scale"])]
            tok += [len(d["moms"])] + d["moms"]
            tok.append(len(d["tabs"]))
            for t in d["tabs"]:
                tok += [t["grid"], t["nK"], t["ldo"], t["nonnegative"], t["r0"]]
            s = d["syn"]
            tok.append(s["grid"])
            if s["grid"] >= 0:
                tok += [s["nE"], s["n1"], s["ldo"], s["ldo2"], s["two_outputs"], s["bcol"],
                        repr(s["x_first"]), repr(s["x_last"])]
            tok.append(len(d["comps"]))
            for c in d["comps"]:
                tok += [c["table"], c["at"]]
            tok.append(len(d["blobs"]))
            for b in d["blobs"]:
                tok += [b["kind"], b["m"], b["mom"]]
        r = subprocess.run([exe], input=" ".join(str(t) for t in tok), capture_output=True,
                           text=True)
        assert r.returncode == 0 and "runtime error" not in r.stderr and \
            "AddressSanitizer" not in r.stderr, r.stderr  # (clean under both sanitizers)
        plans, resident = [], None
        for line in r.stdout.splitlines():
            kind, _, rest = line.partition(" ")
            fields = {}
            if " error=" in rest:
                rest, _, fields["error"] = rest.partition(" error=")
            for kv in rest.split():
                key, _, v = kv.partition("=")
                fields[key] = int(v)
            if kind == "plan":
                plans.append(fields)
            else:
                resident = fields
        return plans, resident

    return run


@pytest.fixture(scope="module")
def replayed(planner):
    """every golden case through the planner, once"""
    golden = PC.load_golden()
    return golden, {cid: planner(rec) for cid, rec in golden.items()}


def test_golden_file_holds_every_case(replayed):
    golden, _ = replayed
    assert sorted(golden) == sorted(PC.case_ids())


@pytest.mark.parametrize("cid", PC.case_ids())
def test_planner_decides_what_the_library_decided(replayed, cid):
    golden, got = replayed
    rec, (plans, resident) = golden[cid], got[cid]
    assert len(plans) == len(rec["plans"])
    for p, g in zip(plans, rec["plans"]):
        assert p["rc"] == 0, p
        assert {k: p[k] for k in PLAN_KEYS} == {k: g["out"][k] for k in PLAN_KEYS}
        assert p["offsets_inside"] == 1 and p["lds_core"] <= 150 * 1024 and p["nT"] <= p["nT_cap"]
    if rec["resident"] is not None:
        assert resident["rc"] == 0, resident
        assert {k: resident[k] for k in RUN_KEYS} == {k: rec["resident"][k] for k in RUN_KEYS}
        assert resident["offsets_inside"] == 1 and resident["lds_bytes"] <= 160 * 1024
    elif rec.get("resident_reason") is None:
        pass  # (the device loop did not ask for a resident loop: a staged plan)
    elif OCCUPANCY_REFUSAL in rec["resident_reason"]:
        assert resident["rc"] == 0, resident  # (the planner has no objection: the grid step refuses)
    else:
        assert resident["rc"] != 0 and resident["error"] == rec["resident_reason"]


def test_every_branch_occurs_in_a_golden_case(replayed):
    golden, got = replayed
    plans = [p for ps, _ in got.values() for p in ps]
    runs = [r for _, r in got.values() if r is not None and r["rc"] == 0]
    assert {p["split"] for p in plans} >= {1, 2, 8}
    assert {p["threads"] for p in plans} == {256, 512, 1024}
    assert {p["rowsplit"] for p in plans} == {0, 1} and {p["rt"] for p in plans} == {0, 1}
    assert {p["syn_form"] for p in plans} == {0, 1, 2}
    assert {r["rows_split"] for r in runs} == {0, 1}
    assert {r["tables_in_registers"] for r in runs} == {0, 1}
    assert {r["syn_log_domain"] for r in runs} == {0, 1}
    assert {r["s2_own"] for r in runs if r["syn_log_domain"]} == {0, 1}
    assert {r["tcompact"] for r in runs} == {0, 1}
    assert {p["segscale"] for p in plans} >= {1, 2}
    # the one that no recorded case reaches (test_synthetic_four_workgroups_per_walker)
    assert 4 not in {p["split"] for p in plans}


def _synthetic(golden, nloc):
    rec = copy.deepcopy(golden["cfg3/8"])
    d = rec["plans"][-1]["in"]
    d["ns"] = d["nloc"] = nloc
    return rec


def _properties(plans, resident):
    (p,) = plans
    assert p["rc"] == 0, p
    assert p["lds_core"] <= 150 * 1024 and p["nT"] <= p["nT_cap"] and p["offsets_inside"] == 1
    assert p["lds_bytes"] <= 160 * 1024
    if resident["rc"] == 0:
        assert resident["lds_bytes"] <= 160 * 1024 and resident["offsets_inside"] == 1
    return p


def test_synthetic_four_workgroups_per_walker(replayed, planner):
    golden, _ = replayed
    p = _properties(*planner(_synthetic(golden, 64)))
    assert p["split"] == 4
