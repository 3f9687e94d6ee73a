"""The sketch planner (csrc/sketch_plan.cpp), checked on the CPU by
fp-mash_amd/tools/sketchplan_check.cpp under the host address and undefined-behaviour sanitizers:
the structure of every plan (tiles cover each k-mer start once, one producer per row and pass,
reads after writes, fallback schedules over the same lists) at the planner's edges, two-level
selections among them.  The program is built from the planner alone (no kernel, no device call)
and like the devmem and hostrows checks runs only where no device is visible.

Its printing mode then plans the inputs of tests/test_gpu_sketch_dispatch.py (record lengths
only), and the plan is compared with that file's restatement of the staging rules: plan_tiles /
class_counts, sample_rule, tight_kt, survivors_rule and merge_rounds."""
import json
import os
import subprocess

import numpy as np
import pytest

import test_gpu_sketch_dispatch as D
from conftest import ROOT

AMD = os.path.join(ROOT, "fp-mash_amd")
HIPCC = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import fpmash
    if fpmash.device_count() > 0:
        pytest.skip("a device is visible")
    d = tmp_path_factory.mktemp("sketchplan")
    out = str(d / "sketchplan_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall",
                    "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(AMD, "csrc", "sketch_plan.cpp"),
                    os.path.join(AMD, "tools", "sketchplan_check.cpp"), "-o", out],
                   check=True, cwd=str(d))
    return out


def test_sketchplan_structure(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "sketchplan ok", r.stdout + r.stderr


def plan_of(exe, k, s, lens, groups, device=False):
    """the planner's summary of records given by length (the structure checks run on it too)"""
    args = [exe, str(k), str(s), "1" if D.use64_of(k) else "0", "device" if device else "host"]
    args += [f"{g}:{L}" for g, L in zip(groups, lens)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout)


def model_of(k, s, lens, groups, device=False):
    """the same summary from the restated rules of test_gpu_sketch_dispatch.py"""
    tiles = D.plan_tiles(lens, groups, k, device)
    use_sel = s + s // 8 + 64 <= D.SEL_CAP
    every, kt, est, sest = [], [], [], []
    for g in sorted({t[0] for t in tiles}):
        mine = [t for t in tiles if t[0] == g]
        sampled, ev = D.sample_rule(len(mine), s)
        # a tile's list: at most its windows and s; in a sampled group ~2 every s / tiles + 64
        e = [min(s, t[2] - k + 1) for t in mine]
        if sampled:
            every.append(ev)
            if use_sel:
                kt.append(D.tight_kt(len(mine), ev, s)[0])
            e = [min(x, 2 * ev * s // len(mine) + 64) for x in e]
            if not use_sel:                         # (no a-priori sample bound without selections)
                sest.append([min(s, t[2] - k + 1) for t in mine[::ev]])
        if not (sampled and use_sel):               # a group with a selection has no merge rounds
            est.append(e)
    main, sample = D.merge_rounds(est, s), D.merge_rounds(sest, s)
    return {"tiles": D.class_counts(tiles, k), "n_slots": len(every), "every": every, "kt": kt,
            "main": [int(x) for x in main], "sample": [int(x) for x in sample]}


def assert_matches(plan, model):
    assert plan["tiles"] == model["tiles"]
    assert (plan["n_slots"], plan["every"], plan["kt"]) == (model["n_slots"], model["every"],
                                                           model["kt"])
    assert plan["rounds_small"]["main"] == model["main"]
    assert plan["rounds_small"]["sample"] == model["sample"]


@pytest.mark.parametrize("k", D.STRADDLE_K)
def test_plan_straddle(exe, k):
    lens = [n + k - 1 for n in D.STRADDLE_STARTS]
    plan = plan_of(exe, k, 1000, lens, range(len(lens)))
    assert_matches(plan, model_of(k, 1000, lens, list(range(len(lens)))))
    assert plan["tiles"] == list(np.sum([D.straddle_classes(n) for n in D.STRADDLE_STARTS], axis=0))
    assert plan["n_slots"] == 0 and not plan["thr4"]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("k", [21, 12])
def test_plan_packed_tiles(exe, k, device):
    recs, groups, _ng = D.packed_input(k, device)
    lens = [len(r) for r in recs]
    plan = plan_of(exe, k, 1000, lens, groups, device)
    assert_matches(plan, model_of(k, 1000, lens, groups, device))
    assert plan["tiles"] == list(np.sum([t for _g, t in D.PACKED_TILES], axis=0))


@pytest.mark.parametrize("starts,s,sizes", [(1100, 2048, D.MERGE_SIZES), (1100, 2049, D.MERGE_SIZES),
                                            (2100, 2048, D.MERGE_SIZES), (2100, 2049, D.MERGE_SIZES),
                                            (D.CHUNK, 16384, (2,)), (D.CHUNK, 16385, (2,))])
def test_plan_merge_rounds(exe, starts, s, sizes):
    recs, groups, _ng = D.merge_input(21, starts, sizes=sizes)
    lens = [len(r) for r in recs]
    plan = plan_of(exe, 21, s, lens, groups)
    assert_matches(plan, model_of(21, s, lens, groups))
    assert plan["rounds_small"]["main"] == [int(x) for x in D.merge_expect(starts, s, sizes=sizes)]
    assert plan["n_slots"] == 0


@pytest.mark.parametrize("s", [13597, 13598])
def test_plan_selection_group(exe, s):
    lens = [D.SEL_TILES * D.CHUNK + 20]
    plan = plan_of(exe, 21, s, lens, [0])
    assert_matches(plan, model_of(21, s, lens, [0]))
    assert plan["sample_tiles"] == [0, 0, 0, 0, D.SEL_TILES // 16, 0]
    assert bool(plan["thr4"]) == D.survivors_rule(D.SEL_TILES, s)
    if s <= 13597:
        assert plan["n_sel"] > 0 and plan["n_ssel"] > 0 and plan["tight"] == 1
        assert len(plan["rounds_small"]["fallback"]) == 8          # 224 lists
        assert len(plan["rounds_small"]["sample_fallback"]) == 4   # 14 lists
    else:
        assert plan["n_sel"] == 0 and plan["n_ssel"] == 0 and plan["tight"] == 0
        assert (len(plan["rounds_small"]["main"]), len(plan["rounds_small"]["sample"])) == (8, 4)
        assert plan["rounds_small"]["fallback"] == [] == plan["rounds_small"]["sample_fallback"]


@pytest.mark.parametrize("k,s,ntile", D.SURVIVOR_CASES + [(21, 1000, 31), (21, 1000, 63)])
def test_plan_survivor_shapes(exe, k, s, ntile):
    lens = [ntile * D.CHUNK + k - 1]
    plan = plan_of(exe, k, s, lens, [0])
    assert_matches(plan, model_of(k, s, lens, [0]))
    assert plan["tiles"] == [0, 0, 0, 0, ntile, 0]
    assert bool(plan["thr4"]) == D.survivors_rule(ntile, s)
    sampled, every = D.sample_rule(ntile, s)
    assert plan["n_slots"] == int(sampled)
    assert plan["sample_tiles"][4] == (-(-ntile // every) if sampled else 0)
