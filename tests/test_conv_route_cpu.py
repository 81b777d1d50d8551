"""The conv routing (csrc/kernels/gemm_conv.hip route_fwd / route_dgrad / route_dgrad_fold) is host
arithmetic: its size queries answer without a GPU.  tests/data/conv_routes_parent.json holds the
answers of the last revision that wrote the routing out once per query (recorded with
tools/dump_conv_routes.py); the single route functions must reproduce every one of them, and the
full-geometry data-gradient query must close the gap the old one left for 3x3 pad-0 convs."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
RECORDED = os.path.join(ROOT, "tests", "data", "conv_routes_parent.json")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def recorded():
    with open(RECORDED) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def current(tmp_path_factory):
    """the current library's answers, dumped in a fresh process without MI355X_DP_* variables (the
    switches are process-wide state that other tests set)"""
    from mi355x_dp.build import build_kernels
    lib = build_kernels(verbose=False)
    out = tmp_path_factory.mktemp("routes") / "routes.json"
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI355X_DP_")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dump_conv_routes.py"), lib, "--out", str(out),
                        "--new"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out) as f:
        return json.load(f)


def test_recorded_answers_reproduced(recorded, current):
    """every query, every shape, every switch setting: exactly the recorded answer"""
    for key in ("shape_fields", "shapes", "settings", "queries"):
        assert current[key] == recorded[key], f"the tool's {key} differ from the recorded document's"
    assert len(recorded["shapes"]) >= 100 and len(recorded["settings"]) == 8
    bad = []
    for s in recorded["settings"]:
        rec, cur = recorded["answers"][s["name"]], current["answers"][s["name"]]
        assert len(rec) == len(cur) == len(recorded["shapes"])
        for shape, a, b in zip(recorded["shapes"], rec, cur):
            for q, x, y in zip(recorded["queries"], a, b):
                if x != y:
                    bad.append((s["name"], shape, q, x, y))
    assert not bad, f"{len(bad)} answers differ (setting, shape, query, recorded, now): {bad[:10]}"


def test_dgrad_rows_g_equals_old_query_on_same_padded_square_convs(recorded, current):
    n = 0
    for s in recorded["settings"]:
        for i, sh in enumerate(recorded["shapes"]):
            Nb, H, W, C, K, R, S, stride, pad, P, Q = sh
            if R == S and pad == R // 2:
                assert current["new"]["dgrad_stat_rows_g"][s["name"]][i] == recorded["answers"][s["name"]][i][1], \
                    (s["name"], sh)
                n += 1
    assert n >= 8 * 100


def test_pad0_3x3_dgrad_rows_are_the_nt_kernels(current):
    """a 3x3 pad-0 stride-1 data gradient never runs on the panel kernel (the launch sends only pad-1
    convs there), so with the 3x3 panel mode on the slab must be sized for the NT kernel: the old
    query, which took no pad, said 2 rows for Nb 2, 14x14, C = K = 64 where the NT kernel writes 4"""
    new = current["new"]
    assert new["pad0_shapes"][0] == [2, 14, 14, 64, 64, 3, 3, 1, 0, 12, 12]
    assert new["pad0_dgrad_stat_rows_g"]["panel0"][0] == 4
    for mode in ("panel5", "panel6"):
        assert new["pad0_dgrad_stat_rows_g"][mode] == new["pad0_dgrad_stat_rows_g"]["panel0"], mode
    assert len(new["pad0_shapes"]) >= 3


def test_nol_ok_only_on_the_128_tile_kernels(recorded, current):
    """mi_conv_nol_ok is 0 wherever either direction leaves the 128-tile kernels.  A row count alone
    does not name the kernel (2 * cdiv(M, 256) rows of the 256-wide kernel equal cdiv(M, 128) rows of
    the NT kernel whenever M % 256 is 0 or above 128), so the route is read from two facts: the
    count equals the stem / 256-wide / panel kernel's, and it is not what the same setting gives
    with the panel and 256-wide routes switched off."""
    qi = {q: i for i, q in enumerate(recorded["queries"])}
    off_route = 0
    for s in recorded["settings"]:
        for i, sh in enumerate(recorded["shapes"]):
            a = recorded["answers"][s["name"]][i]
            nt_f, nt_d = current["new"]["nt_only"][s["name"]][i]
            rf, rd = a[qi["conv_stat_rows_g"]], current["new"]["dgrad_stat_rows_g"][s["name"]][i]
            stem = sh[3] == 8 and sh[5] == 7  # the stem kernel has no switch to take away: C = 8 names it
            special_f = stem or (rf != nt_f and rf in (a[qi["g256_rows_fwd"]], a[qi["panel_rows_fwd"]]))
            special_d = rd != nt_d and rd in (a[qi["g256_rows_dgrad"]], a[qi["panel_rows_dgrad"]])
            assert rf == nt_f or special_f, (s["name"], sh)  # nothing but those three leaves the NT kernels
            assert rd == nt_d or special_d, (s["name"], sh)
            if special_f or special_d:
                off_route += 1
                assert a[qi["conv_nol_ok"]] == 0, (s["name"], sh)
    assert off_route >= 100
