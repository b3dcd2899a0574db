"""The one-point-per-round forms of the planar-disk tests (vr_planar_disks.hpp (1) - (3); trace_kernel
MODE_ABSORB_FLAT_PLANAR_ROUND, pq_hit_packet ROUND) on the host.  No GPU: tests/aux/planar_round.cpp compares
planar_round_point / planar_round_cand with the header's two-point forms over more than 10^7 cases (equal decisions, equal
bits of t where the hit test accepts), checks that the ball filter passes every accepted centre on the box of the lane's
point alone, and that a lane the wall rule calls wall-free is rejected by the wall test's float pre-tests for all four walls,
with origins on and one ulp outside a wall, points on the shrunk rectangle's edge and t near tnear.  The same program runs
once more built with AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "aux", "planar_round.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall"]


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "\n0 failed checks" in out.stdout
    m = re.search(r"^(\d+) cases: (\d+) hit accepts, (\d+) neighbour accepts, (\d+) with t near tnear; (\d+) box checks, "
                  r"(\d+) of them at the acceptance edge$", out.stdout, flags=re.M)
    assert m, out.stdout
    cases, hits, locals_, near, boxes, edge = (int(v) for v in m.groups())
    assert cases >= 10_000_000
    # (the comparison is about accepted hits as much as about refusals)
    assert hits >= cases // 50 and locals_ >= cases // 50, (cases, hits, locals_)
    assert near >= cases // 20 and boxes >= cases // 50 and edge >= boxes // 4, (near, boxes, edge)
    w = re.search(r"^(\d+) wall cases: (\d+) wall-free, (\d+) of them with a plane hit, (\d+) origins on a wall, (\d+) one ulp outside, "
                  r"(\d+) aims at the shrunk edge, (\d+) rectangles beyond the limit, (\d+) origins outside; "
                  r"smallest wall parameter ([0-9.]+) t$", out.stdout, flags=re.M)
    assert w, out.stdout
    total, free, free_hits, on_wall, outside, on_edge, beyond, refused = (int(v) for v in w.groups()[:8])
    assert total >= 3_000_000
    assert free_hits >= total // 20 and free >= free_hits
    assert min(on_wall, outside, on_edge, beyond, refused) >= total // 10
    assert float(w.group(9)) >= 1.0017  # (the derivation's bound, in double)
    return out


def test_round_forms_equal_the_planar_forms(tmp_path):
    exe = str(tmp_path / "planar_round")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    _run(exe)


def test_round_forms_under_sanitizers(tmp_path):
    """the same program with ASan and UBSan, run stand-alone (nothing is loaded into python)"""
    exe = str(tmp_path / "planar_round_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
