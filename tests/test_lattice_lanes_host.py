"""Four corners per lane (MODE_ABSORB_FLAT_LATTICE_LANES, pq_hit_lattice_lanes; vr_planar_lattice.hpp: lattice_lanes_rule,
lattice_lane_corner, lattice_window_slot) on the host.  No GPU: tests/aux/lattice_lanes.cpp tests every disk of a lattice
against points that are random, on lattice lines and within +-4 ulp of them, at the table's edges and non-finite — pitches 1,
0.5 and 0.37, phases 0, 0.37 and -499.5, radii at the rule's limit and just below it, centres jittered by up to exactly
delta / 8 — and every disk planar_round_cand accepts is one of the four corners of the cell the cell function names, inside
the round's window, in the slot of the lane that files it; every index handed out is inside the table or flagged absent.
The rule refuses a radius one ulp above its limit and a scene so far from the origin that the rounding eats the margin,
and takes the headline scene's numbers.  The same program runs built with AddressSanitizer and UndefinedBehaviorSanitizer,
stand-alone."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "viennaray_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "aux", "lattice_lanes.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", CSRC]


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "\n0 failed checks" in out.stdout and "FAILED" not in out.stdout
    m = re.search(r"^(\d+) clouds, (\d+) points \((\d+) on or beside lattice lines, (\d+) not finite or huge\), (\d+) accepting disks, "
                  r"(\d+) absent corners, (\d+) centres at the tolerance's edge, (\d+) window slots$", out.stdout, flags=re.M)
    assert m, out.stdout
    clouds, points, lines, nonfinite, accepted, absent, edge, slots = (int(v) for v in m.groups())
    assert clouds == 27 and points >= 200_000 and lines >= 50_000 and nonfinite >= 500
    # (the check is about the disks that accept a point; corners beyond the table and centres at delta / 8 must occur)
    assert accepted >= points and slots == accepted and absent >= points // 10 and edge >= 1000
    m = re.search(r"^rule: limit radius (\S+) at pitch 1 \(headline scene\), refusing offset (\S+)$", out.stdout, flags=re.M)
    assert m, out.stdout
    assert 0.87 < float(m.group(1)) < 0.875 and float(m.group(2)) == 8192.0
    return out


def test_every_accepting_disk_is_a_corner_of_the_points_cell(tmp_path):
    exe = str(tmp_path / "lattice_lanes")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    _run(exe)


def test_lane_corner_arithmetic_under_sanitizers(tmp_path):
    """the same program with ASan and UBSan, run stand-alone (nothing is loaded into python)"""
    exe = str(tmp_path / "lattice_lanes_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
