"""The lattice table's arithmetic (vr_planar_lattice.hpp; MODE_ABSORB_FLAT_LATTICE, pq_hit_lattice) on
the host.  No GPU: tests/aux/planar_lattice.cpp checks against a double-precision brute force that every lattice disk whose
ball meets a round's padded box lies inside the index window — over random boxes, phases, pitches (also 0.5 and 0.37),
radii and centres jittered by up to delta / 8 — that the window never leaves the table, that a lane's cell of the window
is l % w, l / w, and that the table rule takes lattice clouds (with holes, with jitter) and refuses a centre 0.3 delta off,
two disks in one cell and a table of more than 4 N words.  The same program runs once more built with AddressSanitizer
and UndefinedBehaviorSanitizer, stand-alone."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "viennaray_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "aux", "planar_lattice.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", CSRC]


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "\n0 failed checks" in out.stdout and "FAILED" not in out.stdout
    m = re.search(r"^(\d+) window cases: (\d+) disks, (\d+) of them meeting the box, (\d+) clamped ends, (\d+) empty windows, "
                  r"(\d+) centres at the tolerance's edge$", out.stdout, flags=re.M)
    assert m, out.stdout
    cases, disks, meeting, clamped, empty, edge = (int(v) for v in m.groups())
    assert cases >= 20_000 and disks >= 10_000_000
    # (the check is about the disks that meet the box, about windows cut at the table's edge and about empty ones)
    assert meeting >= 5 * cases and clamped >= cases // 10 and empty >= cases // 100 and edge >= disks // 100
    assert re.search(r"^20480 lane cells$", out.stdout, flags=re.M)
    assert re.search(r"^table rule: 5 clouds taken, 3 refused$", out.stdout, flags=re.M)
    return out


def test_window_holds_every_disk_that_meets_the_box(tmp_path):
    exe = str(tmp_path / "planar_lattice")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    _run(exe)


def test_lattice_arithmetic_under_sanitizers(tmp_path):
    """the same program with ASan and UBSan, run stand-alone (nothing is loaded into python)"""
    exe = str(tmp_path / "planar_lattice_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
