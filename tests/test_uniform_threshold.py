"""The uniform-disk neighbour test compares the squared distance with a threshold T instead of taking its square root
(vr_uniform_disks.hpp: uniform_disk_threshold, made on the host at prepare).  No GPU: tests/aux/uniform_threshold.cpp
checks (radius > sqrtf(x)) == (x < T) on the host for the radii 0.8660254 x gridDelta with gridDelta 1, 0.5, 0.01 and
37.3, and 1, 2^-20 and 3e18 — every float within 65 536 ulps of radius^2, 10^7 random positive floats, +0, +infinity and
a NaN each — and that T is the smallest float whose square root reaches the radius."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_threshold_replaces_the_square_root(tmp_path):
    exe = str(tmp_path / "uniform_threshold")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           os.path.join(ROOT, "tests", "aux", "uniform_threshold.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "\n0 failed checks" in out.stdout
    rows = re.findall(r"^radius (\S+)  T \S+ \(radius\^2 [+-]\d+ ulps\)  (\d+) inputs  0 mismatches$", out.stdout, flags=re.M)
    assert len(rows) == 7, out.stdout
    for _, n in rows:  # (2 x 65 536 + 1 neighbours of radius^2, 10^7 random floats, three special values)
        assert int(n) == 131073 + 10_000_000 + 3, rows
