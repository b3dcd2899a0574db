"""vr_bin_grid.hpp on the host (no GPU): the rule that sizes the aligned sort-bin grid and the generator's float key,
against a double-precision reference over a table of domains (tests/aux/bin_grid.cpp has the table and the checks:
cells and bins in range for 1e6 positions per row under every wall fold, float cell == double cell except within 2 ulp
of an edge, every edge on a lattice line, mean rays per bin within the rule's bounds or the fall-back taken, the caps)."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bin_grid_rule_and_key(tmp_path):
    exe = str(tmp_path / "bin_grid")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "aux", "bin_grid.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "\n0 failed checks" in out.stdout
    # the rows reach every branch of the rule
    assert "m1 1 m2 1 k2 2" in out.stdout  # C2: 1 x 1/2
    assert "plane40 2e3" in out.stdout and "plane40 2e5" in out.stdout
    # tools/bin_order_sim.py keeps a copy of the rule for its `--grid rule`: the two agree on the square rows whose domain
    # starts on a centre of a pitch-1 lattice
    spec = importlib.util.spec_from_file_location("bin_order_sim", os.path.join(ROOT, "tools", "bin_order_sim.py"))
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    rows = {"C2": (999.0, 100000000), "C2 30 rays per disk": (999.0, 30000000), "plane40 2e3": (39.0, 2000),
            "plane40 2e4": (39.0, 20000), "plane40 2e5": (39.0, 200000)}
    for name, (ext, rays) in rows.items():
        m = re.search(r"^%s +aligned .*\(m1 (\d+) m2 (\d+) k2 (\d+)\)" % re.escape(name), out.stdout, flags=re.M)
        assert m, name
        assert sim.rule(ext, rays) == tuple(int(x) for x in m.groups()), (name, sim.rule(ext, rays), m.groups())
    assert sim.rule(99.0, 1000000, 16, 64) == (1, 1, 6) and sim.rule(99.0, 1000000, 40, 8) == (1, 1, 26)
