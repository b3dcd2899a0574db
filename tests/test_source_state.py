"""RaySource (viennaray_amd/csrc/vr_source.hpp), the ray source in force, without a device: tests/aux/source_state.cpp
includes the header alone and walks it from each of the five kinds through every setter and every clearing call; the kind,
the other kinds' payload, the ray counts and the answers of the named questions are asserted there against tables written
out in the program.  Built as the other tests/aux programs are, and once more with the address and undefined-behaviour
sanitizers (a stand-alone host program: nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "aux", "source_state.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_source_state_transitions_and_questions(tmp_path, flags):
    exe = str(tmp_path / "source_state")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "source state ok: 1440 steps" in out.stdout


def test_source_header_needs_no_hip_header():
    """the header and what it includes stay host code: no HIP include, so that the program above compiles it alone"""
    csrc = os.path.join(ROOT, "viennaray_amd", "csrc")
    for name in ("vr_source.hpp", "vr_types.hpp"):
        text = open(os.path.join(csrc, name)).read()
        assert "hip/" not in text, name
