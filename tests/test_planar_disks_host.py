"""The planar-disk candidate tests (vr_planar_disks.hpp; pq_hit_packet PLANAR) on the host.  No GPU:
tests/aux/planar_disks.cpp restates hit_disc_uniform and local_disc_hit_uniform in plain float and compares them with the
header's per-round and per-candidate forms over more than 10^7 cases — plane heights +-0, 0.3, -7.25, both signs of s,
every axis, every sign pattern of the normal's zeros; zeros, denormals, origins on the plane, zero divisors, tiny
products, infinite and NaN origins mixed in — equal decisions everywhere, equal bits of t wherever the hit test accepts;
then the host's axis rule on a table of normals.  The same program runs once more built with AddressSanitizer and
UndefinedBehaviorSanitizer, stand-alone.  The header itself compiles alone: with the host compiler, and with hipcc for
the device, plain and with -DVR_DIAG, like the other role headers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "viennaray_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "aux", "planar_disks.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
HIPCC = os.environ.get("VR_HIPCC", "/opt/rocm/bin/hipcc")


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "\n0 failed checks" in out.stdout
    m = re.search(r"^(\d+) cases: (\d+) hit accepts, (\d+) neighbour accepts, (\d+) origins on the plane, (\d+) zero divisors, "
                  r"(\d+) tiny products, (\d+) non-finite origins$", out.stdout, flags=re.M)
    assert m, out.stdout
    cases, hits, locals_, on_plane, zero_div, tiny, nonfinite = (int(v) for v in m.groups())
    assert cases >= 10_000_000
    # (the comparison is about accepted hits as much as about refusals: both tests accept a fair share of the cases)
    assert hits >= cases // 50 and locals_ >= cases // 50, (cases, hits, locals_)
    assert min(on_plane, zero_div, tiny, nonfinite) >= cases // 100
    assert re.search(r"^12 normals of the axis table$", out.stdout, flags=re.M)
    return out


def test_planar_forms_equal_the_uniform_forms(tmp_path):
    exe = str(tmp_path / "planar_disks")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    _run(exe)


def test_planar_forms_under_sanitizers(tmp_path):
    """the same program with ASan and UBSan, run stand-alone (nothing is loaded into python)"""
    exe = str(tmp_path / "planar_disks_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]


def test_planar_header_is_plain_cxx(tmp_path):
    text = open(os.path.join(CSRC, "vr_planar_disks.hpp")).read()
    assert "float4" not in text and "threadIdx" not in text
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    unit = tmp_path / "only.cpp"
    unit.write_text('#include "vr_planar_disks.hpp"\n')
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I", CSRC, str(unit)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("define", [None, "-DVR_DIAG"])
def test_planar_header_stands_alone_on_the_device(define, tmp_path):
    assert os.path.isfile(HIPCC), "hipcc is needed: " + HIPCC
    unit = tmp_path / "only.hip"
    unit.write_text('#include "vr_planar_disks.hpp"\n')
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", "-I", CSRC, str(unit)]
    r = subprocess.run(cmd + ([define] if define else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_planar_header_is_a_module_source():
    """a run-time module is compiled from vr_trace.hip and what it includes: the Makefile names this header too"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    listed = re.findall(r"^MODEL_SRCS\s*:?=\s*(.*)$", text, flags=re.M)[0].split()
    assert "vr_planar_disks.hpp" in listed
