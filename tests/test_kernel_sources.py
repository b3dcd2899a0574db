"""The files a run-time module is compiled from are named once, in the Makefile (MODEL_SRCS): the list covers everything
vr_trace.hip can include, and vr_models.cpp carries no list of its own (no GPU, no compiler)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "viennaray_amd", "csrc")
# the role headers behind the umbrella vr_device.hpp (its comment has the map)
ROLE_HEADERS = ["vr_frame.hpp", "vr_math.hpp", "vr_diag_macros.hpp", "vr_rng.hpp", "vr_intersect.hpp", "vr_walk.hpp",
                "vr_packet_query.hpp"]
HIPCC = os.environ.get("VR_HIPCC", "/opt/rocm/bin/hipcc")


def _model_srcs():
    text = open(os.path.join(CSRC, "Makefile")).read()
    m = re.findall(r"^MODEL_SRCS\s*:?=\s*(.*)$", text, flags=re.M)
    assert len(m) == 1, "the Makefile names the module sources once"
    return text, m[0].split()


def _reached(start):
    """every file a quoted #include "vr_*.hpp" leads to from `start`, whatever preprocessor branch it stands in: a superset
    of what any one module reads"""
    seen, todo = set(), [start]
    while todo:
        fn = todo.pop()
        if fn in seen:
            continue
        seen.add(fn)
        todo += re.findall(r'^\s*#\s*include\s+"(vr_\w+\.hpp)"', open(os.path.join(CSRC, fn)).read(), flags=re.M)
    return seen


def test_module_source_list_covers_every_include():
    makefile, listed = _model_srcs()
    reached = _reached("vr_trace.hip")
    assert {"vr_trace.hip", "vr_generate.hpp", "vr_trace_kernel.hpp", "vr_modules.hpp", "vr_device.hpp", "vr_types.hpp"} <= reached
    assert set(ROLE_HEADERS) <= reached
    assert reached <= set(listed), sorted(reached - set(listed))
    assert len(set(listed)) == len(listed)
    for fn in listed:
        assert os.path.isfile(os.path.join(CSRC, fn)), fn
    # the checksum and the list vr_models.cpp reads both come from that variable
    assert re.search(r"^SRC_CKSUM\s*:?=.*\$\(MODEL_SRCS\)", makefile, flags=re.M)
    assert "-DVR_MODEL_SRCS='\"$(MODEL_SRCS)\"'" in makefile


def test_models_cpp_has_no_source_list_of_its_own():
    text = open(os.path.join(CSRC, "vr_models.cpp")).read()
    text = re.sub(r"//[^\n]*", "", text)
    for init in re.findall(r"\{[^{};]*\}", text):
        # (a whole file name; the suffixes "_model.hpp" / "_source.hpp" of the caller's text in the cache are none)
        for quoted in re.findall(r'"([^"]*)"', init):
            assert not re.fullmatch(r"[A-Za-z]\w*\.(hip|hpp)", quoted), init
    assert "VR_MODEL_SRCS" in text


@pytest.mark.parametrize("define", [None, "-DVR_DIAG"])
@pytest.mark.parametrize("header", ROLE_HEADERS + ["vr_device.hpp", "vr_kernel_table.hpp"])
def test_device_header_stands_alone(header, define, tmp_path):
    """each role header, the umbrella, and the kernel table's header compiles as the only include of an otherwise empty .hip file"""
    assert os.path.isfile(HIPCC), "hipcc is needed: " + HIPCC
    unit = tmp_path / "only.hip"
    unit.write_text('#include "%s"\n' % header)
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", "-I", CSRC, str(unit)]
    r = subprocess.run(cmd + ([define] if define else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_frame_header_is_plain_cxx(tmp_path):
    """vr_frame.hpp is what host code reads of the device side: the host compiler alone takes it, no HIP in its text"""
    text = open(os.path.join(CSRC, "vr_frame.hpp")).read()
    assert "__device__" not in text and "hip_runtime" not in text
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    unit = tmp_path / "only.cpp"
    unit.write_text('#include "vr_frame.hpp"\n')
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", CSRC, str(unit)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_device_header_is_only_the_umbrella():
    """vr_device.hpp defines nothing: without its comments it is '#pragma once' and the includes of the role headers"""
    text = open(os.path.join(CSRC, "vr_device.hpp")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lines = [l.strip() for l in re.sub(r"//[^\n]*", "", text).split("\n") if l.strip()]
    assert lines[0] == "#pragma once"
    included = []
    for l in lines[1:]:
        m = re.fullmatch(r'#include "(vr_\w+\.hpp)"', l)
        assert m, l
        included.append(m.group(1))
    assert sorted(included) == sorted(ROLE_HEADERS)
