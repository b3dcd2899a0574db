"""The files a run-time module is compiled from are named once, in the Makefile (MODEL_SRCS): the list covers everything
vr_trace.hip can include, and vr_models.cpp carries no list of its own (no GPU, no compiler)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "viennaray_amd", "csrc")


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
