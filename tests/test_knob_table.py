"""The knob table (viennaray_amd/csrc: struct Knobs in vr_context.hpp, read_knobs in vr_knobs.cpp).

Every tuning or experiment switch of the library is read from the environment in read_knobs and nowhere else, and every
switch the tests set is one read_knobs reads: a switch that a change silently dropped would leave the tests that set it
passing without testing anything.  (No GPU: these read the sources.)"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "viennaray_amd", "csrc")
# configuration of vr_register_particle_model (where the kernel sources, the compiler and the code-object cache are),
# read where a model is registered: not a knob
CONFIG_NAMES = {"VR_CSRC_DIR", "VR_HIPCC", "VR_CACHE_DIR", "XDG_CACHE_HOME", "HOME"}
# variables the tests hand to subprocesses of their own
SUBPROCESS_NAMES = {"VR_ROOT", "VR_ID_FILE", "VR_OUT"}


def _sources():
    for ext in ("cpp", "hpp", "hip"):
        for path in sorted(glob.glob(os.path.join(CSRC, "*." + ext))):
            with open(path) as f:
                yield path, f.read()


def _read_knobs_body():
    with open(os.path.join(CSRC, "vr_knobs.cpp")) as f:
        text = f.read()
    start = text.index("{", text.index("Knobs read_knobs()"))
    depth = 0
    for k in range(start, len(text)):
        depth += {"{": 1, "}": -1}.get(text[k], 0)
        if depth == 0:
            return text[start:k + 1]
    raise AssertionError("read_knobs has no closing brace")


def _names_the_tests_set():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "tests", "*.py")):
        if os.path.samefile(path, __file__):
            continue
        with open(path) as f:
            text = f.read()
        names.update(re.findall(r'setenv\(\s*"(VR_[A-Z0-9_]+)"', text))             # monkeypatch.setenv("VR_X", ...)
        names.update(re.findall(r'"(VR_[A-Z0-9_]+)"\s*:', text))                    # knob dicts: {"VR_X": "1"}
        names.update(re.findall(r'\[\s*"(VR_[A-Z0-9_]+)"\s*\]\s*=[^=]', text))      # env["VR_X"] = ...
    return names - CONFIG_NAMES - SUBPROCESS_NAMES


def test_getenv_only_in_read_knobs_and_model_registration():
    body = _read_knobs_body()
    for name in re.findall(r"getenv\s*\(([^)]*)\)", body):
        assert re.fullmatch(r'"VR_[A-Z0-9_]+"', name.strip()), f"read_knobs reads getenv({name}): a literal VR_ name expected"
    for path, text in _sources():
        if os.path.basename(path) == "vr_knobs.cpp":
            text = text.replace(body, "")
        for arg in re.findall(r"getenv\s*\(([^)]*)\)", text):
            lit = re.fullmatch(r'"([A-Za-z0-9_]+)"', arg.strip())
            assert lit and lit.group(1) in CONFIG_NAMES, \
                f"{os.path.basename(path)}: getenv({arg}) outside read_knobs (tuning switches belong in struct Knobs)"


def test_every_knob_the_tests_set_is_read_by_read_knobs():
    read = set(re.findall(r'getenv\("(VR_[A-Z0-9_]+)"\)', _read_knobs_body()))
    names = _names_the_tests_set()
    assert len(names) >= 30, sorted(names)  # (the scan found the knob tables of tests/test_gpu_parity.py)
    missing = sorted(names - read)
    assert not missing, f"set by the tests but not read by read_knobs: {missing}"
