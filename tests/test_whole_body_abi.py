"""include/drm_hip_whole_body.h, backend.WHOLE_BODY_PROTOTYPES and csrc/drm_args_whole_body.hpp, held to one another the way
tests/test_host_logic.py and tests/test_abi_refusals.py hold include/drm_hip.h, backend.PROTOTYPES and csrc/drm_args.hpp: the header's
names are the table's and both libraries export them; each row of the table below, one fault in an otherwise valid call of B = 0 rows on
the 2-link robot, is refused by libdrm_cpu.so and libdrm_hip.so with the same code and the same drm_last_error() (the host library
first, the HIP library only once the host library has refused: nothing here can launch a kernel, and no device is needed); every
fail() literal of the new argument header is the error of at least one row.  The addition leaves backend.EXPORTS and the ABI version
as they were."""
import ctypes
import os
import re

import pytest

from differentiable_robot_model_amd import backend
from test_abi_refusals import BATCH, BUF, INVALID, NAN, INF, NO_OPS, TREE, WALK_FAULTS, Call, Struct, nulls, on, refused, walks  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drm_hip_whole_body.h")
ARGS = os.path.join(os.path.dirname(os.path.abspath(backend.__file__)), "csrc", "drm_args_whole_body.hpp")
NAME = "drm_whole_body"
OUTPUTS = ("com", "com_vel", "com_acc", "com_jac", "ang_mom", "force", "moment")

BASE = Struct(backend.DrmBaseShare, mass=1.0, mc=(0.0, 0.0, 0.5))
BASELINE = dict(w=TREE, q=BUF, qd=BUF, qdd=BUF, B=0, flags=1, base=BASE, com=BUF, com_vel=BUF, com_acc=BUF, com_jac=BUF, ang_mom=BUF,
                force=BUF, moment=BUF, scratch=None, stream=None)
ROWS = on("w", TREE, NO_OPS) + nulls("q", "q must not be NULL") + BATCH + [
    ({k: None for k in OUTPUTS}, INVALID, "every output is NULL"),
    (dict(qd=None), INVALID, "com_vel / com_acc / ang_mom need qd"),
    (dict(qd=None, com_vel=None, ang_mom=None), INVALID, "com_vel / com_acc / ang_mom need qd"),
    (dict(qd=None, com_vel=None, com_acc=None), INVALID, "com_vel / com_acc / ang_mom need qd"),
    (dict(base=BASE(mass=-1.0)), INVALID, "the base share must be finite and its mass >= 0"),
    (dict(base=BASE(mass=NAN)), INVALID, "the base share must be finite and its mass >= 0"),
    (dict(base=BASE(mc=(0.0, INF, 0.0))), INVALID, "the base share must be finite and its mass >= 0"),
    (dict(w=None), INVALID, "walk is NULL")] + on("w", TREE, *WALK_FAULTS)
# calls that stand: no base share; the wrench and the positions alone need neither qd nor qdd
VALID = [dict(base=None), dict(qd=None, qdd=None, com_vel=None, com_acc=None, ang_mom=None), dict(qdd=None), dict(base=BASE(mass=0.0))]


def test_the_header_the_table_and_the_libraries_name_the_same_entry_points():
    header = open(HEADER).read()
    declared = set(re.findall(r"\b(drm_[a-z_]+)\s*\(", header))
    assert declared == set(backend.WHOLE_BODY_PROTOTYPES) == {NAME, NAME + "_scratch_floats", NAME + "_scratch_floats_aligned"}
    for path in (backend.LIB_PATH, backend.CPU_LIB_PATH):
        assert os.path.exists(path), "run `python __graft_entry__.py build` first"
        lib = ctypes.CDLL(path)
        for sym in declared:
            assert hasattr(lib, sym), (path, sym)
    assert int(re.search(r"#define DRM_WHOLE_BODY_COMPOSED (\d+)", header).group(1)) == backend.WHOLE_BODY_COMPOSED
    # its flag is a bit of its own
    main = open(os.path.join(ROOT, "include", "drm_hip.h")).read()
    taken = {int(v) for v in re.findall(r"#define DRM_[A-Z]+_COMPOSED (\d+)", main)} | {1, 2, 4}
    assert backend.WHOLE_BODY_COMPOSED not in taken and bin(backend.WHOLE_BODY_COMPOSED).count("1") == 1


def test_the_addition_leaves_the_main_table_and_the_version_alone():
    assert not set(backend.WHOLE_BODY_PROTOTYPES) & set(backend.EXPORTS)
    assert tuple(backend.PROTOTYPES) == backend.EXPORTS
    for lib in (backend.load_library(kind="cpu"), backend.load_library()):
        assert lib.drm_abi_version() == backend.ABI_VERSION == 15
    assert "DRM_ABI_VERSION" not in re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    # load_library declares the new prototypes too
    fn = getattr(backend.load_library(kind="cpu"), NAME)
    assert fn.argtypes == backend.WHOLE_BODY_PROTOTYPES[NAME][1] and len(fn.argtypes) == len(BASELINE)


def test_both_libraries_refuse_the_same_calls_with_the_same_words(walks):
    host, hip = backend.load_library(kind="cpu"), backend.load_library()
    for changes in [{}] + VALID:
        call = Call(walks, dict(BASELINE, **changes))
        assert refused(host, NAME, call)[0] == 0, (changes, host.drm_last_error())
        assert refused(hip, NAME, call)[0] == 0, (changes, hip.drm_last_error())
    for changes, code, message in ROWS:
        assert set(changes) <= set(BASELINE), changes
        call = Call(walks, dict(BASELINE, **changes))
        rc, said = refused(host, NAME, call)
        assert rc == code and message.encode() in said, (changes, rc, said)
        assert refused(hip, NAME, call) == (rc, said), (changes, rc, said)      # (only a call the host library refused gets here)
    # the queries answer 0 for a walk they cannot size, and for the 2-link robot, whose records fit
    for lib in (host, hip):
        for query in (lib.drm_whole_body_scratch_floats, lib.drm_whole_body_scratch_floats_aligned):
            assert query(None, 64) == 0 and query(ctypes.byref(walks["tree"][0]), 64) == 0


def test_the_table_hits_every_refusal_of_the_new_header(walks):
    """Every message of csrc/drm_args_whole_body.hpp is the whole drm_last_error() of at least one row."""
    source = re.sub(r"//[^\n]*", "", open(ARGS).read())
    literals = {"".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1)))
                for m in re.finditer(r'\bfail\(\s*DRM_ERR_\w+,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', source)}
    assert len(literals) == 5, literals      # (the pattern still finds them)
    host = backend.load_library(kind="cpu")
    said = {refused(host, NAME, Call(walks, dict(BASELINE, **changes)))[1].decode() for changes, _, _ in ROWS}
    for literal in literals:
        assert literal in said, literal
