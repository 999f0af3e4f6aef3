"""The shipped rosdyn_amd/librdyn_hip.so is a release build, not a lab build (VERDICT r5 "What's weak" 6, task 5).

Diagnostic environment switches exist only behind -DRDYN_ENABLE_PROBES (rdyn_api_common.h): in the default build probe_env() ignores
its argument, so the NAMES of those switches do not even reach the object.  The only variables the product reads are the two of
rdyn_multi_gpu.cpp.  The tests read the built object's bytes: no process, no GPU."""
import os
import re

from conftest import ROOT

LIB = os.path.join(ROOT, "rosdyn_amd", "librdyn_hip.so")
CSRC = os.path.join(ROOT, "rosdyn_amd", "csrc")

# RDYN_* tokens of the object that are no environment names: RDYN_HIP_TRY (rdyn_api_common.h) puts the text of the failed call into
# the error message ("HIP error: ... (rdyn_launch_local_sweep(c->n_joints(), RDYN_MODE_TORQUE, a, stream))"), and these enumerators
# are spelled inside such calls.  token -> the files whose RDYN_HIP_TRY lines spell it.
ERROR_TEXT_TOKENS = {
    "RDYN_MODE_TORQUE": ("rdyn_api.cpp",),
    "RDYN_MODE_INERTIA": ("rdyn_api_dynamics.cpp",),
    "RDYN_MODE_REGRESSOR": ("rdyn_api.cpp",),
    "RDYN_MODE_REGRESSOR_GRAM": ("rdyn_api_gram.cpp",),
    "RDYN_ADJ_OP_INIT": ("rdyn_api_dynamics.cpp",),
    "RDYN_ADJ_OP_ZERO": ("rdyn_api_dynamics.cpp",),
    "RDYN_ADJ_OP_OUT": ("rdyn_api_dynamics.cpp",),
    "RDYN_ADJ_OP_ADD_SEED": ("rdyn_api_dynamics.cpp",),
    "RDYN_ADJ_OP_EULER_PRE": ("rdyn_api_dynamics.cpp",),
    "RDYN_ADJ_OP_EULER_POST": ("rdyn_api_dynamics.cpp",),
    "RDYN_ADJ_OP_RK4_PRE": ("rdyn_api_dynamics.cpp",),
    "RDYN_ADJ_OP_RK4_SEED": ("rdyn_api_dynamics.cpp",),
    "RDYN_ADJ_OP_RK4_FWD": ("rdyn_api_dynamics.cpp",),
    "RDYN_ADJ_OP_RK4_POST": ("rdyn_api_dynamics.cpp",),
    "RDYN_ADJ_OP_RK4_END": ("rdyn_api_dynamics.cpp",),
}


def _object_bytes():
    with open(LIB, "rb") as f:
        return f.read()


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_object_names_no_environment_switch_but_the_documented_two():
    documented = set(re.findall(r'getenv\("(RDYN_[A-Z0-9_]+)"\)', _source("rdyn_multi_gpu.cpp")))
    assert documented == {"RDYN_RCCL_PATH", "RDYN_TEST_ALIAS_DEVICES"}
    tokens = {t.decode() for t in re.findall(rb"RDYN_[A-Z0-9_]+", _object_bytes())}
    assert documented <= tokens  # the search does see names that are there
    assert tokens - documented <= set(ERROR_TEXT_TOKENS), sorted(tokens - documented - set(ERROR_TEXT_TOKENS))
    # the listed exceptions are what the table says they are: arguments inside an RDYN_HIP_TRY(...) of the file named
    for token, files in ERROR_TEXT_TOKENS.items():
        for name in files:
            assert re.search(r"RDYN_HIP_TRY\([^;]*\b%s\b" % token, _source(name)), (token, name)


def test_the_retired_gram_kernels_are_not_in_the_object():
    """The single-wave pipelined and LDS-tile regressor->Gram kernels, which no shipped route reached, are gone from the product: their
    names appear nowhere (host symbol table, kernel registration, the embedded gfx950 code object), while the kernel that serves
    their range does."""
    blob = _object_bytes()
    assert blob.count(b"k_regressor_gram_duo") > 0
    assert blob.count(b"k_regressor_gram_pipe") == 0
    assert blob.count(b"k_regressor_gram_lds") == 0
