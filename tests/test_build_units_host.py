"""The library's dependency structure (csrc/Makefile), asked of `make -n` in a copy of the sources with empty files in place of the objects:
nothing is compiled.  One object per kernel set (odk_shapes.h: ODK_ENV_SET_<name>), so that a new robot compiles its own kernels alone and an
edit of the host code compiles no kernel.  The env step's device code (odk_kernels.h) stands on layered headers: an edit of the physics
compiles the kernel sets alone, and every layer compiles as a translation unit of its own."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_duck_playground_amd", "csrc")
SHIPPED_SETS = ["A", "B", "AE", "BE", "C", "D", "E"]
HOST_OBJECTS = ["odk_engine.o", "odk_model_load.o"]      # the translation units that include odk_shapes.h and are no kernel set
LAYERS = ["odk_algebra.h", "odk_convex.h", "odk_lanes.h", "odk_shape.h"]   # odk_kernels.h includes these
PHYSICS_HEADERS = ["odk_kernels.h", "odk_algebra.h", "odk_convex.h"]     # the env step's device code and the layers that nothing else includes
HIPCC = "/opt/rocm/bin/hipcc"
USER_HEADER = ("#pragma once\nusing ShapeU0 = Shape<21, 20, 18, 14, 15, 148, 181, 76, 12, 18, false, 6, true>;\n#define ODK_ENV_SET_U0(X) X(ShapeU0, 32, 0)\n"
               "#define ODK_USER_SHAPES(X) X(4, ShapeU0)\n")


def outputs(tree, *args):
    """what `make -n libodk.so` would write: the -o operand of every command it prints"""
    p = subprocess.run(["make", "-C", os.path.join(tree, "open_duck_playground_amd", "csrc"), "-n", *args, "libodk.so"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return sorted(re.findall(r" -o (\S+)", p.stdout))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """the sources with one user shape added, and an up-to-date (empty) file for every product of a full build"""
    tree = str(tmp_path_factory.mktemp("units"))
    dst = os.path.join(tree, "open_duck_playground_amd", "csrc")
    os.makedirs(dst)
    os.makedirs(os.path.join(tree, "include"))
    shutil.copy(os.path.join(ROOT, "include", "odk.h"), os.path.join(tree, "include"))
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h")) and f != "odk_shapes_user.h" or f == "Makefile":
            shutil.copy(os.path.join(CSRC, f), dst)
    with open(os.path.join(dst, "odk_shapes_user.h"), "w") as f:
        f.write(USER_HEADER)
    products = outputs(tree)
    assert products == sorted([f"odk_env_{s}.o" for s in SHIPPED_SETS + ["U0"]] + HOST_OBJECTS + ["odk_reports.o", "odk_learner.o", "odk_mlp.o", "libodk.so"])
    for f in [p for p in products if p != "libodk.so"] + ["libodk.so"]:
        open(os.path.join(dst, f), "w").close()
    assert outputs(tree) == []
    return tree


def test_a_new_user_shape_compiles_its_own_kernel_set_and_the_host_objects(tree):
    # (odk_reports.o is not among them: the report kernels include no odk_shapes.h)
    assert outputs(tree, "-W", "odk_shapes_user.h") == sorted(["odk_env_U0.o"] + HOST_OBJECTS + ["libodk.so"])


def test_an_edit_of_the_model_loader_compiles_one_object(tree):
    assert outputs(tree, "-W", "odk_model_load.hip") == ["libodk.so", "odk_model_load.o"]


def test_an_edit_of_the_batch_api_compiles_no_env_kernel(tree):
    assert outputs(tree, "-W", "odk_engine.hip") == ["libodk.so", "odk_engine.o"]


def test_an_edit_of_the_reports_compiles_one_object(tree):
    assert outputs(tree, "-W", "odk_reports.hip") == ["libodk.so", "odk_reports.o"]


@pytest.mark.parametrize("header", PHYSICS_HEADERS)
def test_an_edit_of_the_physics_compiles_the_kernel_sets_alone(tree, header):
    # (not the batch API, the model loader or the report kernels)
    assert outputs(tree, "-W", header) == sorted([f"odk_env_{s}.o" for s in SHIPPED_SETS + ["U0"]] + ["libodk.so"])


def test_an_edit_of_the_lane_layer_also_compiles_the_reports(tree):
    assert outputs(tree, "-W", "odk_lanes.h") == sorted([f"odk_env_{s}.o" for s in SHIPPED_SETS + ["U0"]] + ["odk_reports.o", "libodk.so"])


def test_an_edit_of_the_shape_layer_also_compiles_the_host_objects(tree):
    assert outputs(tree, "-W", "odk_shape.h") == sorted([f"odk_env_{s}.o" for s in SHIPPED_SETS + ["U0"]] + HOST_OBJECTS + ["libodk.so"])


def test_the_device_code_includes_the_layers_and_only_the_env_kernels_include_it():
    src = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h")) and f != "odk_shapes_user.h"}
    assert set(re.findall(r'^#include "(\S+)"', src["odk_kernels.h"], re.M)) == set(LAYERS)
    assert [f for f, text in sorted(src.items()) if '#include "odk_kernels.h"' in text] == ["odk_env_kernels.h"]


@pytest.mark.parametrize("header", LAYERS + ["odk_kernels.h"])
def test_each_layer_stands_alone(tmp_path, header):
    """a translation unit that includes the one header and nothing else, through the host and the device pass (and the shape layer, the host code's,
    through the host pass alone as the model loader is compiled)"""
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc is needed to compile the layers")
    tu = os.path.join(str(tmp_path), "alone.hip")
    with open(tu, "w") as f:
        f.write(f'#include "{header}"\n')
    for extra in [[]] + ([["--cuda-host-only"]] if header == "odk_shape.h" else []):
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", *extra, "-I", CSRC, tu], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
