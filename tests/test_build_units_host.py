"""The library's dependency structure (csrc/Makefile), asked of `make -n` in a copy of the sources with empty files in place of the objects:
nothing is compiled.  One object per kernel set (odk_shapes.h: ODK_ENV_SET_<name>), so that a new robot compiles its own kernels alone and an
edit of the host code compiles no kernel."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_duck_playground_amd", "csrc")
SHIPPED_SETS = ["A", "B", "AE", "BE", "C", "D", "E"]
HOST_OBJECTS = ["odk_engine.o", "odk_model_load.o"]      # the translation units that include odk_shapes.h and are no kernel set
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
