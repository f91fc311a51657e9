"""Which compiled env-kernel instantiation is held to the float64 oracle by which GPU test -- as a table, checked without a GPU.

csrc/odk_shapes.h lists the instantiations (`#define ODK_ENV_SET_<name>(X) X(Shape, lanes per env, HF) ...`; the Makefile reads the same lines).
Each one is three launches: the physics kernel (`Batch.physics_step`), the reset kernel and the env-step kernel.  MATRIX gives, per instantiation
and launch, either the tests that compare that launch's outputs with the oracle -- (module, function, parameter tuple or None) -- or one line
saying why it is not judged.  The 64-lane kernels of the two duck models once sat in this table with reasons where tests belong
(profiles/lanes64/NOTES.md); an instantiation added to odk_shapes.h without a row here fails `test_every_instantiation_has_a_row`.

Which launch a test reaches follows odk_engine.hip `launch()`: shape by the model (0 flat_terrain: A, 1 the backlash models: B, tail_biped: C,
biped12: D, biped_arms: E), the cone variants (AE / BE) for `opt_cone = 1` on the duck, HF 1 / 2 for a height field under hull / primitive feet,
64 lanes only when asked for AND the model is the duck on a plane floor with pyramidal cones -- which is why every 64-lane case asserts
`lanes_per_env == 64` on its batch.  This module reads source text for the instantiation names only."""
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_duck_playground_amd", "csrc")

P, E, C, F, A = "test_gpu_parity", "test_gpu_env", "test_gpu_commands", "test_gpu_four_chains", "test_gpu_api"
FT, FB, RB = "flat_terrain", "flat_terrain_backlash", "rough_terrain_backlash"
TAIL, B12 = ("tail_biped.xml", 15, 107, 221), ("biped12.xml", 12, 89, 194)


def _duck_physics(task, lanes):
    """the physics launch of a duck model on its own floor at `lanes`"""
    t = [(P, "test_one_substep_stages", (task, lanes)), (P, "test_differential_sweep", (task, lanes)),
         (P, "test_env_step_ten_substeps", (task,)), (P, "test_env_step_ten_substeps_on_rollout_states", (task,))]      # (the flat tasks: both lane counts in one test)
    return t + ([(P, "test_foot_foot_contacts", (task, lanes))] if task != RB else [])


def _duck_reset(task, lanes):
    return [(E, "test_reset_matches_oracle", (task, lanes)), (E, "test_standing_env_matches_oracle", (task, lanes)), (E, "test_env_step_with_domain_randomisation", (task, False, lanes))]


def _duck_step(task, lanes):
    return [(E, "test_step_sequence_with_resync", (task, lanes)), (E, "test_standing_env_matches_oracle", (task, lanes)), (E, "test_env_step_with_domain_randomisation", (task, False, lanes)),
            (E, "test_in_step_command_resample", (task, lanes))]


NO_DIRECT_RESET = "no reset comparison of its own: the reset kernel's first observation is judged where the auto-reset of the step test hands it back"

MATRIX = {
    ("ShapeA", 32, 0): dict(physics=_duck_physics(FT, 32), reset=_duck_reset(FT, 0), step=_duck_step(FT, 0) + [(C, "test_bound_commands_match_the_oracle_env", (FT, False, 0))]),
    ("ShapeA", 64, 0): dict(physics=_duck_physics(FT, 64), reset=_duck_reset(FT, 64), step=_duck_step(FT, 64)),
    ("ShapeB", 32, 0): dict(physics=_duck_physics(FB, 32), reset=_duck_reset(FB, 0), step=_duck_step(FB, 0) + [(C, "test_bound_commands_match_the_oracle_env", (FB, False, 0))]),
    ("ShapeB", 64, 0): dict(physics=_duck_physics(FB, 64), reset=_duck_reset(FB, 64), step=_duck_step(FB, 64) + [(C, "test_bound_commands_match_the_oracle_env", (FB, False, 64))]),
    # hull feet on the height field: no Joystick reset test of its own, the reset observations are judged by the Standing and the randomisation test
    ("ShapeB", 32, 1): dict(physics=_duck_physics(RB, 32) + [(P, "test_height_field_far_from_the_origin", None), (P, "test_height_field_lists_shared_across_the_wave", None)],
                            reset=[(E, "test_standing_env_matches_oracle", (RB, 0)), (E, "test_env_step_with_domain_randomisation", (RB, False, 0))],
                            step=[(E, "test_step_sequence_with_resync", (RB, 0)), (E, "test_standing_env_matches_oracle", (RB, 0)), (E, "test_env_step_with_domain_randomisation", (RB, False, 0))]),
    # sphere / capsule feet on the height field: no shipped task has them
    ("ShapeB", 32, 2): dict(physics=[(P, "test_primitive_feet_on_a_height_field", (k,)) for k in (("sphere", "sphere"), ("capsule", "capsule"), ("capsule", "sphere"))],
                            reset="reachable only from test-built model variants (primitive feet on a height field); run from NaN-filled LDS, not against the oracle",
                            step="reachable only from test-built model variants (primitive feet on a height field); run from NaN-filled LDS, not against the oracle"),
    # the duck with elliptic cones
    ("ShapeAE", 32, 0): dict(physics=[(P, "test_the_duck_with_elliptic_cones", (FT,))], reset=NO_DIRECT_RESET, step=[(E, "test_step_sequence_of_the_duck_with_elliptic_cones", (FT,))]),
    ("ShapeBE", 32, 0): dict(physics=[(P, "test_the_duck_with_elliptic_cones", (FB,))], reset=NO_DIRECT_RESET, step=[(E, "test_step_sequence_of_the_duck_with_elliptic_cones", (FB,))]),
    ("ShapeBE", 32, 1): dict(physics=[(P, "test_the_duck_with_elliptic_cones", (RB,))], reset=NO_DIRECT_RESET, step=[(E, "test_step_sequence_of_the_duck_with_elliptic_cones", (RB,))]),
    # robots that are not the duck
    ("ShapeC", 32, 0): dict(physics=[(P, "test_a_robot_that_is_not_the_duck", None)], reset=[(E, "test_reset_of_a_robot_that_is_not_the_duck", TAIL)],
                            step=[(E, "test_step_sequence_of_a_robot_that_is_not_the_duck", TAIL)]),
    ("ShapeD", 32, 0): dict(physics=[(P, "test_a_biped_with_six_dof_legs", None)], reset=[(E, "test_reset_of_a_robot_that_is_not_the_duck", B12)],
                            step=[(E, "test_step_sequence_of_a_robot_that_is_not_the_duck", B12), (E, "test_a_robot_that_is_not_the_duck_with_domain_randomisation_and_command_resampling", None)]),
    ("ShapeE", 32, 0): dict(physics=[(F, "test_a_biped_with_arms_through_the_physics_kernels", ("biped_arms.xml",))], reset=[(F, "test_env_steps_of_a_biped_with_arms", None)],
                            step=[(F, "test_env_steps_of_a_biped_with_arms", None)]),
}
LAUNCHES = ("physics", "reset", "step")


def compiled_instantiations(text):
    """[(shape, lanes, HF)] of the `#define ODK_ENV_SET_<name>(X) ...` lines of odk_shapes.h (the pattern the Makefile's `set_names` uses)"""
    out = []
    for line in text.split("\n"):
        m = re.match(r"^#define ODK_ENV_SET_([A-Za-z0-9]*)\(X\)(.*)", line)
        if m:
            inst = [(s, int(g), int(hf)) for s, g, hf in re.findall(r"X\((\w+), (\d+), (\d+)\)", m.group(2))]
            assert inst, line
            out += inst
    return out


def _param_tuples(fn):
    """every parameter tuple of a test function, from its `parametrize` marks (one mark per function in these modules), or None"""
    marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
    if not marks:
        return None
    assert len(marks) == 1, fn.__name__
    names, values = marks[0].args[0], marks[0].args[1]
    single = isinstance(names, str) and "," not in names
    out = set()
    for v in values:
        v = getattr(v, "values", v)      # (pytest.param(...))
        out.add((v,) if single and not hasattr(v, "_fields") else tuple(v))
    return out


def table_problems(matrix, triples):
    """what is wrong with `matrix` for the compiled `triples`: a list of strings, empty when it is in order"""
    bad = []
    if set(matrix) != set(triples) or len(triples) != len(set(triples)):
        bad.append(f"rows and instantiations differ: without a row {sorted(set(triples) - set(matrix))}, rows of nothing compiled {sorted(set(matrix) - set(triples))}")
    for triple, row in matrix.items():
        if set(row) != set(LAUNCHES):
            bad.append(f"{triple}: cells {sorted(row)}")
            continue
        for launch in LAUNCHES:
            cell = row[launch]
            if isinstance(cell, str):
                if len(cell) < 20 or "\n" in cell:
                    bad.append(f"{triple} {launch}: a reason is one line that says something")
                continue
            if not cell:
                bad.append(f"{triple} {launch}: neither a test nor a reason")
            for module, name, params in cell:
                fn = getattr(importlib.import_module(module), name, None)
                if not callable(fn):
                    bad.append(f"{triple} {launch}: no function {module}.{name}")
                    continue
                have = _param_tuples(fn)
                if (params is None) != (have is None):
                    bad.append(f"{triple} {launch}: {module}.{name} is {'not ' if have is None else ''}parametrised")
                elif params is not None and tuple(params) not in have:
                    bad.append(f"{triple} {launch}: {module}.{name} has no case {params}")
    return bad


def _triples():
    return compiled_instantiations(open(os.path.join(CSRC, "odk_shapes.h")).read())


def test_every_instantiation_has_a_row():
    triples = _triples()
    assert len(triples) == 12 and ("ShapeA", 64, 0) in triples and ("ShapeB", 64, 0) in triples, triples
    assert set(MATRIX) == set(triples), (sorted(set(triples) - set(MATRIX)), sorted(set(MATRIX) - set(triples)))


def test_every_named_test_and_case_exists():
    assert table_problems(MATRIX, _triples()) == []


def test_the_64_lane_kernels_of_both_duck_models_are_judged_in_every_cell():
    for triple in (("ShapeA", 64, 0), ("ShapeB", 64, 0)):
        for launch in LAUNCHES:
            cell = MATRIX[triple][launch]
            assert isinstance(cell, list) and cell, (triple, launch)
            for module, name, params in cell:
                assert 64 in params or name.startswith("test_env_step_ten_substeps"), (triple, launch, name, params)      # (ten substeps: both lane counts inside one test)
    from test_gpu_parity import LANES64_TASKS
    assert LANES64_TASKS == (FT, FB)


def test_the_check_notices_a_missing_row_a_missing_case_and_a_new_instantiation():
    triples = _triples()
    less = {k: v for k, v in MATRIX.items() if k != ("ShapeB", 64, 0)}
    assert any("without a row [('ShapeB', 64, 0)]" in p for p in table_problems(less, triples))
    wrong = dict(MATRIX)
    wrong["ShapeB", 64, 0] = dict(MATRIX["ShapeB", 64, 0], reset=[(E, "test_reset_matches_oracle", (RB, 64))])
    assert table_problems(wrong, triples) == ["('ShapeB', 64, 0) reset: test_gpu_env.test_reset_matches_oracle has no case ('rough_terrain_backlash', 64)"]
    wrong["ShapeB", 64, 0] = dict(MATRIX["ShapeB", 64, 0], step=[(E, "test_no_such_test", None)], physics=[])
    assert len(table_problems(wrong, triples)) == 2
    more = compiled_instantiations("#define ODK_ENV_SET_A(X) X(ShapeA, 32, 0) X(ShapeA, 64, 0)\n#define ODK_ENV_SET_C(X) X(ShapeC, 32, 0) X(ShapeC, 64, 0)\nusing x = int;\n")
    assert more == [("ShapeA", 32, 0), ("ShapeA", 64, 0), ("ShapeC", 32, 0), ("ShapeC", 64, 0)]
    assert any("without a row [('ShapeC', 64, 0)]" in p for p in table_problems(MATRIX, triples + [("ShapeC", 64, 0)]))
