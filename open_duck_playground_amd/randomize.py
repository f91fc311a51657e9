"""Domain randomization (host mirror of reference playground/common/randomize.py:26-146).

`domain_randomize(model, rng, num_envs)` samples, once per env for the whole run, the same fields
with the same distributions as the reference and returns them with an `in_axes`-style dict that
names the batched fields.  `apply(batch, fields)` hands them to the engine (odk_batch_set_param).

Bug-compatibility kept on purpose:
  * FLOOR_GEOM_ID = 0 is a visual trunk mesh, so the sampled friction has no physical effect: it is
    returned but not sent to the engine;
  * TORSO_BODY_ID = 1 is the massless `base` body: its ipos is jittered and its mass becomes
    0 * U(0.9,1.1) + U(-0.1,0.1), which can be negative; inertias and invweights are not updated.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from . import engine
from .model import Model

FLOOR_GEOM_ID = 0
TORSO_BODY_ID = 1


def domain_randomize(model: Model, rng: np.random.Generator, num_envs: int) -> Tuple[Dict[str, np.ndarray], Dict[str, int]]:
    a = model.a
    nu, nbody = model.nu, model.nbody
    act_jnt = np.asarray(a["actuator_trnid"])
    dof_addr = np.asarray(a["jnt_dofadr"])[act_jnt]          # dofs with frictionloss (backlash joints have none)
    joint_addr = np.asarray(a["jnt_qposadr"])[act_jnt]
    U = lambda lo, hi, shape: rng.uniform(lo, hi, size=(num_envs,) + shape)
    geom_friction0 = U(0.5, 1.0, ())                                              # randomize.py:42-45 (no-op geom)
    frictionloss = np.asarray(a["dof_frictionloss"])[dof_addr][None] * U(0.9, 1.1, (nu,))   # :48-52
    armature = np.asarray(a["dof_armature"])[dof_addr][None] * U(1.0, 1.05, (nu,))          # :55-59
    dpos = U(-0.05, 0.05, (3,))                                                    # :62-66
    body_ipos_torso = np.asarray(a["body_ipos"])[TORSO_BODY_ID][None] + dpos
    body_mass = np.asarray(a["body_mass"])[None] * U(0.9, 1.1, (nbody,))           # :69-71
    body_mass[:, TORSO_BODY_ID] += U(-0.1, 0.1, ())                                # :74-76
    qpos0 = np.asarray(a["qpos0"])[joint_addr][None] + U(-0.03, 0.03, (nu,))       # :79-86
    factor = U(0.9, 1.1, (nu,))                                                    # :89-95
    kp = np.asarray(a["actuator_gainprm0"])[None] * factor
    fields = {
        "geom_friction": geom_friction0, "body_ipos": body_ipos_torso, "dof_frictionloss": frictionloss, "dof_armature": armature,
        "body_mass": body_mass, "qpos0": qpos0, "actuator_gainprm": kp, "actuator_biasprm": -kp,
    }
    in_axes = {k: 0 for k in fields}   # every returned field is batched over envs (randomize.py:119-131)
    return fields, in_axes


def nominal_fields(model: Model, num_envs: int) -> Dict[str, np.ndarray]:
    """The model's own values in `domain_randomize`'s layout (float64 [num_envs, ...], without the no-op geom friction): what `apply` hands
    the engine for a plant that differs from the XML in nothing.  `scale_fields` builds a controlled plant on top of it."""
    a = model.a
    act_jnt = np.asarray(a["actuator_trnid"])
    dof_addr = np.asarray(a["jnt_dofadr"])[act_jnt]
    joint_addr = np.asarray(a["jnt_qposadr"])[act_jnt]
    kp = np.asarray(a["actuator_gainprm0"], np.float64)
    one = lambda v: np.repeat(np.asarray(v, np.float64).reshape(1, -1), int(num_envs), axis=0)
    return {"body_ipos": one(np.asarray(a["body_ipos"])[TORSO_BODY_ID]), "dof_frictionloss": one(np.asarray(a["dof_frictionloss"])[dof_addr]),
            "dof_armature": one(np.asarray(a["dof_armature"])[dof_addr]), "body_mass": one(a["body_mass"]),
            "qpos0": one(np.asarray(a["qpos0"])[joint_addr]), "actuator_gainprm": one(kp), "actuator_biasprm": one(-kp)}


# a plant's scale axes -> the fields they multiply (kp: gain and bias together, as `apply` hands the engine the gain alone and the kernels take
# the bias from it; mass: the body masses alone -- inertias are not rescaled, randomize.py's semantics)
SCALED_FIELDS = {"kp": ("actuator_gainprm", "actuator_biasprm"), "mass": ("body_mass",), "frictionloss": ("dof_frictionloss",),
                 "armature": ("dof_armature",)}


def scale_fields(fields: Dict[str, np.ndarray], scales: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """`fields` (nominal_fields or domain_randomize) with env e's row of every field of axis k multiplied by scales[k][e]; the other fields
    (body_ipos, qpos0) are passed on.  The product is taken in float64 and rounded to float32 once, by `Batch.set_param`: a scale of exactly 1
    leaves the float32 value the engine's own model holds."""
    out = {k: np.array(v, np.float64) for k, v in fields.items()}
    for axis, scale in scales.items():
        if axis not in SCALED_FIELDS:
            raise ValueError(f"unknown plant scale {axis!r} (one of {', '.join(SCALED_FIELDS)})")
        sc = np.asarray(scale, np.float64).reshape(-1)
        for k in SCALED_FIELDS[axis]:
            out[k] = out[k] * sc.reshape((-1,) + (1,) * (out[k].ndim - 1))
    return out


def apply(batch: "engine.Batch", fields: Dict[str, np.ndarray]) -> None:
    batch.set_param(engine.PARAM_BODY_MASS, fields["body_mass"])
    batch.set_param(engine.PARAM_BODY_IPOS_TORSO, fields["body_ipos"])
    batch.set_param(engine.PARAM_DOF_FRICTIONLOSS, fields["dof_frictionloss"])
    batch.set_param(engine.PARAM_DOF_ARMATURE, fields["dof_armature"])
    batch.set_param(engine.PARAM_QPOS0, fields["qpos0"])
    batch.set_param(engine.PARAM_KP, fields["actuator_gainprm"])
