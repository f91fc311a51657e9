#!/usr/bin/env python3
"""Blob files for tools/loader_check.cpp (the model loader on the CPU: byte comparison of two builds, sanitizer run).

    python tools/loader_check_blobs.py OUT_DIR

OUT_DIR/good/*.odkm: the three task assets, each also with opt_cone = 1; every XML under tests/assets that the loader takes; the
primitive-foot and equality variants that tests/test_capi_and_model.py builds.  OUT_DIR/bad/*.odkm, from the two backlash task blobs:
one record's nbytes set to 2^63 (or to what wraps an offset sum), a 2-D record's shape doubled; their truncations are made by
loader_check itself (--truncations).  Which XMLs load is asked of libodk.so (host-only); nothing here needs a GPU.
"""
import glob
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def record_offsets(blob: bytes):
    """[(name, header offset, nbytes, ndim)] of an ODKM blob"""
    n = struct.unpack_from("<I", blob, 8)[0]
    off, out = 16, []
    for _ in range(n):
        nm, _code, ndim, _s0, _s1, _s2, _s3, nbytes = struct.unpack_from("<32sII4IQ", blob, off)
        out.append((nm.rstrip(b"\0").decode(), off, nbytes, ndim))
        off += 64 + nbytes + (-nbytes) % 8
    return out


def with_nbytes(blob: bytes, name: str, nbytes: int) -> bytes:
    off = next(o for nm, o, _n, _d in record_offsets(blob) if nm == name)
    return blob[:off + 56] + struct.pack("<Q", nbytes) + blob[off + 64:]


def with_shape_doubled(blob: bytes, name: str) -> bytes:
    off = next(o for nm, o, _n, d in record_offsets(blob) if nm == name and d == 2)
    s0 = struct.unpack_from("<I", blob, off + 40)[0]
    return blob[:off + 40] + struct.pack("<I", 2 * s0) + blob[off + 44:]


def main():
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import Model, load_task_model
    from test_gpu_parity import _prim_feet_variant
    out = sys.argv[1]
    for d in ("good", "bad"):
        os.makedirs(os.path.join(out, d), exist_ok=True)
    good = {}
    for task in ("flat_terrain", "flat_terrain_backlash", "rough_terrain_backlash"):
        m = load_task_model(task)
        good[task] = m
        good[task + "_cone"] = Model({**m.a, "opt_cone": np.array([1], np.int32)})
    for xml in sorted(glob.glob(os.path.join(ROOT, "tests", "assets", "*.xml"))):
        good["xml_" + os.path.basename(xml)[:-4]] = Model.from_xml(xml)
    good["prim_capsule_sphere"] = _prim_feet_variant("rough_terrain_backlash", ("capsule", "sphere"))
    good["prim_sphere_sphere"] = _prim_feet_variant("rough_terrain_backlash", ("sphere", "sphere"))
    good["prim_flat_sphere_capsule"] = _prim_feet_variant("flat_terrain", ("sphere", "capsule"))
    eqm = good["xml_tail_biped_equality"]
    for tag, act in (("1100", (1, 1, 0, 0)), ("0000", (0, 0, 0, 0)), ("0010", (0, 0, 1, 0)), ("0001", (0, 0, 0, 1))):
        good["eq_active_" + tag] = Model({**eqm.a, "eq_active": np.array(act, np.int32)})
    b12 = good["xml_biped12"]
    j = b12.joint_id
    good["eq_biped12_joint"] = Model(dict(
        b12.a, eq_type=np.array([2], np.int32), eq_obj1id=np.array([j("left_ankle_pitch")], np.int32), eq_obj2id=np.array([j("left_knee")], np.int32),
        eq_active=np.array([1], np.int32), eq_data=np.array([[0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]], np.float64), eq_solref=np.array([[0.02, 1.0]]),
        eq_solimp=np.array([[0.9, 0.95, 0.001, 0.5, 2.0]]), neq=np.array([1], np.int32)))
    nload = 0
    for name, m in good.items():
        try:
            engine.model_reduction(m)
        except (engine.OdkError, ValueError, KeyError) as e:      # (ValueError / KeyError: tables.py cannot build the kernels' tables)
            print(f"  (not written: {name} does not load: {str(e)[:100]})")
            continue
        open(os.path.join(out, "good", name + ".odkm"), "wb").write(m.blob())
        nload += 1
    nbad = 0
    for task in ("flat_terrain_backlash", "rough_terrain_backlash"):
        blob = good[task].blob()
        recs = record_offsets(blob)
        two_d = [nm for nm, _o, _n, d in recs if d == 2]
        bad = {}
        bad[f"{task}_nbytes_first"] = with_nbytes(blob, recs[0][0], 1 << 63)
        bad[f"{task}_nbytes_mid"] = with_nbytes(blob, "k_body_chain", 1 << 63)
        bad[f"{task}_nbytes_last"] = with_nbytes(blob, recs[-1][0], 1 << 63)
        bad[f"{task}_nbytes_wrap"] = with_nbytes(blob, "k_body_chain", (1 << 64) - 64)
        for nm in (two_d[0], "k_dof_anc", two_d[-1]):
            bad[f"{task}_shape2x_{nm}"] = with_shape_doubled(blob, nm)
        for name, b in bad.items():
            open(os.path.join(out, "bad", name + ".odkm"), "wb").write(b)
        nbad += len(bad)
    print(f"{nload} blobs that load in {out}/good, {nbad} malformed ones in {out}/bad")


if __name__ == "__main__":
    main()
