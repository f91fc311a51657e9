"""Host-side checks of the model's launch-invariant values in their packed form (profiles/load_waits): the three words the plane-floor
step kernel extracts its small integers from (DevModel::hot_pk), the loader's refusal of a value that does not fit its field, and the
rest of the device model, which the change may not touch.  The load-wait tool (tools/isa_load_waits.py) is run on a listing of shape A's
kernel set compiled here (CPU only, cross-compiled for gfx950)."""
import glob
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "assets")
CSRC = os.path.join(ROOT, "open_duck_playground_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# include/odk.h odk_model_hot_words: (field, word, first bit, bits, scale) -- a scaled field holds the byte offset value * 4
LAYOUT = [("foot_body0", 0, 0, 8, 4), ("foot_body1", 0, 8, 8, 4), ("foot_nvert0", 0, 16, 8, 1), ("foot_nvert1", 0, 24, 8, 1),
          ("foot_rchain_first0", 1, 0, 8, 4), ("foot_rchain_first1", 1, 8, 8, 4), ("foot_rchain_len0", 1, 16, 4, 1), ("foot_rchain_len1", 1, 20, 4, 1),
          ("ls_iterations", 1, 24, 8, 1), ("max_nonpath_level", 2, 0, 8, 1), ("np_count", 2, 8, 8, 1), ("foot_prim", 2, 16, 8, 1)]


def _shipped_models():
    from open_duck_playground_amd.model import Model, load_task_model
    for task in ("flat_terrain", "flat_terrain_backlash", "rough_terrain_backlash"):
        yield task, load_task_model(task)
    for path in sorted(glob.glob(os.path.join(ASSETS, "*.xml"))):
        yield os.path.basename(path), Model.from_xml(path, sim_dt=0.002)


def _pack(fields):
    words = [0, 0, 0]
    for name, w, shift, bits, scale in LAYOUT:
        v = fields[name] + (1 if name == "max_nonpath_level" else 0)
        assert 0 <= v * scale < (1 << bits), (name, v)
        words[w] |= (v * scale) << shift
    return words


def _unpack(words):
    out = {}
    for name, w, shift, bits, scale in LAYOUT:
        stored = (words[w] >> shift) & ((1 << bits) - 1)
        assert stored % scale == 0, (name, stored)
        out[name] = stored // scale - (1 if name == "max_nonpath_level" else 0)
    return out


def test_packed_words_round_trip_for_every_shipped_model():
    from open_duck_playground_amd import engine
    seen = 0
    for name, model in _shipped_models():
        try:
            hw = engine.model_hot_words(model)
        except (engine.OdkError, ValueError) as e:      # the assets without a kernel set (or without the env's sites) are refused for THAT reason, not for a field's range
            assert "does not fit" not in str(e), (name, str(e))
            continue
        assert _pack(hw["fields"]) == hw["packed"], (name, hw)
        assert _unpack(hw["packed"]) == hw["fields"], (name, hw)
        # the bits no field owns stay clear
        assert hw["packed"][2] >> 24 == 0, (name, hw["packed"])
        f = hw["fields"]
        assert f["ls_iterations"] == int(np.asarray(model.a["opt_ls_iterations"]).ravel()[0]) and 1 <= f["np_count"] <= 4 and f["foot_body0"] != f["foot_body1"], (name, f)
        seen += 1
    assert seen >= 10


def test_loader_refuses_an_over_range_field_by_name():
    from open_duck_playground_amd import engine
    from open_duck_playground_amd.model import Model, load_task_model
    m = load_task_model("flat_terrain")
    with pytest.raises(engine.OdkError, match=r"ls_iterations = 256 does not fit the 8-bit field the step kernels read it from \(0 \.\. 255\)"):
        engine.model_hot_words(Model({**m.a, "opt_ls_iterations": np.array([256], np.int32)}))
    assert engine.model_hot_words(Model({**m.a, "opt_ls_iterations": np.array([255], np.int32)}))["fields"]["ls_iterations"] == 255


def test_device_model_outside_the_new_fields_is_the_parents(tmp_path):
    """tools/loader_check dumps the DevModel bytes of every blob tools/loader_check_blobs.py writes; the new fields sit behind every older
    one, so the bytes in front of them must be the ones the commit before the change wrote: tests/golden/devmodel_parent_sha256.json holds
    that commit's size of DevModel and the SHA-256 of its bytes per blob (made with that commit's loader_check, never this one)."""
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc is needed to compile tools/loader_check.cpp")
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "devmodel_parent_sha256.json")))
    exe, blobs, dump = str(tmp_path / "loader_check"), str(tmp_path / "blobs"), str(tmp_path / "dump")
    os.makedirs(dump)
    subprocess.run([HIPCC, "-O1", "-std=c++17", "--cuda-host-only", "-x", "hip", "-o", exe, os.path.join(ROOT, "tools", "loader_check.cpp"),
                    os.path.join(CSRC, "odk_model_load.hip")], check=True, capture_output=True)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "loader_check_blobs.py"), blobs], check=True, capture_output=True)
    files = sorted(glob.glob(os.path.join(blobs, "good", "*.odkm")))
    subprocess.run([exe, "--dump", dump, "--expect", "ok", *files], check=True, capture_output=True)
    n, seen = gold["devmodel_bytes"], 0
    for f in files:
        name = os.path.basename(f)[:-5]
        raw = open(os.path.join(dump, name + ".odkm.bin"), "rb").read()
        assert len(raw) > n + 12, name      # the new fields lie behind the parent's last byte
        assert hashlib.sha256(raw[:n]).hexdigest() == gold["sha256"][name], name
        seen += 1
    assert seen == len(gold["sha256"]) >= 20


def test_load_wait_tool_on_shape_a(tmp_path):
    """tools/isa_load_waits.py on a fresh listing: the queue model (a wait vmcnt(N) covers all but the last N) gives every load of the substep a
    covering wait, and the plane-floor step kernel no longer loads, inside a substep, the values the model packs for it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_load_waits as lw
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc is needed to compile the listing the tool reads")
    listing = lw.compile_listing("A", str(tmp_path / "odk_env_A.s"))
    recs = lw.substep(lw.load_waits(listing, "A"))
    assert recs and all(r["n_all"] is not None and 0 <= r["n_valu"] <= r["n_all"] for r in recs)
    per = {}
    for r in recs:
        per.setdefault(r["phase"], []).append(r)
    print({k: len(v) for k, v in per.items()})
    # P7 (after 6: foot poses, plane, 17th vertex), the candidates of P9 (after 9: foot chains) and the line search (after 15: its loop
    # bound) load nothing; what is left in P2 (after 1) is the fold's second pass, which no shipped robot runs
    assert "after 6" not in per and "after 9" not in per and "after 15" not in per, sorted(per)
    assert len(per.get("after 1", [])) <= 5
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_load_waits.py"), "A", "--listing", listing], check=True, capture_output=True, text=True).stdout
    assert any(l.startswith("substep") and int(l.split()[1]) == len(recs) for l in txt.splitlines())
