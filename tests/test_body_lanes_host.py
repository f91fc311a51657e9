"""Body-to-lane layout of the kinematics / inertia sweeps (odk_model_body_lanes): every serial body chain in
consecutive lanes of ONE 16-lane row, in chain order, so the chain scans are DPP row shifts.  Host-only, no GPU."""
import os

import pytest

from conftest import ROOT

TASKS = ("flat_terrain", "flat_terrain_backlash", "rough_terrain_backlash")
XMLS = ("biped12.xml", "tail_biped.xml", "tail_biped_elliptic.xml", "tail_biped_equality.xml", "tail_biped_loop.xml")


def _model(name):
    from open_duck_playground_amd.model import Model, load_task_model
    if name in TASKS:
        return load_task_model(name)
    return Model.from_xml(os.path.join(ROOT, "tests", "assets", name))


def _chains(model):
    """[[body, ...], ...]: the serial chains as the kernel tables define them (head first)."""
    from open_duck_playground_amd.tables import build_kernel_tables
    t = build_kernel_tables(model.a)
    is_path, head = t["k_body_is_path"], t["k_body_path_head"]
    chains = []
    for b in range(len(is_path)):
        if is_path[b] and head[b]:
            chains.append([b])
        elif is_path[b]:
            chains[-1].append(b)
    return chains


@pytest.mark.parametrize("lanes", [32, 64])
@pytest.mark.parametrize("name", TASKS + XMLS)
def test_every_chain_sits_in_one_row_in_order(name, lanes):
    from open_duck_playground_amd import engine
    model = _model(name)
    nb = int(model.a["nbody"][0])
    lane_body = engine.model_body_lanes(model, lanes)
    assert len(lane_body) == lanes
    placed = [b for b in lane_body if b >= 0]
    assert sorted(placed) == list(range(nb))                 # every body on exactly one lane, no other ids
    where = {b: l for l, b in enumerate(lane_body) if b >= 0}
    chains = _chains(model)
    assert chains
    for chain in chains:
        lanes_of = [where[b] for b in chain]
        assert lanes_of == list(range(lanes_of[0], lanes_of[0] + len(chain))), (chain, lanes_of)   # contiguous, in chain order
        assert lanes_of[0] // 16 == lanes_of[-1] // 16, (chain, lanes_of)                          # inside one 16-lane row


def test_duck_third_chain_moves_to_the_second_row():
    from open_duck_playground_amd import engine
    model = _model("flat_terrain")
    assert [c[0] for c in _chains(model)] == [3, 8, 12]
    for lanes in (32, 64):
        lane_body = engine.model_body_lanes(model, lanes)
        assert lane_body[:12] == list(range(12))             # bodies 0-11 keep their lanes
        assert lane_body[16:21] == [12, 13, 14, 15, 16]      # the chain at body 12 no longer crosses lanes 15 / 16
        assert lane_body[12] == 17                           # the body after it takes the first free lane
        assert all(b == -1 for b in lane_body[13:16] + lane_body[21:])


def test_body_lanes_rejects_other_lane_counts(model_a):
    from open_duck_playground_amd import engine
    with pytest.raises(engine.OdkError):
        engine.model_body_lanes(model_a, 16)
