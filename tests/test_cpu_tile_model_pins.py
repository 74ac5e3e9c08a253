"""The NumPy model of the tile kernel's hand-written loop (tests/tile_model.py) returns, for each of the loops it has modelled (before the score-bound exit, with it,
and with stamps and marks behind the fold's decision), what was recorded of it in tests/golden/tile_model_pins.json: every stats counter, f and p, the anchors that
left early and the events, on the inputs of tests/test_cpu_score_exit.py and tests/test_cpu_late_stamps.py and the fold drivers (tests/golden/make_tile_model_pins.py
says which, and makes the file).  A model may count more than was recorded; what was recorded must not move."""
import functools
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_tile_model_pins as mk  # noqa: E402

FIXTURE = json.load(open(mk.FIXTURE))


@functools.lru_cache(None)
def _records():
    return {key: rest for key, *rest in mk.records()}


def test_the_fixture_holds_every_pin_and_nothing_else():
    assert sorted(FIXTURE["pins"]) == sorted(_records())
    assert sorted(FIXTURE["keys"]) == sorted(mk.MODELS)


@pytest.mark.parametrize("key", sorted(FIXTURE["pins"]))
def test_model_returns_what_was_recorded(key):
    model, work, kw, mode = _records()[key]
    got = mk.pin(model, work, kw, mode, keys=FIXTURE["keys"][model])
    assert got.pop("keys") == FIXTURE["keys"][model]
    want = FIXTURE["pins"][key]
    moved = {k: (w, g) for k, w, g in zip(FIXTURE["keys"][model], want["stats"], got["stats"]) if w != g}
    assert not moved, f"{key}: stats that moved (recorded, now): {moved}"
    assert got == want, key
