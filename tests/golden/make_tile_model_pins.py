"""Pins of the NumPy model of the tile kernel's hand-written loop (tests/tile_model.py), first recorded from the three separate models it was merged from (the
loop before the score-bound exit, with it, and with stamps and marks behind the fold's decision): what each returns on the inputs the CPU tests already build (tests/score_exit_data.py, tests/late_stamp_data.py, the fold drivers of tests/helpers.py), recorded so that a
change to a model that is meant to keep its results can be held to them (tests/test_cpu_tile_model_pins.py).  Nothing here comes from the reference or the oracle:
the models alone (avg is the oracle's avg_qspan_scaled, as in the tests).  Per (group of inputs, model, arguments): the stats summed over the group's tasks, a SHA-256
over the per-task stats, one over the bytes of every task's f and p, and length and SHA-256 of exit_anchors and of the two events lists where the model has them.
Output: tests/golden/tile_model_pins.json (totals and digests only)."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "minimap2-fpga_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import late_stamp_data as ls  # noqa: E402
from oracle_binding import avg_qspan  # noqa: E402
import score_exit_data as sx  # noqa: E402
from tile_model import chain_tile_model  # noqa: E402

FIXTURE = os.path.join(HERE, "tile_model_pins.json")
# the loop that each pin was recorded from -> (the arguments that make the model that loop, what was recorded of it beyond stats)
MODELS = {"before": (dict(score_exit="off", late_stamps=False, tile_skip=True), ()),
          "exit": (dict(late_stamps=False), ("score_exit", "exit_anchors")),
          "late_stamps": ({}, ("score_exit", "exit_anchors", "events"))}
FOLD_SHAPES = ((1100, 4, 0.05, 0.15), (2000, 3, 0.0, 0.3), (700, 12, 0.2, 0.15), (500, 40, 0.0, 0.2))


def groups():
    """[(name, [(P, task, avg)], model arguments, score_exit modes)]"""
    from helpers import fold_driver_tasks
    from mm2chain import params
    own = lambda P, tasks: [(P, t, avg_qspan(t)) for t in tasks]
    G = []
    for form, (compact, NX) in sx.FORMS.items():
        for max_skip in sx.SKIPS:
            G.append((f"standard, max_skip {max_skip}, {form}", own(params.make_params(max_skip=max_skip), sx.standard_tasks()), dict(NX=NX, compact=compact), ("auto",)))
        G.append((f"equality edge, {form}", [(P, t, avg_qspan(t)) for P, t, _ in (sx.edge_case(kind, far) for kind, far in sx.EDGE_CASES)], dict(NX=NX, compact=compact), ("auto",)))
        G.append((f"short tasks, {form}", own(params.map_ont(), sx.short_tasks()), dict(NX=NX, compact=compact), ("auto",)))
        # (less the 2 000-anchor one, for the run time: the standard inputs hold it at every max_skip)
        fold = [t for t in fold_driver_tasks(np.random.default_rng(4242), shapes=FOLD_SHAPES) if t.shape[0] != 2000]
        G.append((f"fold drivers, max_skip 3, {form}", own(params.make_params(max_skip=3), fold), dict(NX=NX, NF=4, compact=compact), ("auto", "off")))
    P, tasks, _ = sx.negative_gap_case()
    G.append(("gap_scale -2", own(P, tasks), dict(NX=16, compact=True), ("auto", "force")))
    P, t = sx.cut_task()
    G.append(("pieces of the device-cut task", [(P, t[s:e], avg_qspan(t)) for s, e in sx.cut_pieces(P, t)], dict(NX=16, NF=4, compact=True), ("auto",)))
    for gap_scale in (1.0, 0.8):
        cases = [ls.depth_case(m, part, gap_scale)[:2] for m, part in ls.DEPTH_CASES]
        G.append((f"depth cases, gap_scale {gap_scale}", [(P, t, avg_qspan(t)) for P, t in cases], dict(NX=16, NF=4, compact=True), ("auto",)))
    return G


def _digest(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()


def pin(model, work, kw, mode, keys=None):
    """one record: `model` over the tasks of `work`.  keys: the stats to record (all that the model gives, when None)"""
    own_kw, takes = MODELS[model]
    fp = hashlib.sha256()
    per_task, exits, events = [], [], dict(unstamped=[], own_marks=[])
    for P, t, avg in work:
        st, ex, ev = {}, [], dict(unstamped=[], own_marks=[])
        more = dict(zip(("score_exit", "exit_anchors", "events"), (mode, ex, ev)))
        f, p = chain_tile_model(P, t, avg, stats=st, **kw, **own_kw, **{k: more[k] for k in takes})
        assert f.dtype == np.int32 and p.dtype == np.int32
        fp.update(f.tobytes()); fp.update(p.tobytes())
        per_task.append({k: int(st[k]) for k in (keys or sorted(st))})
        exits.append([int(i) for i in ex])
        events["unstamped"].append([[int(i), where] for i, where in ev["unstamped"]])
        events["own_marks"].append([int(i) for i in ev["own_marks"]])
    rec = dict(keys=list(per_task[0]), stats=[sum(s[k] for s in per_task) for k in per_task[0]], stats_sha256=_digest(per_task), fp_sha256=fp.hexdigest())
    if "exit_anchors" in takes:
        rec["exit_anchors"] = dict(n=sum(map(len, exits)), sha256=_digest(exits))
    if "events" in takes:
        rec["events"] = {k: dict(n=sum(map(len, v)), sha256=_digest(v)) for k, v in events.items()}
    return rec


def records():
    """(fixture key, model, work, model arguments, score_exit) of every pin"""
    for name, work, kw, modes in groups():
        for model, (_, takes) in MODELS.items():
            for mode in (modes if "score_exit" in takes else ("-",)):
                yield f"{name} | {model} | {mode}", model, work, kw, mode


if __name__ == "__main__":
    pins = {key: pin(model, work, kw, mode) for key, model, work, kw, mode in records()}
    keys = {}                                                         # the same for every record of a model: stored once
    for key, rec in pins.items():
        assert keys.setdefault(key.split(" | ")[1], rec["keys"]) == rec.pop("keys")
    with open(FIXTURE, "w") as fp:
        json.dump(dict(keys=keys, pins=pins), fp, separators=(",", ":"), sort_keys=True)
        fp.write("\n")
    print(f"{len(pins)} pins, {os.path.getsize(FIXTURE)} bytes")
