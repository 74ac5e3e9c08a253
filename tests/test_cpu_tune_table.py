"""The tuning knobs are one table (csrc/knobs.def) that mm2c_tune, mm2c_tune_get, mm2c_tune_key and mm2c_init walk.  tests/golden/tune_table.json holds what the
ladder of strcmp branches it replaced answered for every key and 26 probe values (recorded), and each key's default and environment variable (transcribed from the
sources of that time): the table must give the same.  No device is needed: mm2c_tune works before mm2c_init."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "tune_table.json")))
KEYS = GOLD["keys"]
ANY = {k for k, row in KEYS.items() if all(rc == 0 for rc in row["rc"])}   # the knobs that take any value and store 0 / 1

CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import mm2chain
print(json.dumps({k: mm2chain.tune_get(k) for k in mm2chain.tune_keys()}))
"""


def test_keys_and_environment_names_are_the_recorded_ones():
    import mm2chain
    assert len(KEYS) == 38
    assert mm2chain.tune_keys() == {k: row["env"] for k, row in KEYS.items()}
    with pytest.raises(mm2chain.Mm2cError):
        mm2chain.tune_get("trim")                       # a command, not a knob
    with pytest.raises(mm2chain.Mm2cError):
        mm2chain.tune_get("no_such_knob")


def test_a_fresh_process_holds_the_defaults():
    env = {k: v for k, v in os.environ.items() if not k.startswith("MM2C_") or k == "MM2C_LIB_PATH"}
    out = subprocess.check_output([sys.executable, "-c", CHILD, os.path.join(ROOT, "minimap2-fpga_amd")], text=True, env=env)
    got = json.loads(out.splitlines()[-1])
    assert got == {k: [row["default"], row["default"]] for k, row in KEYS.items()}


def test_return_codes_and_stored_values_are_the_recorded_ones():
    import mm2chain
    lib = mm2chain.load()
    E_ARG = GOLD["unknown_key_rc"]
    assert E_ARG != 0 and lib.mm2c_tune(b"no_such_knob", 1) == E_ARG and b"no_such_knob" in lib.mm2c_last_error()
    assert lib.mm2c_tune(None, 1) == GOLD["null_key_rc"]
    assert lib.mm2c_tune(b"trim", 0) == GOLD["trim_rc"] == 0
    for key, row in KEYS.items():
        entry = mm2chain.tune_get(key)
        assert entry[1] == row["default"], key
        try:
            for v, want in zip(GOLD["probes"], row["rc"]):
                before = mm2chain.tune_get(key)[0]
                rc = lib.mm2c_tune(key.encode(), v)
                assert rc == want, f"mm2c_tune({key!r}, {v}) returned {rc}, recorded {want}"
                if rc != 0:
                    assert rc == E_ARG and key.encode() in lib.mm2c_last_error(), (key, v, lib.mm2c_last_error())
                    stored = before                                         # a refused value changes nothing
                elif key in ANY:
                    stored = int(v != 0)
                elif key == "coop_w8_above":
                    stored = min(v, 1 << 30)
                else:
                    stored = v
                assert mm2chain.tune_get(key) == (stored, row["default"]), (key, v)
        finally:
            mm2chain.tune(key, entry[0])


def test_tuned_puts_back_what_it_found():
    import mm2chain
    get = lambda k: mm2chain.tune_get(k)[0]
    d_ring, d_far, d_seg = get("ring_class"), get("far_ring"), get("seg_min")
    assert (d_ring, d_far, d_seg) == (3, 1, 256)
    with mm2chain.tuned(ring_class=4, far_ring=2):
        assert (get("ring_class"), get("far_ring")) == (4, 2)
        with mm2chain.tuned(far_ring=0, ring_class=1, seg_min=0):           # nested, in the other order
            assert (get("ring_class"), get("far_ring"), get("seg_min")) == (1, 0, 0)
        assert (get("ring_class"), get("far_ring"), get("seg_min")) == (4, 2, d_seg)   # ... back to what the outer block set, not to the defaults
    assert (get("ring_class"), get("far_ring")) == (d_ring, d_far)
    with pytest.raises(ZeroDivisionError):                                  # the body raises
        with mm2chain.tuned(seg_min=77, coop_plans=0):
            assert (get("seg_min"), get("coop_plans")) == (77, 0)
            1 / 0
    assert (get("seg_min"), get("coop_plans")) == (d_seg, 2)
    with mm2chain.tuned(seg_min=5):                                         # a refused value: the ones set before it are put back, the body never runs
        with pytest.raises(mm2chain.Mm2cError):
            with mm2chain.tuned(seg_min=9, ring_class=99):
                raise AssertionError("the body ran")
        assert (get("seg_min"), get("ring_class")) == (5, d_ring)
    assert get("seg_min") == d_seg
    with mm2chain.tuned(ring_class=4), mm2chain.tuned(ring_class=0):        # the same knob twice: each level puts back its own
        assert get("ring_class") == 0
    assert get("ring_class") == d_ring


def test_integration_md_lists_every_key_and_variable():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## F. "):]
    sec = sec[:sec.index("\n## ", 1)] if "\n## " in sec[1:] else sec
    missing = [name for key, row in KEYS.items() for name in (key, row["env"]) if name and f"`{name}`" not in sec]
    assert not missing, f"INTEGRATION.md section F does not name {missing}"
