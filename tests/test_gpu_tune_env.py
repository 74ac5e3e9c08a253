"""mm2c_init applies the knobs' environment variables from the table of csrc/knobs.def: out-of-range values are clamped (mm2c_tune refuses them), the on / off
variables take atoi(...) != 0, and ring_class -- alone among the knobs -- goes back to its default at every init that finds its variable unset.  The expected
values are those of the getenv block the table replaced; the line of mm2c_init (csrc/mm2chain_api.cpp of that time) each comes from stands beside it."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = (
    "import json, sys\n"
    f"sys.path.insert(0, {os.path.join(ROOT, 'minimap2-fpga_amd')!r})\n"
    "import mm2chain\n"
    "get = lambda k: mm2chain.tune_get(k)[0]\n"
    "mm2chain.init()\n")
UNSET = HEAD + (
    "bad = {k: mm2chain.tune_get(k) for k in mm2chain.tune_keys() if get(k) != mm2chain.tune_get(k)[1]}\n"
    "assert not bad, bad\n"
    "mm2chain.tune('ring_class', 4); mm2chain.tune('far_ring', 2)\n"
    "mm2chain.shutdown(); mm2chain.init()\n"
    "assert get('ring_class') == 3, get('ring_class')\n"       # :559  G.ring_class = rc ? ... : 3
    "assert get('far_ring') == 2, get('far_ring')\n"           # :563  if (fr) ...: untouched without the variable
    "mm2chain.shutdown()\n")
SET = HEAD + (
    "print(json.dumps({k: get(k) for k in mm2chain.tune_keys()}))\n"
    "mm2chain.shutdown()\n")

# variable: (value, key, what mm2c_init made of it)
CLAMPED = {
    "MM2C_RING_CLASS": ("9", "ring_class", 4),                       # :559  max(0, min(4, atoi))
    "MM2C_FAR_RING": ("-3", "far_ring", 0),                          # :563  max(0, min(2, atoi))
    "MM2C_WIDE_SHARE_THRESHOLD": ("250", "wide_share_threshold", 100),   # :567  max(0, min(100, atoi))
    "MM2C_COMBINER_LANES": ("0", "combiner_lanes", 1),               # :571  max(1, min(16, atoi))
    "MM2C_SPLIT_STREAMS": ("7", "split_streams", 2),                 # :565  max(0, min(2, atoi))
    "MM2C_DECLINE_WHEN_BUSY": ("5", "decline_when_busy", 2),         # :587  max(0, min(2, atoi))
    "MM2C_COMBINE_MAX": ("-1", "combine_max_anchors", 0),            # :569  max(0, atoi)
    "MM2C_COOP_WAVES": ("-2", "coop_waves", 0),                      # :575  max(0, atoi)
    "MM2C_PIPE_COOP_CHUNKS": ("-1", "pipe_coop_chunks", 0),          # :577  max(0, atoi)
    "MM2C_FAR_RING_THRESHOLD": ("-4", "far_ring_threshold", 0),      # :589  max(0, atoi)
}
ON_OFF = {                                                           # atoi(...) != 0
    "MM2C_EPI_FUSED": "epi_fused",                                   # :561
    "MM2C_DIRECT_PASS": "direct_pass",                               # :573
    "MM2C_Q24_RING": "q24_ring",                                     # :579
    "MM2C_COMPACT_RING": "compact_ring",                             # :581
    "MM2C_SINGLE_LAUNCH": "single_launch",                           # :583
    "MM2C_FUSE_ST": "fuse_st",                                       # :585
}


def _child(code, env):
    return subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", code], capture_output=True, text=True, env=env)


def test_init_applies_the_environment_as_the_table_says():
    import mm2chain
    table = mm2chain.tune_keys()
    assert {v for v in table.values() if v} == set(CLAMPED) | set(ON_OFF)                       # one value for every variable of the table
    base = {k: v for k, v in os.environ.items() if k not in set(table.values())}
    r = _child(UNSET, base)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-1500:])                 # (the second child starts only after a clean first one)
    env = dict(base, **{var: val for var, (val, _, _) in CLAMPED.items()}, **{var: "7" for var in ON_OFF})
    r = _child(SET, env)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-1500:])
    got = json.loads(r.stdout.splitlines()[-1])
    want = {k: mm2chain.tune_get(k)[1] for k in table}
    want.update({key: val for _, key, val in CLAMPED.values()})
    want.update({key: 1 for key in ON_OFF.values()})
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
