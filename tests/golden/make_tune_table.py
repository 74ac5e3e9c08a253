"""Records tests/golden/tune_table.json: what mm2c_tune answers for every key and every probe value, in a fresh process that never calls mm2c_init (no device is
needed).  First recorded from the library as it stood while mm2c_tune was a ladder of strcmp branches, before the knobs moved into csrc/knobs.def
(tests/test_cpu_tune_table.py holds the table-driven mm2c_tune to it).

Recorded: the return codes ("rc", one per probe value), and those for an unknown key, for key == NULL and for "trim".
Transcribed by hand, NOT recorded (the library of that time had no getter): "default", from the initialisers in csrc/api_internal.h and csrc/mm2chain_sketch.cpp,
and "env", from the getenv calls of mm2c_init in csrc/mm2chain_api.cpp.

    python tests/golden/make_tune_table.py [path/to/libmm2chain_hip.so] > tests/golden/tune_table.json
"""
import ctypes as C
import json
import os
import sys

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
PROBES = [INT_MIN, -5, -1, 0, 1, 2, 3, 4, 5, 6, 7, 15, 16, 17, 63, 64, 65, 100, 101, 1023, 1024, 1025, 1 << 20, 1 << 30, (1 << 30) + 1, INT_MAX]

# key: (default, environment variable) -- the keys of the ladder in its order, "trim" left out
KEYS = {
    "ring_class": (3, "MM2C_RING_CLASS"),
    "far_ring": (1, "MM2C_FAR_RING"),
    "far_ring_threshold": (7, "MM2C_FAR_RING_THRESHOLD"),
    "noskip_loop": (1, None),
    "read_chunk_bases": (1 << 27, None),
    "index_chunk_bases": (1 << 27, None),
    "heap_sort": (0, None),
    "wide_share_threshold": (40, "MM2C_WIDE_SHARE_THRESHOLD"),
    "split_streams": (1, "MM2C_SPLIT_STREAMS"),
    "compact_ring": (1, "MM2C_COMPACT_RING"),
    "force_tab": (0, None),
    "epi_fused": (1, "MM2C_EPI_FUSED"),
    "pipeline_chunk_anchors": (20 << 20, None),
    "pipeline_pieces": (8, None),
    "pipeline_taper": (0, None),
    "pipeline_min_chunk": (4 << 20, None),
    "coop_waves": (16, "MM2C_COOP_WAVES"),
    "combine_max_anchors": (1 << 17, "MM2C_COMBINE_MAX"),
    "combiner_lanes": (4, "MM2C_COMBINER_LANES"),
    "pipe_coop_chunks": (1, "MM2C_PIPE_COOP_CHUNKS"),
    "q24_ring": (1, "MM2C_Q24_RING"),
    "packed_fp": (1, None),
    "score_bound_exit": (1, None),
    "pin_workers": (1, None),
    "decline_when_busy": (0, "MM2C_DECLINE_WHEN_BUSY"),
    "direct_pass": (1, "MM2C_DIRECT_PASS"),
    "coop_plans": (2, None),
    "host_st": (0, None),
    "fused_out": (1, None),
    "single_launch": (1, "MM2C_SINGLE_LAUNCH"),
    "fuse_st": (1, "MM2C_FUSE_ST"),
    "seg_prepass": (1, None),
    "coop_w8_above": (256, None),
    "coop_max_tasks": (1024, None),
    "plan_cut": (1, None),
    "plan_cut_min": (8192, None),
    "multi_min_anchors": (1 << 20, None),
    "seg_min": (256, None),
}


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    lib_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "..", "..", "minimap2-fpga_amd", "libmm2chain_hip.so")
    lib = C.CDLL(lib_path)
    lib.mm2c_tune.restype = C.c_int
    lib.mm2c_tune.argtypes = [C.c_char_p, C.c_int]
    out = {
        "recorded": ["rc", "unknown_key_rc", "null_key_rc", "trim_rc"],
        "transcribed": ["default", "env"],
        "probes": PROBES,
        "unknown_key_rc": lib.mm2c_tune(b"no_such_knob", 1),
        "null_key_rc": lib.mm2c_tune(None, 1),
        "trim_rc": lib.mm2c_tune(b"trim", 0),
        "keys": {key: {"default": dflt, "env": env, "rc": [lib.mm2c_tune(key.encode(), v) for v in PROBES]} for key, (dflt, env) in KEYS.items()},
    }
    lines = ["{"]
    for k in ("recorded", "transcribed", "probes", "unknown_key_rc", "null_key_rc", "trim_rc"):
        lines.append(f" {json.dumps(k)}: {json.dumps(out[k])},")
    lines.append(' "keys": {')
    rows = [f"  {json.dumps(key)}: {json.dumps(row)}" for key, row in out["keys"].items()]
    lines.append(",\n".join(rows))
    lines.append(" }\n}")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
