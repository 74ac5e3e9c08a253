"""The route decision of launch_chain_dp (chain_kernel.hip, decide_route), pinned without a GPU: tests/route_dump.cpp asks the launcher, by dry run, which
kernels it would take for a few thousand calls -- scalar sets x ring_class 0 .. 4 x knobs, pass shapes, device-side cuts and per-task distances -- and prints
the variant text with the LaunchInfo flags that are not in it.  The output must be tests/golden/route_table.txt line for line.

The table was recorded with this dumper from the launcher as it stood before the decision was gathered into decide_route.  To make it again after a change that
is MEANT to alter a route: build, run the dumper as this test does, put its output in the table's place and review the diff of the T / case lines."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "minimap2-fpga_amd")


def build_dumper(out_dir, lib=None):
    lib = lib or os.path.join(PKG, "libmm2chain_hip.so")
    exe = os.path.join(str(out_dir), "route_dump")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "route_dump.cpp"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(os.path.abspath(lib)),
                           "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


def test_route_table_is_the_recorded_one(tmp_path):
    exe = build_dumper(tmp_path)
    env = {k: v for k, v in os.environ.items() if k != "MM2C_FORCE_TAB"}      # (the launcher's one environment switch)
    got = subprocess.check_output([exe], text=True, env=env).splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "route_table.txt")).read().splitlines()
    cases = [ln for ln in want if ln[:1].isdigit()]
    texts = [ln for ln in want if ln.startswith("T")]
    assert len(cases) >= 3000 and len(texts) >= 40, "the recorded table is not whole"
    diff = [(k + 1, w, g) for k, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff, f"{len(diff)} lines differ from the recorded table; first: line {diff[0][0]}: recorded {diff[0][1]!r}, now {diff[0][2]!r}"
    assert len(got) == len(want)
