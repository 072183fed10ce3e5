"""(no GPU) which of an aligner's two buffer sets takes the next device-resident launch (bgreat_amd/csrc/launch_taker.h) on the host:
tests/launch_taker_check.cpp, a stand-alone program, enumerates the rule's eight inputs under the undefined-behaviour sanitizer -- the primary
whenever it is idle, the twin only when the primary is busy, never the taker of the launch before when both are busy.  And the knob's number."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_launch_taker_rule(tmp_path):
    exe = str(tmp_path / "launch_taker_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(HERE, "..", "bgreat_amd", "csrc"), os.path.join(HERE, "launch_taker_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok 8", (out.stdout, out.stderr)


def test_knob_number():
    """KNOB_DEVICE_OVERLAP is the header's BGR_KNOB_DEVICE_OVERLAP, and no other knob of the header has its number."""
    import bgreat_amd as B
    text = open(os.path.join(HERE, "..", "include", "bgreat_gpu.h")).read()
    knobs = {name: int(num) for name, num in re.findall(r"#define BGR_KNOB_(\w+) (\d+)u", text)}
    assert knobs["DEVICE_OVERLAP"] == B.KNOB_DEVICE_OVERLAP == 14
    assert len(set(knobs.values())) == len(knobs), knobs
    for name, num in knobs.items():
        assert getattr(B, "KNOB_" + name) == num, name
