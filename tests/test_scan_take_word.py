"""(no GPU) the packed word of the anchor scan (bgreat_amd/csrc/scan_take_word.h) on the host: tests/take_word_check.cpp, a stand-alone
program, packs and unpacks every admissible item under the undefined-behaviour sanitizer."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_take_word_round_trip(tmp_path):
    exe = str(tmp_path / "take_word_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(HERE, "..", "bgreat_amd", "csrc"), os.path.join(HERE, "take_word_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.stdout, out.stderr)
    assert int(out.stdout.split()[1]) > 1000000
