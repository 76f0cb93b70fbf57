"""csrc/nlr_tape.h on the CPU: the header is plain C++, so the walk of a GEMM on the weight tape, the stacked heads and the program tables
the kernels take their constants from are checked by a stand-alone program (tests/tape_layout_check.cpp) built with the host compiler."""
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_walk_program_tables_and_heads(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tape_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "tape_layout_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "tape layout ok" in r.stdout


def test_no_tape_literals_left_in_the_builders():
    """The chunk size is named (NLR_CHUNK_*), and the element map of the walk is written once in the host code."""
    csrc = os.path.join(os.path.dirname(HERE), "nerf-lidar_amd", "csrc")
    for name in ("nlr_api.hip", "nlr_mlp_train.hip"):
        text = open(os.path.join(csrc, name)).read()
        for line in text.split("\n"):  # a chunk-size literal in a line about tapes (sizes, padding, slack, chunk counts)
            assert not (re.search(r"\b(16384|16383|32768)\b", line) and re.search(r"tape|chunk|slack|frag|\bt\.size", line, re.I)), f"{name}: {line.strip()}"
        assert "(lane & 15)" not in text, f"{name}: a copy of the fragment's element map"
    assert open(os.path.join(csrc, "nlr_tape.h")).read().count("(lane & 15)") == 1
