"""The owners of effex_amd/csrc/h_own.h (DevBuf, PinnedBuf, Event, Stream, the large-result group) on the host: tests/emul/emul_own.cpp
is a program of its own with counting stand-ins for the HIP calls, built here with the sanitizers linked in and run as a child."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_own.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# the runtimes inside the executable where g++ has them as archives (nothing about the process's other libraries can then come
# between the program and them), else as g++ links them by default, else -- a g++ without the runtimes -- the program's own checks alone
BUILDS = (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, [])


def test_owners_release_once_and_in_order(tmp_path):
    exe = str(tmp_path / "emul_own")
    for flags in BUILDS:
        built = subprocess.run(["g++", "-std=c++17", "-O1", "-g"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
        if built.returncode == 0:
            break
        sys.stderr.write("emul_own: g++ %s failed: %s\n" % (" ".join(flags), built.stderr.strip().splitlines()[-1:]))
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "emul_own: ok" in run.stdout
