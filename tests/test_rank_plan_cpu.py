"""The blocking arithmetic of ptnn_rank_convergence (csrc/ptnn_rank_plan.hpp) under the address and undefined-behaviour sanitizers:
tests/rank_plan_check.cpp, a stand-alone program, is built with the host compiler and run as a process of its own.  Nothing of it
is loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-tempering-neural-net_amd", "csrc")


def test_block_plan_under_the_sanitizers(tmp_path):
    cxx = next(c for c in (shutil.which("g++"), shutil.which("c++"), shutil.which("clang++")) if c)
    exe = str(tmp_path / "rank_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "rank_plan_check.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.stdout, run.stderr)
