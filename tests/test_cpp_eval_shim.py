"""The evaluation surface of include/NetPimpl.h (NetPimpl::Evaluation, RuntimeNet::Evaluate, TrainingNet::Evaluate) compiles warning-free
against the C ABI; tests/cpp/eval_shim.cpp checks the figures on a given matrix and, with a GPU, the trainer's call against a
snapshot's, bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "eval_shim")
    lib = os.path.join(ROOT, "annonet_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "eval_shim.cpp"),
                           "-o", exe, "-L" + lib, "-lannonet_hip", "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_eval_shim_builds_and_checks_the_figures(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "eval shim ok" in out.stdout


@pytest.mark.gpu
def test_eval_shim_evaluates_on_gpu(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "evaluated 2 windows" in out.stdout
