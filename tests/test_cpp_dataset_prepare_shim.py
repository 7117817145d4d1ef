"""NetPimpl::Dataset::Prepare and TrainingNet::StartTrainingOnPickedCrops (include/NetPimpl.h) compile warning-free against the C ABI;
tests/cpp/dataset_prepare_shim.cpp prepares one image and runs one optimiser step on picked crops."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "dataset_prepare_shim")
    lib = os.path.join(ROOT, "annonet_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "dataset_prepare_shim.cpp"),
                           "-o", exe, "-L" + lib, "-lannonet_hip", "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_dataset_prepare_shim_builds_and_resolves(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "dataset prepare shim ok" in out.stdout


@pytest.mark.gpu
def test_dataset_prepare_shim_steps_on_gpu(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "one step on 4 picked crops" in out.stdout
