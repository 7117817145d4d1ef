"""The tile list of the conv and filter-gradient kernels (annonet_amd/csrc/tilewalk.h) on the CPU: tests/cpp/tilewalk_check.cpp
includes the header alone and checks, exhaustively over small grids, that the workgroups' walks partition the list (plain and in
XCD bands), that the incremental cursor equals the division decode, and that the band walk and the host tile counts equal lists
written out by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_walk_partition_cursor_and_frozen_lists(tmp_path):
    exe = str(tmp_path / "tilewalk_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "annonet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "tilewalk_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tilewalk ok" in out.stdout
