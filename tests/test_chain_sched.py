"""ops/csrc/chain_sched.h -- which row tiles a block of the persistent conv_chain form takes -- checked
on the host: every tile is taken exactly once for tile counts 0..2000 and grids 1..520
(tests/native/chain_sched_check.cpp, built with -fsanitize=undefined)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mlmicroservicetemplate_amd", "ops", "csrc")


@pytest.mark.timeout(300)
def test_chain_schedule_takes_every_tile_once(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "chain_sched_check")
    build = subprocess.run([cxx, "-std=c++17", "-O2", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                            "-I", CSRC, os.path.join(HERE, "native", "chain_sched_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert run.returncode == 0 and "chain_sched: ok" in run.stdout, (run.stdout[-2000:], run.stderr[-2000:])
