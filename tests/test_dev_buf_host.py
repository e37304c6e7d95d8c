"""csrc/dev_buf.hpp on its own: tests/dev_buf_host_main.cpp includes only that header, brings its own hip_check (which counts
the calls) and checks the buffer's contract in a form that holds whether an allocation succeeds or fails.  Here the program
runs with every device hidden, so it opens no GPU: each allocation fails and the failure half of the contract is what runs --
nothing left behind after a failure, a retry on the next request, no call when the capacity suffices.
test_gpu_workspace_regrow.py runs the same program with a device for the success half."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openkeonspark_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "dev_buf_host_main.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build_and_run(tmp_path, hide_devices):
    """-> (checks, failed, hip_check calls, allocations that succeeded) as the program reports them"""
    exe = str(tmp_path / "dev_buf_host")
    cc = subprocess.run([HIPCC, "-std=c++17", "-O1", "-Wall", "-I", CSRC, SRC, "-ldl", "-o", exe], capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stderr
    env = dict(os.environ)
    if hide_devices:
        env["HIP_VISIBLE_DEVICES"] = "-1"
    run = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"checks (\d+) failed (\d+) calls (\d+) allocated (\d+)", run.stdout)
    assert m, run.stdout
    return tuple(int(v) for v in m.groups())


def test_dev_buf_contract_without_a_device(tmp_path):
    checks, failed, calls, _ = build_and_run(tmp_path, hide_devices=True)
    assert failed == 0 and checks >= 20 and calls > 0
