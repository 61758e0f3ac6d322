"""CPU: the flow output's host side (netgauze_amd/csrc/ngz_output_plan.cpp, no HIP) as a stand-alone program built
with g++ -fsanitize=address,undefined (tests/native/output_plan_check.cpp): config, schema, and the plan of a
template record at every truncated length."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_plan_is_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "output_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "output_plan_check.cpp"),
                           os.path.join(ROOT, "netgauze_amd", "csrc", "ngz_output_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[-6:-1] == ["F0 t6 n0 :", "F1 t1 n1 : 3", "F2 t8 n1 : 4", "F3 t2 n1 : 5", "F4 t6 n1 : 6"]
    assert lines[-1] == "R -21 Invalid FieldConfig for port, reason: Coalesce list cannot be empty"
