"""The flow-options planner (netgauze_amd/csrc/ngz_options_plan.cpp) as a stand-alone program built
with g++ -fsanitize=address,undefined (tests/native/options_plan_check.cpp): it plans seeded template
records, whole and truncated, and its plans must equal the restatement's."""
import os
import random
import shutil
import subprocess

import pytest

import options_ref as OR
from test_options_plan import ipfix_options, nf9_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASS = {"none": 0, "sampling": 1, "interface": 2, "vrf": 3, "unclassified": 4}
OUTCOME = {"ops": 0, "not_options": 1, "conversion_error": 2, "missing_required_fields": 3}
POOL = [10, 14, 34, 50, 82, 83, 90, 141, 144, 210, 234, 235, 236, 302, 305, 306, 311, 1, 2]


def line(plan):
    out = "P 0 %d %d %d %d" % (CLASS[plan["class"]], OUTCOME[plan["outcome"]], len(plan["ops"]), plan["id_equal"])
    for op in plan["ops"]:
        out += " |" + "".join(" s%d.%d.%d@%d" % (r + (s,)) for r, s in zip(op["scope"], op["scope_src"]))
        out += "".join(" f%d.%d.%d@%d" % (r + (s,)) for r, s in zip(op["fields"], op["fields_src"]))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_planner_under_asan_and_ubsan_matches_the_restatement(tmp_path):
    exe = str(tmp_path / "options_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "netgauze_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "options_plan_check.cpp"),
                           os.path.join(ROOT, "netgauze_amd", "csrc", "ngz_options_plan.cpp"), "-o", exe])
    rng = random.Random(0x4F505453)
    script, expect = [], []
    for _ in range(600):
        proto = rng.choice([10, 10, 9])
        fields = [(rng.choice([0, 0, 0, 3746, 9]), rng.choice(POOL)) for _ in range(rng.randrange(0, 6))]
        if proto == 10:
            scope = [(rng.choice([0, 0, 0, 9]), rng.choice(POOL)) for _ in range(rng.randrange(1, 5))]
            rec = ipfix_options(scope, fields)
        else:
            scope = [(0, rng.choice([1, 1, 2, 2, 3, 3, 4, 5, 77])) for _ in range(rng.randrange(1, 4))]
            rec = nf9_options(scope, fields)
        script.append("T %d 1 %s" % (proto, rec.hex()))
        expect.append(line(OR.plan(scope, fields, proto)))
        cut = rec[:rng.randrange(0, len(rec))]  # a truncated record: refused, and never read past its end
        script.append("T %d 1 %s" % (proto, cut.hex() or "-"))
        expect.append("P -1")
    path = tmp_path / "script.txt"
    path.write_text("\n".join(script) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.splitlines() == expect
    assert sum(1 for ln in expect if " | " in ln) > 300
