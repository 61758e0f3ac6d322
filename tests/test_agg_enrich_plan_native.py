"""The aggregation-over-enrichment planner (netgauze_amd/csrc/ngz_agg_enrich_plan.cpp) as a stand-alone
program built with g++ -fsanitize=address,undefined (tests/native/agg_enrich_plan_check.cpp): it
resolves seeded queries over exact-size heap copies of the field and column lists, and its
resolutions must equal the restatement's (tests/test_agg_enrich_plan.py's expect)."""
import os
import random
import shutil
import subprocess

import pytest

from netgauze_amd import _lib
from test_agg_enrich_plan import expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IES = [(0, 10), (0, 82), (0, 234), (3746, 7), (0, 1)]


def line(res):
    cand = res.get("candidates", [])
    return "R 0 %d %d %d %d %d %d |%s" % (res["kind"], res["dropped"], res.get("own_field", 0), len(cand),
                                          res.get("ordinal", 0), res.get("writer_after", False),
                                          "".join(" %d" % c for c in cand))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_planner_under_asan_and_ubsan_matches_the_restatement(tmp_path):
    exe = str(tmp_path / "agg_enrich_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "netgauze_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "agg_enrich_plan_check.cpp"),
                           os.path.join(ROOT, "netgauze_amd", "csrc", "ngz_agg_enrich_plan.cpp"), "-o", exe])
    rng = random.Random(0x41474745)
    script, want = [], []
    for _ in range(800):
        fields = [rng.choice(IES) + (int(rng.random() < 0.03),) for _ in range(rng.randrange(0, 7))]
        cols = sorted({rng.choice(IES) + (rng.randrange(0, 4),) for _ in range(rng.choice([0, 1, 2, 5, 32]))})
        ref = rng.choice(IES) + (rng.choice([0, 0, 1, 2, 3, 40, 65535]),)
        script.append("Q %d %s %d %s %d %d %d" % (len(fields), " ".join("%d %d %d" % f for f in fields), len(cols),
                                                  " ".join("%d %d %d" % c for c in cols), ref[0], ref[1], ref[2]))
        want.append(line(expect(fields, cols, ref)))
    # more added columns than the aggregation takes: refused before any is read
    script.append("Q 0  33 %s 0 82 0" % " ".join("0 82 %d" % i for i in range(33)))
    want.append("R %d" % _lib.NGZ_E_LIMIT)
    path = tmp_path / "script.txt"
    path.write_text("\n".join(script) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.splitlines() == want
    assert sum(1 for ln in want if ln.startswith("R 0 2")) > 100
