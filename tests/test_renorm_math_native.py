"""netgauze_amd/csrc/ngz_renorm_math.h on the host, as a stand-alone program built with
-fsanitize=undefined,float-cast-overflow, against the Python restatement (tests/renorm_ref.py): every
known-answer case, every edge, and 20 000 seeded random parameter sets biased to the edge values."""
import json
import math
import os
import random
import shutil
import subprocess

import pytest

import renorm_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
with open(os.path.join(HERE, "golden", "renorm_kats.json")) as f:
    KATS = json.load(f)
NAME = KATS["ie_ids"]
U32_EDGES = [0, 1, 2, 3, 4, 5, 10, 99, 255, 256, 65535, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
P_EDGES = [0, 1, 1 << 63, 0x7ff8000000000000, 0x7ff0000000000000, 0xfff0000000000000, R.f64_bits(1.0),
           R.f64_bits(math.nextafter(1.0, 2.0)), R.f64_bits(math.nextafter(1.0, 0.0)), R.f64_bits(0.1), R.f64_bits(0.5),
           R.f64_bits(-0.5), R.f64_bits(2.2250738585072014e-308), R.f64_bits(1e-300), R.f64_bits(1.0 / 3.0),
           0x000fffffffffffff]
C_EDGES = [0, 1, 2, 100, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 62), (1 << 63) - 1, 1 << 63, (1 << 63) + 1025,
           (1 << 64) - 2, (1 << 64) - 1]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/native/renorm_math_check.cpp")
    exe = str(tmp_path_factory.mktemp("renorm") / "renorm_math_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "netgauze_amd", "csrc"),
                           os.path.join(HERE, "native", "renorm_math_check.cpp"), "-o", exe])
    return exe


def line_of(params, count):
    """params {IE: value} (311 as f64 bits) -> the checker's input line."""
    present = sum(1 << i for i, ie in enumerate(R.PARAM_IES) if ie in params)
    vals = [params.get(ie, 0) for ie in R.PARAM_IES[:9]]
    return "%d %s %x %d" % (present, " ".join(str(v) for v in vals), params.get(311, 0), count)


def expect(params, count):
    p = dict(params)
    if 311 in p:
        p[311] = R.f64_from_bits(p[311])
    st = R.new_stats()
    k = R.factor(p, st)
    new = count if k is None else R.scale(count, k)
    return "%d %016x %d %d %d %d" % (k is not None, 0 if k is None else R.f64_bits(k), new, k is not None,
                                     st["ie_missing_or_invalid"], st["sampling_algorithm_inferred"])


def cases():
    out = []
    for c in KATS["kats"] + KATS["edges"]:
        params, counts = {}, []
        for n, v in c["input"]:
            ie = NAME[n]
            if ie in R.PARAM_IES:
                params[ie] = (int(v["f64_bits"], 16) if isinstance(v, dict) else R.f64_bits(v)) if ie == 311 else v
            else:
                counts.append(v)
        for cnt in counts or [0]:
            out.append((params, cnt))
    rng = random.Random(0x4E475A52)
    for _ in range(20000):
        params = {}
        for ie in R.PARAM_IES:
            if rng.random() < 0.35:
                if ie == 311:
                    params[ie] = rng.choice(P_EDGES) if rng.random() < 0.6 else R.f64_bits(rng.random())
                elif ie in (35, 49):
                    params[ie] = rng.choice([0, 1, 2, 3, 99, 255])
                elif ie == 304:
                    params[ie] = rng.choice([0, 1, 2, 3, 4, 5, 9, 65535])
                else:
                    params[ie] = rng.choice(U32_EDGES) if rng.random() < 0.6 else rng.getrandbits(32)
        out.append((params, rng.choice(C_EDGES) if rng.random() < 0.6 else rng.getrandbits(rng.choice([8, 32, 53, 64]))))
    return out


def test_math_header_agrees_with_the_restatement(checker):
    cs = cases()
    assert len(cs) > 20000
    text = "\n".join(line_of(p, c) for p, c in cs) + "\n"
    run = subprocess.run([checker], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.splitlines()
    assert len(got) == len(cs)
    for (p, c), g in zip(cs, got):
        assert g == expect(p, c), (p, c, g, expect(p, c))
