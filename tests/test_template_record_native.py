"""The template-record walker the per-template planners share (netgauze_amd/csrc/ngz_template_record.h)
as a stand-alone program built with g++ -fsanitize=address,undefined
(tests/native/template_record_check.cpp): it walks seeded records of the four kinds, whole and cut at
every length, each from a heap copy of exactly its length.  A whole record yields the fields that were
packed; a cut one is refused, and no byte at or past its length is read."""
import os
import random
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSED = "R -1"


def spec(pen, ie, length):
    if pen:
        return struct.pack(">HHI", 0x8000 | ie, length, pen)
    return struct.pack(">HH", ie, length)


def template(tid, fields):  # IPFIX and NetFlow v9: id, field count
    return struct.pack(">HH", tid, len(fields)) + b"".join(spec(*f) for f in fields)


def ipfix_options(tid, scope, fields):  # id, field count (scope included), scope field count
    return struct.pack(">HHH", tid, len(scope) + len(fields), len(scope)) + b"".join(spec(*f) for f in scope + fields)


def nf9_options(tid, scope, fields, short=0, pad=b""):
    """id, scope bytes, option bytes.  Scope codes are raw (no enterprise number follows, whatever the top
    bit).  `short`: the option length understates the last specifier by that many bytes; `pad`: bytes
    after the specifiers."""
    sb = b"".join(struct.pack(">HH", code, length) for _pen, code, length in scope)
    ob = b"".join(spec(*f) for f in fields)
    return struct.pack(">HHH", tid, len(sb), len(ob) - short) + sb + ob + pad


def fields_line(scope, fields):
    return "F" + "".join(" s%d.%d.%d" % f for f in scope) + "".join(" f%d.%d.%d" % f for f in fields)


def nf9_options_expect(rec):
    """What a NetFlow v9 options record of these bytes yields, from the byte lengths in its header: the
    specifiers that begin before the end those lengths give, each read whole, or the refusal where the
    record does not hold that end or such a specifier."""
    if len(rec) < 6:
        return REFUSED
    scope_end = 6 + struct.unpack_from(">H", rec, 2)[0]
    end = scope_end + struct.unpack_from(">H", rec, 4)[0]
    if end > len(rec):
        return REFUSED
    pos, out = 6, "F"
    while pos < end:
        if pos + 4 > len(rec):
            return REFUSED
        code, length = struct.unpack_from(">HH", rec, pos)
        scope = pos < scope_end
        pos += 4
        pen = 0
        if not scope and code & 0x8000:
            if pos + 4 > len(rec):
                return REFUSED
            pen, = struct.unpack_from(">I", rec, pos)
            pos += 4
            code &= 0x7FFF
        out += " %s%d.%d.%d" % ("s" if scope else "f", pen, code, length)
    return out


def records(rng):
    """(proto, options, record bytes, expected line) of seeded records: every kind with no field, with
    enterprise fields, and options records whose fields are all scope fields."""
    def some(n, pens=(0, 0, 0, 9, 3746, 0xFFFFFFFF)):
        return [(rng.choice(pens), rng.randrange(1, 0x8000), rng.choice([0, 1, 2, 4, 8, 16, 0xFFFF])) for _ in range(n)]

    out = []
    for i in range(320):
        kind = i % 4
        tid = rng.randrange(256, 0x10000)
        empty = i < 8
        n = 0 if empty else rng.randrange(0, 7)
        if kind == 0 or kind == 2:
            fields = some(n)
            out.append((10 if kind == 0 else 9, 0, template(tid, fields), fields_line([], fields)))
        elif kind == 1:
            scope = some(0 if empty else rng.randrange(0, 4))
            fields = [] if i % 8 == 1 else some(n)  # every other one: scope count == field count
            out.append((10, 1, ipfix_options(tid, scope, fields), fields_line(scope, fields)))
        else:
            scope = [(0, rng.choice([1, 2, 3, 4, 5, 0x8001, 0xFFFF]), rng.choice([0, 2, 4])) for _ in range(0 if empty else rng.randrange(0, 4))]
            fields = some(n)
            short = rng.randrange(0, 4) if fields and i % 3 == 0 else 0
            pad = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 6))) if i % 5 == 0 else b""
            rec = nf9_options(tid, scope, fields, short, pad)
            out.append((9, 1, rec, fields_line(scope, fields)))
            assert nf9_options_expect(rec) == out[-1][3]
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_walker_under_asan_and_ubsan_yields_the_packed_fields_and_refuses_every_cut(tmp_path):
    exe = str(tmp_path / "template_record_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "netgauze_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "template_record_check.cpp"), "-o", exe])
    rng = random.Random(0x544D504C)
    script, expect = [], []
    for proto, options, rec, line in records(rng):
        script.append("T %d %d %s" % (proto, options, rec.hex()))
        expect.append(line)
        for cut in range(len(rec)):
            # count-driven kinds: a proper prefix cuts the header or a specifier the counts promise
            script.append("T %d %d %s" % (proto, options, rec[:cut].hex() or "-"))
            expect.append(nf9_options_expect(rec[:cut]) if (proto, options) == (9, 1) else REFUSED)
    path = tmp_path / "script.txt"
    path.write_text("\n".join(script) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.splitlines()
    assert len(got) == len(expect)
    bad = [(s, g, e) for s, g, e in zip(script, got, expect) if g != e]
    assert not bad, bad[:3]
    whole = [e for e in expect if e != REFUSED]
    assert len(whole) > 320 and sum(1 for e in whole if e == "F") >= 8  # cuts of padded NFv9 options records walk too
    assert sum(1 for e in whole if any(t in e for t in (" f3746.", " s3746.", " f9.", " s9."))) > 100
