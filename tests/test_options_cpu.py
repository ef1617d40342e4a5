"""The value parsers of fs_set_option (csrc/options.h), on the host: a driver built over the header as it is parses a list
of texts, and the test compares every answer with a restatement in Python of the C library's rules for strtol (base 10),
strtod and strtoull (base 0) plus the header's own conditions -- nothing after the number, the range, finiteness, no
leading '-' for the seed.  The texts: a fixed list of the edges (blanks, signs, other notations, the bounds of the ranges
in use and their neighbours, numbers too long for the type) and seeded random strings over the alphabet numbers are
written in.  The same driver is built once more with AddressSanitizer and UBSan as a stand-alone program and run over the
list.  Last, the fixture tests/test_gpu_options.py replays must know every option the source knows."""
import json
import math
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid_simulation_amd", "csrc")
LONG_MAX, U64_MAX = (1 << 63) - 1, (1 << 64) - 1
SPACE = " \t\n\v\f\r"

# stdin: one request per line, the text in hex (it may be empty or hold blanks) --
#   "int LO HI TEXT", "list LO HI MAX TEXT", "real LEAST TEXT", "u64 TEXT", "word W1,W2,.. TEXT"
# stdout: "-" for a refusal, else the value(s); "word" prints the index, -1 for none
DRIVER = r'''
#include "options.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static std::string unhex(const char* h)
{
    std::string s;
    if (!std::strcmp(h, ".")) return s;
    for (; h[0] && h[1]; h += 2) {
        unsigned v = 0;
        std::sscanf(h, "%2x", &v);
        s.push_back((char)v);
    }
    return s;
}

int main()
{
    char op[16], a[4096], b[64], c[64], d[64];
    while (std::scanf("%15s", op) == 1) {
        if (!std::strcmp(op, "int")) {
            long lo, hi, n = -777;
            if (std::scanf("%ld %ld %4095s", &lo, &hi, a) != 3) return 2;
            if (fs::parse_int(unhex(a).c_str(), lo, hi, &n)) std::printf("%ld\n", n);
            else if (n != -777) return 3;                       // a refusal leaves the value alone
            else std::printf("-\n");
        } else if (!std::strcmp(op, "list")) {
            long lo, hi;
            int max, count = -777;
            if (std::scanf("%ld %ld %d %4095s", &lo, &hi, &max, a) != 4) return 2;
            std::vector<int> out((size_t)max + 1, -777);        // one more than it may fill
            if (fs::parse_int_list(unhex(a).c_str(), lo, hi, max, out.data(), &count)) {
                std::printf("%d:", count);
                for (int i = 0; i < count; ++i) std::printf(" %d", out[(size_t)i]);
                std::printf("\n");
            } else if (count != -777) return 3;
            else std::printf("-\n");
            if (out[(size_t)max] != -777) return 4;
        } else if (!std::strcmp(op, "real")) {
            double least, x = -777.0;
            if (std::scanf("%63s %4095s", b, a) != 2) return 2;
            least = std::strtod(b, nullptr);
            if (fs::parse_real(unhex(a).c_str(), least, &x)) std::printf("%.17g\n", x);
            else if (x != -777.0) return 3;
            else std::printf("-\n");
        } else if (!std::strcmp(op, "u64")) {
            uint64_t x = 777;
            if (std::scanf("%4095s", a) != 1) return 2;
            if (fs::parse_u64(unhex(a).c_str(), &x)) std::printf("%llu\n", (unsigned long long)x);
            else if (x != 777) return 3;
            else std::printf("-\n");
        } else if (!std::strcmp(op, "word")) {
            if (std::scanf("%63s %63s %63s %4095s", b, c, d, a) != 4) return 2;
            std::printf("%d\n", fs::keyword(unhex(a).c_str(), {b, c, d}));
        } else {
            return 2;
        }
    }
    return 0;
}
'''


def compile_driver(d, name, flags):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / name
    subprocess.run([cxx, "-std=c++17", "-Wall", "-I", CSRC, str(src), "-o", str(exe)] + flags, check=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("options"), "driver", ["-O2"])


# ---- the C library's rules, restated ------------------------------------------------------------------------------------
def c_strtol10(text):
    """(value saturated to a long, characters consumed); consumed 0 = no number"""
    m = re.match(r"[ \t\n\v\f\r]*([+-]?)(\d+)", text)
    if not m:
        return 0, 0
    v = int(m.group(2)) * (-1 if m.group(1) == "-" else 1)
    return max(-LONG_MAX - 1, min(LONG_MAX, v)), m.end()


def c_strtod(text):
    """(value, characters consumed): decimal and hexadecimal floating notation, inf / infinity, nan / nan(...)"""
    m = re.match(r"[ \t\n\v\f\r]*([+-]?)", text)
    sign, rest, at = (-1.0 if m.group(1) == "-" else 1.0), text[m.end():], m.end()
    w = re.match(r"(?i)(infinity|inf)", rest)
    if w:
        return sign * math.inf, at + w.end()
    w = re.match(r"(?i)nan(\([0-9a-z_]*\))?", rest)
    if w:
        return math.nan, at + w.end()
    w = re.match(r"0[xX]([0-9a-fA-F]+\.?[0-9a-fA-F]*|\.[0-9a-fA-F]+)([pP][+-]?\d+)?", rest)
    if w:
        try:
            return sign * float.fromhex(w.group(0)), at + w.end()
        except OverflowError:
            return sign * math.inf, at + w.end()
    w = re.match(r"(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?", rest)
    if w:
        return sign * float(w.group(0)), at + w.end()            # float(): correctly rounded, inf past the range, as strtod
    return 0.0, 0


def c_strtoull0(text):
    """(value, characters consumed, out of range)"""
    m = re.match(r"[ \t\n\v\f\r]*([+-]?)", text)
    neg, rest, at = m.group(1) == "-", text[m.end():], m.end()
    w = re.match(r"0[xX]([0-9a-fA-F]+)", rest)
    if w:
        v = int(w.group(1), 16)
    else:
        w = re.match(r"0[0-7]*", rest) or re.match(r"[1-9]\d*", rest)
        if not w:
            return 0, 0, False
        v = int(w.group(0), 8 if w.group(0)[0] == "0" else 10)
    if v > U64_MAX:
        return U64_MAX, at + w.end(), True
    return ((1 << 64) - v) & U64_MAX if neg else v, at + w.end(), False


def model_int(text, lo, hi):
    v, used = c_strtol10(text)
    return str(v) if used and used == len(text) and lo <= v <= hi else "-"


def model_list(text, lo, hi, most):
    out, q = [], 0
    while q < len(text):
        v, used = c_strtol10(text[q:])
        end = q + used
        follows = text[end:end + 1]
        if not used or follows not in (",", "") or (follows == "," and end + 1 == len(text)) or not lo <= v <= hi or len(out) == most:
            return "-"
        out.append(v)
        q = end + 1 if follows else end
    return "%d:%s" % (len(out), "".join(" %d" % v for v in out))


def model_real(text, least):
    v, used = c_strtod(text)
    return "%.17g" % v if used and used == len(text) and math.isfinite(v) and v >= least else "-"


def model_u64(text):
    v, used, erange = c_strtoull0(text)
    return str(v) if used and used == len(text) and not erange and not text.startswith("-") else "-"


# ---- the texts ------------------------------------------------------------------------------------------------------------
RANGES = [(0, 1048576), (0, 65536), (0, 4194304), (1, 1 << 30), (0, 1 << 30), (1, 8)]
FIXED = ["", " 5", "+5", "5 ", "5x", "-0", "-1", "0x10", "1e3", "99999999999999999999", "-99999999999999999999", "nan", "inf",
         "-0.0", "1e400", "18446744073709551615", "18446744073709551616", "-1", " ", "\t7", "\n7", "7\n", "+", "-", "+-5", "--5", "5.",
         ".5", ".", "5.0", "0", "00", "007", "08", "010", "0x", "0X1F", "0x1p4", "0x1p", "0x.8", "1e", "1e+", "1e-400", "1e308", "1.8e308",
         "-1e400", "INF", "Infinity", "infinit", "-inf", "NaN", "nan(1)", "nan(", "-nan", "9223372036854775807", "9223372036854775808",
         "-9223372036854775808", "-9223372036854775809", " -1", " +1", "1,2", "1,", ",1", "1,,2", "1, 2", "1 ,2", "1,2,3,4,5,6,7,8",
         "1,2,3,4,5,6,7,8,1", "8,8,8", "0.25", "0.75", "1.0", "0.99999999999999989", "auto", "0,0,0", "\x7f5", "5\x80"]
for lo_, hi_ in RANGES:
    FIXED += [str(v) for v in (lo_ - 1, lo_, lo_ + 1, hi_ - 1, hi_, hi_ + 1)]
ALPHABET = " +-0123456789.eExXabfnipNI,\t()"
WORDS = ("auto", "0", "1")


def texts(seed=11, n=1500):
    rng = random.Random(seed)
    out = list(dict.fromkeys(FIXED))
    for _ in range(n):
        k = rng.choice((1, 2, 2, 3, 3, 4, 5, 6, 8, 20))
        if rng.random() < 0.5:                                 # number-like: a prefix, digits, a tail
            t = rng.choice(["", "", " ", "+", "-", "0x", "0", "."]) + "".join(rng.choice("0123456789") for _ in range(k)) + \
                rng.choice(["", "", "", " ", ",", "x", "e5", "e-3", ".5", ",3", "p2"])
        else:
            t = "".join(rng.choice(ALPHABET) for _ in range(k))
        out.append(t)
    return out


def requests_and_model(ts):
    req, want = [], []
    for t in ts:
        hx = t.encode("latin-1").hex() or "."
        for lo, hi in RANGES:
            req.append("int %d %d %s" % (lo, hi, hx))
            want.append(model_int(t, lo, hi))
        req.append("list 1 8 8 %s" % hx)
        want.append(model_list(t, 1, 8, 8))
        req.append("list 1 4096 3 %s" % hx)
        want.append(model_list(t, 1, 4096, 3))
        for least in (0.0, 1.0):
            req.append("real %r %s" % (least, hx))
            want.append(model_real(t, least))
        req.append("u64 %s" % hx)
        want.append(model_u64(t))
        req.append("word %s %s" % (",".join(WORDS).replace(",", " "), hx))
        want.append(str(WORDS.index(t) if t in WORDS else -1))
    return req, want


def check(exe, ts):
    req, want = requests_and_model(ts)
    got = subprocess.run([exe], input="\n".join(req) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(want)
    wrong = [(r, g, w) for r, g, w in zip(req, got, want) if g != w]
    assert not wrong, wrong[:10]
    return want


def test_parsers_agree_with_the_c_rules(driver):
    ts = texts()
    want = check(driver, ts)
    per = len(want) // len(ts)
    # the list is no row of refusals: each parser accepts and refuses often enough to mean something
    for col in range(per - 1):
        taken = sum(w != "-" for w in want[col::per])
        assert 20 <= taken <= len(ts) - 20, (col, taken)


def test_the_model_knows_the_edges():
    """the restated rules on texts whose answer is known without them"""
    assert model_int(" 5", 0, 9) == "5" and model_int("+5", 0, 9) == "5" and model_int("-0", 0, 9) == "0"
    assert [model_int(t, 0, 9) for t in ("", "5 ", "5x", "-1", "0x10", "1e3", "10", "99999999999999999999")] == ["-"] * 8
    assert model_int("1048576", 0, 1 << 20) == "1048576" and model_int("1048577", 0, 1 << 20) == "-"
    assert model_real("1e3", 0.0) == "1000" and model_real("-0.0", 0.0) == "-0" and model_real(" 2.5", 1.0) == "2.5"
    assert [model_real(t, 0.0) for t in ("nan", "inf", "1e400", "-1", "", "2.5x", "0x")] == ["-"] * 7
    assert model_real("0x1p4", 0.0) == "16" and model_real("0.75", 1.0) == "-" and model_real("1e-400", 0.0) == "0"
    assert model_u64("18446744073709551615") == str(U64_MAX) and model_u64("18446744073709551616") == "-"
    assert model_u64("-1") == "-" and model_u64(" -1") == str(U64_MAX) and model_u64("0x10") == "16" and model_u64("010") == "8"
    assert [model_u64(t) for t in ("", "08", "0x", "5 ", "1e3")] == ["-"] * 5
    assert model_list("", 1, 8, 8) == "0:" and model_list("1,2", 1, 8, 8) == "2: 1 2"
    assert [model_list(t, 1, 8, 8) for t in ("1,", ",1", "1,,2", "9", "0", "1 ,2", "1,2,3,4,5,6,7,8,1")] == ["-"] * 7
    assert model_list("1, 2", 1, 8, 8) == "2: 1 2"               # strtol skips the blank before a number


def test_parsers_under_sanitizers(tmp_path):
    exe = compile_driver(tmp_path, "driver_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    check(exe, texts())


def test_fixture_covers_every_option_of_the_source():
    """every key of the `k == "..."` chain of fs_set_option has at least three calls among the recorded replies"""
    src = open(os.path.join(CSRC, "fluidsim.cpp")).read()
    body = src[src.index("int fs_set_option("):src.index("int fs_get_int(")]
    keys = set(re.findall(r'\bk == "([^"]+)"', body))
    assert len(keys) >= 63 and {"precision", "inflow_seed", "monitor_stations", "two_sweep_kernel"} <= keys
    with open(os.path.join(ROOT, "tests", "golden", "option_replies.json")) as f:
        doc = json.load(f)
    calls = {}
    for opt in doc["options"]:
        assert len(opt["calls"]) == len(opt["replies"])
        for c in opt["calls"]:                                 # a call is its value alone where its key is the option's name
            key = opt["name"] if isinstance(c, str) else c[0]
            calls[key] = calls.get(key, 0) + 1
    assert not {k: calls.get(k, 0) for k in keys if calls.get(k, 0) < 3}
    assert sorted(doc["logs"]) == sorted(["force", "body_force", "residual", "probe", "monitor", "image", "volume", "tracer"])
