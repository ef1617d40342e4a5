"""The file side of the frame writer (csrc/dump_files.h), on the host: a driver built over the header as it is opens five
files, writes frames of a known pattern by a script and prints what write_frame and flush_files returned; the test compares
the files with the bytes the script stands for.  On a full device (/dev/full) a frame that did not reach its file must be
reported by the write or by the flush that follows it.  The same driver is built once with AddressSanitizer and UBSan and,
where the compiler has its runtime, once with ThreadSanitizer, and run stand-alone over the append and offset scripts."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fluid_simulation_amd", "csrc")
NAMES = ("data.bin", "obs.bin", "v_x.bin", "v_y.bin", "v_z.bin")
SIZES = (480, 1023, 1024, 5000)         # floats per field: one 8x6x4 field; one short of stdio's buffer; the buffer; beyond it

# argv: the directory, then the mode of fopen.  stdin: one operation per line -- "frame TAG NLOC OFFSET" (write_frame of a
# frame whose field k holds the floats pattern(TAG, k, START + i): OFFSET is a byte offset in each file or -1 to append, and
# START = 0 unless a fourth number follows), "flush", "close" (fclose of all five).  Each prints one line: the operation and
# its return value (close: how many fclose calls failed).
DRIVER = r'''
#include "dump_files.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static float pattern(long tag, int k, long i) { return (float)(tag * 1000003L + k * 100003L + i); }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    static const char* const names[fs::DUMP_NFILE] = {"data.bin", "obs.bin", "v_x.bin", "v_y.bin", "v_z.bin"};
    FILE* fp[fs::DUMP_NFILE];
    for (int k = 0; k < fs::DUMP_NFILE; ++k) {
        const std::string path = std::string(argv[1]) + "/" + names[k];
        fp[k] = std::fopen(path.c_str(), argv[2]);
        if (!fp[k]) { std::printf("open %d failed\n", k); return 3; }
    }
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char op[16];
        long tag = 0, nloc = 0, offset = -1, start = 0;
        const int got = std::sscanf(line, "%15s %ld %ld %ld %ld", op, &tag, &nloc, &offset, &start);
        if (got < 1) continue;
        std::string err;
        if (!std::strcmp(op, "frame") && got >= 4) {
            std::vector<float> host((size_t)nloc * fs::DUMP_NFILE);
            for (int k = 0; k < fs::DUMP_NFILE; ++k)
                for (long i = 0; i < nloc; ++i) host[(size_t)k * nloc + i] = pattern(tag, k, start + i);
            std::printf("frame %d %s\n", fs::write_frame(fp, host.data(), nloc, offset, &err), err.c_str());
        } else if (!std::strcmp(op, "flush")) {
            std::printf("flush %d %s\n", fs::flush_files(fp, &err), err.c_str());
        } else if (!std::strcmp(op, "close")) {
            std::printf("close %d %s\n", fs::close_files(fp, &err), err.c_str());
        } else {
            return 2;
        }
    }
    std::string err;
    fs::close_files(fp, &err);
    return 0;
}
'''


def pattern(tag, k, start, n):
    return (tag * 1000003 + k * 100003 + start + np.arange(n, dtype=np.int64)).astype(np.float32)


def compile_driver(d, name, flags):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / name
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", CSRC, str(src), "-o", str(exe)] + flags,
                       capture_output=True, text=True)
    if r.returncode != 0 and "-fsanitize=thread" in flags and ("tsan" in r.stderr or "-fsanitize=thread" in r.stderr):
        pytest.skip("no ThreadSanitizer runtime for this compiler")
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("dump_files"), "driver", ["-O2"])


def run(exe, d, mode, script):
    text = "".join(" ".join(str(v) for v in op) + "\n" for op in script)
    out = subprocess.run([exe, str(d), mode], input=text, check=True, capture_output=True, text=True, timeout=60).stdout
    replies = [ln.split(None, 2) for ln in out.splitlines()]
    assert [r[0] for r in replies] == [op[0] for op in script], out
    return [int(r[1]) for r in replies]


def files(d):
    return [open(os.path.join(str(d), n), "rb").read() for n in NAMES]


def append_script():
    script, want = [], [b""] * 5
    for tag, n in enumerate(SIZES + SIZES[::-1]):
        script.append(("frame", tag, n, -1))
        want = [w + pattern(tag, k, 0, n).tobytes() for k, w in enumerate(want)]
        if tag % 3 == 2:
            script.append(("flush",))
    return script + [("flush",), ("close",)], want


def check_append(exe, d):
    script, want = append_script()
    assert run(exe, d, "wb", script) == [0] * len(script)
    assert files(d) == want


PLANE, DEPTH, FRAMES = 7 * 9, 10, 2                   # an 5x7x8 grid: planes of 63 cells, 10 planes per frame
RANKS = ((0, 4), (4, 7), (7, 10))                     # the plane ranges [lo, hi) of three slab ranks


def check_offset(exe, tmp):
    """three ranks write their planes of two frames at frames * frame_cells + plane * lo, in a shuffled order, each through
    its own open files, as the slab ranks of Engine::dump_frame do; a single writer appends the same frames in order"""
    one, many = tmp / "one", tmp / "many"
    one.mkdir()
    many.mkdir()
    frame_cells = PLANE * DEPTH
    script = [("frame", 10 + f, frame_cells, -1) for f in range(FRAMES)] + [("flush",), ("close",)]
    assert run(exe, one, "wb", script) == [0] * len(script)
    assert run(exe, many, "wb", [("close",)]) == [0]                      # the lead rank creates the files
    jobs = [(f, lo, hi) for f in range(FRAMES) for lo, hi in RANKS]
    random.Random(5).shuffle(jobs)
    assert jobs != sorted(jobs)
    per_rank = {r: [("frame", 10 + f, PLANE * (hi - lo), (f * frame_cells + PLANE * lo) * 4, PLANE * lo)
                    for f, lo, hi in jobs if (lo, hi) == r] for r in RANKS}
    for r in (RANKS[2], RANKS[0], RANKS[1]):
        script = []
        for op in per_rank[r]:
            script += [op, ("flush",)]
        assert run(exe, many, "r+b", script + [("close",)]) == [0] * (len(script) + 1)
    want = files(one)
    assert len(want[0]) == FRAMES * frame_cells * 4
    assert want[3] == b"".join(pattern(10 + f, 3, 0, frame_cells).tobytes() for f in range(FRAMES))
    assert files(many) == want


def test_appending(driver, tmp_path):
    check_append(driver, tmp_path)


def test_offset_mode_equals_the_single_writer(driver, tmp_path):
    check_offset(driver, tmp_path)


@pytest.mark.parametrize("nloc", SIZES)
def test_a_full_device_is_reported(driver, tmp_path, nloc):
    """five symlinks to /dev/full: the frame cannot reach its file, so the write or the flush after it must say so"""
    try:
        with open("/dev/full", "wb"):
            pass
    except OSError:
        pytest.skip("/dev/full cannot be opened for writing")
    for n in NAMES:
        os.symlink("/dev/full", str(tmp_path / n))
    wrote, flushed, closed = run(driver, tmp_path, "wb", [("frame", 1, nloc, -1), ("flush",), ("close",)])
    print("nloc %d: write_frame %d, flush_files %d, close_files %d" % (nloc, wrote, flushed, closed))
    assert wrote in (0, -1) and flushed in (0, -1)
    assert wrote == -1 or flushed == -1


def test_under_address_and_ub_sanitizers(tmp_path):
    exe = compile_driver(tmp_path, "driver_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    (tmp_path / "a").mkdir()
    (tmp_path / "o").mkdir()
    check_append(exe, tmp_path / "a")
    check_offset(exe, tmp_path / "o")


def test_under_thread_sanitizer(tmp_path):
    exe = compile_driver(tmp_path, "driver_tsan", ["-O1", "-g", "-fsanitize=thread"])
    (tmp_path / "probe").mkdir()
    r = subprocess.run([exe, str(tmp_path / "probe"), "wb"], input="", capture_output=True, text=True, timeout=60)
    if r.returncode != 0 and "FATAL: ThreadSanitizer" in r.stderr:
        pytest.skip("the ThreadSanitizer runtime cannot start here: " + r.stderr.strip().splitlines()[0])
    (tmp_path / "a").mkdir()
    (tmp_path / "o").mkdir()
    check_append(exe, tmp_path / "a")
    check_offset(exe, tmp_path / "o")
