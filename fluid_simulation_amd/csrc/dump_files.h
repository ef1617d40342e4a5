// dump_files.h -- the file side of the frame writer (dump.h), plain C++ without HIP so that it builds and runs on any host
// (tests/test_dump_files_cpu.py drives it as a stand-alone program, once under ASan + UBSan and once under TSan).
//
// A frame is five float32 arrays, one per file, in the order data, obs, v_x, v_y, v_z (simulation.cpp:140-148).  stdio
// buffers a write that is smaller than its buffer, so a full disk shows in fwrite only for large frames; for a small one, and
// for the tail of any frame, it shows in the fflush that follows.  Both report it here: a frame counts as written only once
// flush_files has returned 0 after it.
#pragma once
#include <cstddef>
#include <cstdio>
#include <string>
#include <thread>

namespace fs {

constexpr int DUMP_NFILE = 5;

// Writes the DUMP_NFILE arrays of `nloc` floats that lie one after the other at `host`, array k to fp[k]: at byte `offset`
// of each file, or at the file's position if offset < 0 (appending).  Returns 0, or -1 with *err set.
inline int write_frame(FILE** fp, const float* host, long nloc, long offset, std::string* err)
{
    // the five files are independent: one short-lived thread each (a single fwrite stream into the page cache tops out
    // near 6 GB/s, far below the PCIe copy)
    const char* errs[DUMP_NFILE] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    std::thread workers[DUMP_NFILE];
    for (int k = 0; k < DUMP_NFILE; ++k)
        workers[k] = std::thread([&, k] {
            if (offset >= 0 && fseek(fp[k], offset, SEEK_SET) != 0) errs[k] = "fseek failed";
            else if (fwrite(host + (size_t)k * nloc, sizeof(float), (size_t)nloc, fp[k]) != (size_t)nloc)
                errs[k] = "short write to a frame dump file";
        });
    int rc = 0;
    for (int k = 0; k < DUMP_NFILE; ++k) {
        workers[k].join();
        if (errs[k] && rc == 0) { *err = errs[k]; rc = -1; }
    }
    return rc;
}

// Hands what stdio still holds of the files to the operating system.  Every file is flushed even after one has failed;
// returns 0, or -1 with *err set.
inline int flush_files(FILE** fp, std::string* err)
{
    int rc = 0;
    for (int k = 0; k < DUMP_NFILE; ++k)
        if (fp && fp[k] && fflush(fp[k]) != 0 && rc == 0) { *err = "flushing a frame dump file failed"; rc = -1; }
    return rc;
}

// Closes the files that are open and clears their entries; returns 0, or -1 with *err set if a close reported a failure
// (what stdio still held did not reach the file).
inline int close_files(FILE** fp, std::string* err)
{
    int rc = 0;
    for (int k = 0; k < DUMP_NFILE; ++k) {
        if (!fp[k]) continue;
        if (fclose(fp[k]) != 0 && rc == 0) { *err = "closing a frame dump file failed"; rc = -1; }
        fp[k] = nullptr;
    }
    return rc;
}

}  // namespace fs
