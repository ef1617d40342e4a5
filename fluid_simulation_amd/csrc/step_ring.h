// step_ring.h -- the bookkeeping of a per-step log that lives in a ring of `cap` slots: which slot the next record goes
// to, which records are retained, in which order, and which step each belongs to.  The ten logs of the host driver's parts (driver/*.h: forces,
// body forces, residuals, probes, images, tracers, volumes, flow monitor, heat, zones) keep their records in device memory and their books here.  Plain C++
// without HIP, so that tests/test_step_ring_cpu.py can run it against a model on the CPU.  Internal to libfluidsim.so.
#pragma once

#include <cstddef>
#include <vector>

namespace fs {

struct StepRing {
    int cap = 0;                    // slots; 0 = the log is off
    long logged = 0;                // records committed since the reset or the last drain
    std::vector<long> step;         // step number held by each slot
    std::vector<unsigned> tag;      // one word per slot for the log's own use (the residual log: which solves ran)

    struct Run { long first_slot, count; };   // `count` consecutive slots

    void reset(int cap_)
    {
        cap = cap_ > 0 ? cap_ : 0;
        logged = 0;
        step.assign((std::size_t)cap, 0);
        tag.assign((std::size_t)cap, 0u);
    }
    // the slot of the record that is being written (cap > 0)
    long next() const { return logged % cap; }
    // that record is complete
    void commit(long step_no, unsigned tag_ = 0u)
    {
        step[(std::size_t)next()] = step_no;
        tag[(std::size_t)next()] = tag_;
        ++logged;
    }
    long retained() const { return logged < cap ? logged : cap; }
    long dropped() const { return logged - retained(); }   // overwritten since the last drain
    // the i-th retained record, oldest first (0 <= i < retained())
    long slot_of(long i) const { return (dropped() + i) % cap; }
    long step_of(long i) const { return step[(std::size_t)slot_of(i)]; }
    unsigned tag_of(long i) const { return tag[(std::size_t)slot_of(i)]; }
    // the retained records, oldest first, as runs of consecutive slots: one, or two where the ring wraps; returns how many
    int runs(Run out[2]) const
    {
        const long n = retained();
        if (n == 0) return 0;
        const long start = slot_of(0), first = n < cap - start ? n : cap - start;
        out[0] = Run{start, first};
        if (first == n) return 1;
        out[1] = Run{0, n - first};
        return 2;
    }
    // the records have been handed out (or are to be forgotten): the next one is the oldest again, in slot 0
    void drain() { logged = 0; }
};

}  // namespace fs
