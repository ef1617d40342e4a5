// options.h -- how fs_set_option reads a value: a bounded integer, a finite real with a lower bound, the unsigned 64-bit
// seed, and a keyword out of a list.  Each returns whether the text is a value of that kind; what an option does with it, and
// the message of a refusal, is the option's own business.  Plain C++ without HIP, so that tests/test_options_cpu.py can run
// it against a model on the CPU.  Internal to libfluidsim.so (static: the library exports none of it).
#pragma once

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

namespace fs {

// A decimal integer in lo .. hi, by strtol's rules: blanks and a sign may lead, nothing may follow the digits.  A number too
// long for a long saturates there, and so falls outside every range in use.
static inline bool parse_int(const char* value, long lo, long hi, long* out)
{
    char* end = nullptr;
    const long n = strtol(value, &end, 10);
    if (end == value || *end || n < lo || n > hi) return false;
    *out = n;
    return true;
}

// A list "x1,x2,..." of at most `max` such integers into out[]; "" is the empty list, and a comma is followed by a number.
static inline bool parse_int_list(const char* value, long lo, long hi, int max, int* out, int* count)
{
    int n = 0;
    for (const char* q = value; *q;) {
        char* end = nullptr;
        const long x = strtol(q, &end, 10);
        if (end == q || (*end != ',' && *end != '\0') || (*end == ',' && end[1] == '\0') || x < lo || x > hi || n == max) return false;
        out[n++] = (int)x;
        q = *end ? end + 1 : end;
    }
    *count = n;
    return true;
}

// A finite real >= least, by strtod's rules ("1e3" and "0x1p4" are numbers, "inf" and "nan" are not finite).
static inline bool parse_real(const char* value, double least, double* out)
{
    char* end = nullptr;
    const double x = strtod(value, &end);
    if (end == value || *end || !std::isfinite(x) || !(x >= least)) return false;
    *out = x;
    return true;
}

// An unsigned 64-bit number in C's notation (base 0: decimal, 0x.., 0..).  strtoull would take "-1" for 2^64 - 1: a text
// that begins with '-' is refused, and so is one past 2^64 - 1.
static inline bool parse_u64(const char* value, uint64_t* out)
{
    char* end = nullptr;
    errno = 0;
    const unsigned long long x = strtoull(value, &end, 0);
    if (end == value || *end || errno || value[0] == '-') return false;
    *out = (uint64_t)x;
    return true;
}

// the place of `value` in `words`, -1 if it is none of them
static inline int keyword(const char* value, std::initializer_list<const char*> words)
{
    int i = 0;
    for (const char* w : words) {
        if (!strcmp(value, w)) return i;
        ++i;
    }
    return -1;
}

}  // namespace fs
