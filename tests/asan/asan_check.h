// What the host-side AddressSanitizer drivers share: the CHECK macro and its counters, fake device
// pointers, and the closing "N checks, M failed" line the CPU tests look for.
#pragma once
#include <cstdint>
#include <cstdio>

static int g_checks = 0, g_fail = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond)) { ++g_fail; std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static void* fake(uintptr_t k) { return reinterpret_cast<void*>(0x100000 + 0x1000 * k); }   // never dereferenced

// the driver's last line and exit status
static int report(const char* driver) {
    std::printf("%s: %d checks, %d failed\n", driver, g_checks, g_fail);
    return g_fail ? 1 : 0;
}
