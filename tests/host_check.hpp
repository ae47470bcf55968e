// What the stand-alone host programs (tests/*_host/main.cpp) share: the library's error slot as a stand-in that keeps the text, and CHECK, which prints the failed
// condition with that text and returns 1 from the function it stands in.
#pragma once
#include <cstdarg>
#include <cstdio>

static char g_err[512];
int amuse_failf(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { printf("FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, g_err); return 1; } \
    } while (0)
