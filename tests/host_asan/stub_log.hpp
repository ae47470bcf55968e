// The launch log's line (hip_stub.cpp, amuse_stub_log(2)), shared with the stubs of launchers that live beside it (audio_x_stub.cpp): the tables behind the
// pointer, stream and image texts stay in hip_stub.cpp and are reached through the four functions below.  Test infrastructure only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

int amuse_stub_log_level();                                  // 0 off | 1 image log | 2 launch log
std::string amuse_stub_ptr_text(const void* p);              // `0`, `dev#<n>+<offset>/<block size>`, `<name>+<offset>` or `host`
std::string amuse_stub_stream_text(hipStream_t s);           // `0` or `#<order of creation>`
unsigned long long amuse_stub_image_of(const void* p);       // digest of the last upload to exactly this pointer, 0 if none
void amuse_stub_emit(const std::string& line);               // prints the line (and hands it to amuse_stub_capture's vector, if one is set)

// one line of the launch log: `name key=value ...`, printed when it goes out of scope
struct Line {
    std::string s;
    explicit Line(const char* name) : s(name) {}
    ~Line() { amuse_stub_emit(s); }
    Line& kv(const char* k, const std::string& v) { s += ' '; s += k; s += '='; s += v; return *this; }
    Line& p(const char* k, const void* v) { return kv(k, amuse_stub_ptr_text(v)); }
    Line& i(const char* k, long long v) { return kv(k, std::to_string(v)); }
    Line& u(const char* k, unsigned long long v) { return kv(k, std::to_string(v)); }
    Line& f(const char* k, float v) { char b[40]; snprintf(b, sizeof(b), "%a", (double)v); return kv(k, b); }   // (hex float: exact)
    Line& x(const char* k, unsigned long long v) { char b[24]; snprintf(b, sizeof(b), "%016llx", v); return kv(k, b); }
    Line& st(hipStream_t v) { return kv("stream", amuse_stub_stream_text(v)); }
    Line& wp(const char* k, const void* v) { return p(k, v).x("image", amuse_stub_image_of(v)); }   // a weight pointer: where it is and what was uploaded there
    Line& w(const void* v) { return wp("wstream", v); }
};
#define P_(f) p(#f, a.f)
#define I_(f) i(#f, (long long)a.f)
#define U_(f) u(#f, (unsigned long long)a.f)
