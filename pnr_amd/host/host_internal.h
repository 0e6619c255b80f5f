// host_internal.h -- what the host's source files share with one another and advantra_host.h does not publish.
#pragma once
#include "advantra_host.h"
#include "stack_io.h"
#include <cstdio>

namespace advantra {

// "<what>: <the library's last error>" on stderr (what = nullptr: the error alone, as the tracing run reports it); false
inline bool lib_fail(const char *what)
{
    fprintf(stderr, what ? "%s: %s\n" : "%s%s\n", what ? what : "", pnr_last_error());
    return false;
}

// save_stack_u8 with its message on stderr
inline bool write_stack(const std::string &name, const unsigned char *vol, long long w, long long h, long long l)
{
    std::string e;
    if (save_stack_u8(name, vol, w, h, l, e)) return true;
    fprintf(stderr, "%s\n", e.c_str());
    return false;
}

// a device context that ends with its scope
struct Ctx {
    pnr_ctx *raw = nullptr;
    Ctx() = default;
    Ctx(const Ctx &) = delete;
    Ctx &operator=(const Ctx &) = delete;
    ~Ctx() { if (raw) pnr_destroy(raw); }
    operator pnr_ctx *() const { return raw; }
    // false after lib_fail(what)
    bool create(const pnr_params &p, int device, const char *what = "pnr_create") { return pnr_create(&p, device, &raw) == PNR_OK || lib_fail(what); }
};

// stack_reader.cpp: load_stack with the channel and raw type of settings(), then the refusal of --window / --saturate on an 8-bit
// stack; either failure is reported on stderr
enum class Loaded { ok, unreadable, not_windowable };
Loaded load_input_stack(const std::string &path, const std::string &raw_dims, Stack &out);

// swc_io.cpp: load_swc with its message on stderr; the shortest decimal text without an exponent (nine digits at the most) that reads
// back as the same f32
bool read_swc(const std::string &path, SwcTree &out);
std::string f32_text(float v);

} // namespace advantra
