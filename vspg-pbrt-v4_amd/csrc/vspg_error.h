// vspg_error.h -- the library's error channel: every entry point reports a failure as `return fail(code, message)`, and
// vspg_last_error() returns the calling thread's last message.  The message is defined once, in vspg_scene_api.hip.
#pragma once
#include <string>

#pragma GCC visibility push(hidden)  // shared between the library's units, not part of its ABI
namespace vspg_host {
int fail(int code, const std::string &msg);
}  // namespace vspg_host
#pragma GCC visibility pop

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(VSPG_EHIP, std::string(#expr) + ": " + hipGetErrorName(e_) + " (" + hipGetErrorString(e_) + ")"); \
    } while (0)
