// osp_internal.h -- shared between the HIP side (osp_api.hip) and the host side (osp_host.cpp).
#pragma once
#include <exception>
#include <new>
#include <string>

#include "../../include/outerspace_spgemm.h"
#include "osp_settings.h"

namespace osp {

struct Error : std::exception {
    int status;
    std::string msg;
    Error(int st, std::string m) : status(st), msg(std::move(m)) {}
    const char *what() const noexcept override { return msg.c_str(); }
};

extern thread_local std::string g_last_error;
// Records the message for osp_last_error_string() and returns `status`.
int fail(int status, const char *fmt, ...);

// The exception boundary of a C entry point: runs `body` (which returns a status) and turns what it throws into a status.
template <class F>
int guard(F &&body) {
    try {
        return body();
    } catch (const Error &e) {
        return fail(e.status, "%s", e.what());
    } catch (const std::bad_alloc &) {
        return fail(OSP_ERR_ALLOC, "host allocation failed");
    } catch (const std::exception &e) {
        return fail(OSP_ERR_ALLOC, "%s", e.what());
    }
}

}  // namespace osp
