// gg_error.h — the library's one error channel: a status code returned, its text kept per thread for
// mxmoe_gg_last_error. Used by the ABI layer (gg_api.hip), the host planner (gg_plan.cpp) and the MoE plumbing
// (moe_ops.hip); defined once, in the unit that sets MXMOE_ERROR_DEFINE before including it (gg_plan.cpp).
#pragma once

#include <cstdarg>
#include <cstdio>
#include <string>

namespace mxmoe {
namespace detail {
int set_error(int code, const std::string& msg);  // keeps msg as the calling thread's last error; returns code
}  // namespace detail

#pragma GCC visibility push(hidden)  // (internal: not among the library's exported symbols)
const char* last_error();                         // the calling thread's last error text (valid until its next error)
int fail(int code, const char* fmt, ...);         // set_error of a printf-style text
#pragma GCC visibility pop

#ifdef MXMOE_ERROR_DEFINE
namespace {
thread_local std::string g_last_error;
}
namespace detail {
int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
}  // namespace detail
const char* last_error() { return g_last_error.c_str(); }
int fail(int code, const char* fmt, ...) {
  char buf[768];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}
#endif

}  // namespace mxmoe
