// The calling thread's error string (ccmm_last_error): one thread-local string, defined in ccmm_abi.hip.
// No HIP here: the host-only modules (ccmm_batch.cpp, ccmm_diag.cpp) include this header alone.
#pragma once
#include <string>

namespace ccmm {
void set_last_error(const std::string& msg);  // message of the next ccmm_last_error() on this thread
const std::string& last_error();
}  // namespace ccmm
