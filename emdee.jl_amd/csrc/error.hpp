// error.hpp -- error plumbing: no exception crosses the C ABI.  No HIP include: host-only code (topology.hpp) and its
// stand-alone test program see the same set_error / Failure / EMDEE_REQUIRE as the library.
#pragma once

#include <cstdint>

#include "../../include/emdee_hip.h"

namespace emdee {

void set_error(const char *fmt, ...);
const char *get_error();

struct Failure {
    int32_t code;
};

}  // namespace emdee

#define EMDEE_REQUIRE(cond, code, ...)                                                           \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            ::emdee::set_error(__VA_ARGS__);                                                     \
            throw ::emdee::Failure{code};                                                        \
        }                                                                                        \
    } while (0)
