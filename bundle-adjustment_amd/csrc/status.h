// How a function of the library leaves early.  `err` is the std::string that jaicov_neq_last_error hands out.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/jaicov_neq.h"

#define FAIL(err, code, msg) \
    do {                     \
        (err) = (msg);       \
        return (code);       \
    } while (0)
#define HIPE(err, x)                                                                           \
    do {                                                                                       \
        hipError_t _err = (x);                                                                 \
        if (_err != hipSuccess) {                                                              \
            (err) = std::string(#x) + ": " + hipGetErrorString(_err);                          \
            return _err == hipErrorOutOfMemory ? JAICOV_ERR_OUT_OF_MEMORY : JAICOV_ERR_DEVICE; \
        }                                                                                      \
    } while (0)
#define TRY(x) do { const int _rc = (x); if (_rc) return _rc; } while (0)      // a callee's status (JAICOV_*), passed on
#define HIPCHK(x)                                  \
    do {                                           \
        hipError_t _e = (x);                       \
        if (_e != hipSuccess) return _e;           \
    } while (0)

// what every entry point that may be the process's first asks before it touches the device
inline int check_device(std::string &err) {
    int count = 0;
    hipError_t r = hipGetDeviceCount(&count);
    if (r != hipSuccess || count <= 0) {
        err = "no HIP device available (this engine has no CPU fallback)";
        return JAICOV_ERR_NO_DEVICE;
    }
    return JAICOV_OK;
}
