// dpenv_host.h - private to the two host units of libdpenv.so: dpenv_api.hip (every entry point that takes a handle; the handle's
// struct is defined there and nowhere else) and dpenv_api_free.hip (the entry points that take none).  Error reporting, the device guard and
// the pure validators both units use; hidden like the launchers of dpenv_dev.h.
#ifndef DPENV_HOST_H
#define DPENV_HOST_H

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/dpenv.h"
#include "dpenv_dev.h"

namespace dpenv {
namespace __attribute__((visibility("hidden"))) host {

// The message goes into the handle or, with h == NULL, into the one thread-local string dpenv_last_error(NULL) returns, whichever
// unit failed (defined in dpenv_api.hip, which can look inside a handle).  Returns code.
int fail(dpenv_handle h, int code, const char* fmt, ...);

#define HIP_TRY(h, expr)                                                                               \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(h, DPENV_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// Entry points launch on the handle's device even if the caller's current device is another one.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int want)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != want) switched = (hipSetDevice(want) == hipSuccess);
    }
    ~DeviceGuard()
    {
        if (switched) (void)hipSetDevice(prev);
    }
};

// ---- validators without a handle (dpenv_api_free.hip) ----
int mode_of(const dpenv_config* c);                          // MODE_* of the variant, -1 if unknown
// allow_loss: the caller deals with the inflow thrust-loss coefficients (parameters 26-31), which are not part of a VesselDev
int derive_vessel(const float* p, VesselDev* d, std::string* why, bool allow_loss = false);
// the f32 coefficients, or an error message
const char* reff_coeffs_f32(const dpenv_reference_filter* rf, float dt, float phi[3][9], float gam[3][3]);
// the law's numbers into ControlArgs, or an error message
const char* control_check(const dpenv_dp_controller* c, ControlArgs& g);
// the QP allocation's numbers for the control period dt into QpArgs, or an error message
const char* qp_check(const dpenv_qp_allocator* q, float dt, QpArgs& g);
// the neural allocation's shape and constants into NnArgs (W and b are the caller's pointers, required non-NULL, not dereferenced), or an
// error message; device_pointers is not looked at
const char* nn_check(const dpenv_nn_allocator* a, NnArgs& g);
// nn_check, then device_pointers == 1: what the calls that read the weights in place demand
const char* nn_check_in_place(const dpenv_nn_allocator* a, NnArgs& g);
// what the population calls refuse of K and envs_per_net, or NULL
const char* nn_pop_check(int32_t K, int32_t envs_per_net);

}  // namespace host
}  // namespace dpenv

#endif
