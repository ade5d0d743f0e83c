// nn_host.h -- host error plumbing of the nn_*.hip translation units.  Everything sits in an unnamed namespace: each
// file that includes this gets its OWN buffer, the channel behind its gd_nn_*_last_error() (include/gd_nn.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/gd_nn.h"

namespace {

thread_local char g_err[256] = "";
int fail(int code, const char* msg)
{
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

// Tail of an entry point, after its launches: GD_NN_OK, or GD_NN_ERR_HIP with `msg` (default: HIP's own error string).
int launch_status(const char* msg = nullptr)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GD_NN_OK : fail(GD_NN_ERR_HIP, msg ? msg : hipGetErrorString(e));
}

// The current device, 0 .. kMaxDevices - 1 (the bound of the per-device tables of the library); on failure the error code
// (< 0) with the message set.
constexpr int kMaxDevices = 16;
int current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return fail(GD_NN_ERR_HIP, "hipGetDevice failed");
    return dev;
}

// Reserves `lds` bytes of dynamic LDS for kernel `Kern`, once per device: every launcher of the library keys it so.  The
// key is the kernel INSTANTIATION, a non-type template argument -- all instantiations of one kernel template share their
// function-pointer TYPE, so a helper templated on the type would take conv3x3_wino_kernel<false> for done after <true> ran.
template <auto Kern>
int reserve_lds(int dev, int lds, const char* msg = "cannot reserve the kernel's dynamic LDS")
{
    static bool done[kMaxDevices] = {false};
    if (done[dev]) return GD_NN_OK;
    if (hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return fail(GD_NN_ERR_HIP, msg);
    done[dev] = true;
    return GD_NN_OK;
}

}  // namespace
