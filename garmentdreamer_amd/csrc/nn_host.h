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

}  // namespace
