// Argument checks, precision dispatch and the device guard shared by every source that defines extern "C" entry points.
#pragma once
#include "fb_plan.h"

// (every entry point starts with an argument check: it also reads away a stale "last error" some other user of the
// HIP runtime may have left in this thread, so that the launch checks below report this call's errors only)
#define FB_REQUIRE(cond, msg) do { (void)hipGetLastError(); if (!(cond)) { fb_set_error(msg); return FB_ERR_INVALID; } } while (0)
#define FB_DISPATCH(p, call32, call64) ((p)->prec == 4 ? (call32) : (call64))
// A few words of a result to the host, complete on return: the copy and the wait for stream s -- so everything queued on s
// before it has finished as well, which callers rely on (see the comments where they call it).
static inline int fb_read_back(void* host_dst, const void* dev_src, size_t bytes, hipStream_t s) {
    FB_HIP(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, s));
    FB_HIP(hipStreamSynchronize(s));
    return FB_OK;
}
// A plan belongs to one device.  Every entry point that takes a plan makes that device current for the duration of the
// call (allocations, NULL-stream launches and the plan's own auxiliary stream / events all follow the current device)
// and puts the caller's device back when it returns -- other users of the HIP runtime in this thread (torch, RCCL)
// keep the current device they had -- so plans on different GPUs can be used from one thread in any order.
namespace {
struct FbDeviceGuard {
    int prev = -1;
    bool changed = false;
    int enter(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); }
        if (prev != dev) {
            const int r = fb_hip_check(hipSetDevice(dev), "hipSetDevice");
            if (r) return r;
            changed = prev >= 0;
        }
        return FB_OK;
    }
    ~FbDeviceGuard() { if (changed) (void)hipSetDevice(prev); }
};
}  // namespace
#define FB_USE_DEVICE(p) FbDeviceGuard _fb_devguard; do { const int _r = _fb_devguard.enter((p)->device); if (_r) return _r; } while (0)
