// What every side object (channeliser, scanner, IQ corrector, resampler, mixer, meter, monitors, squelch) does the same way.  Host only.
//
// The call-order rule: a handle's state carries over from call to call, so a process call on any stream is ordered behind
// the previous call's work, and getters, setters and destroy wait for that work on the host.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

namespace fmd {

// The handle's device, the event at the end of the previous call's work and whether a call has been recorded.
// process is  begin(s) -> launches on s -> end(s);  begin and end return nullptr or the failed step's error text.
class CallOrder {
public:
    CallOrder() = default;
    CallOrder(const CallOrder&) = delete;
    CallOrder& operator=(const CallOrder&) = delete;
    ~CallOrder() { if (done_) (void)hipEventDestroy(done_); }

    bool init(int device) {
        device_ = device;
        return hipSetDevice(device) == hipSuccess && hipEventCreateWithFlags(&done_, hipEventDisableTiming) == hipSuccess;
    }
    int device() const { return device_; }

    // a caller that switches streams is ordered behind the previous call
    const char* begin(hipStream_t s) {
        if (hipSetDevice(device_) != hipSuccess) return "hipSetDevice failed";
        if (recorded_ && hipStreamWaitEvent(s, done_, 0) != hipSuccess) return "stream wait failed";
        return nullptr;
    }
    const char* end(hipStream_t s) {
        if (hipEventRecord(done_, s) != hipSuccess) return "event record failed";
        recorded_ = true;
        return nullptr;
    }
    // the previous call's work is complete on return; on false the caller reports "synchronise failed"
    bool quiesce() { return hipSetDevice(device_) == hipSuccess && (!recorded_ || hipEventSynchronize(done_) == hipSuccess); }
    // after a device-wide synchronise there is nothing left to wait for
    void forget() { recorded_ = false; }

private:
    int device_ = 0;
    hipEvent_t done_ = nullptr;
    bool recorded_ = false;
};

// A control call's `channel` as the stations c0 ... c0 + cn - 1 of C (-1: every station); false when it is outside [-1, C).
inline bool channel_range(int channel, int C, int* c0, int* cn) {
    if (channel < -1 || channel >= C) return false;
    *c0 = channel < 0 ? 0 : channel;
    *cn = channel < 0 ? C : 1;
    return true;
}

// Closes a control launch on the null stream, which is done before a later call on any stream: nullptr, or the failed step's error
// text (`launch_failed` for the launch itself).
inline const char* control_end(const char* launch_failed) {
    if (hipGetLastError() != hipSuccess) return launch_failed;
    if (hipStreamSynchronize(nullptr) != hipSuccess) return "synchronise failed";
    return nullptr;
}

// the formatted message into `dst` (a handle's err or the object's global string); returns `code`
inline int fail(std::string& dst, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    dst = buf;
    return code;
}

}  // namespace fmd
