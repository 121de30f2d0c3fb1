// orbx_handle.h -- host plumbing shared by the handles of the C ABI: device + stream, the timing events behind *_last_timing, device
// arrays that free themselves, and the launch checks.  Host only.  A handle struct derives from OrbxHandle, declares its device arrays as
// OrbxOwnedBuf (its staging as OrbxHostStage / OrbxCallBox) and at most one OrbxCallTimer, and its *_destroy is orbx_destroy_handle():
// there is no release list to keep in step with the members.
#ifndef ORBX_HANDLE_H
#define ORBX_HANDLE_H

#include "orbx_internal.h"

/* OrbxDevBuf that frees its memory with its owner.  (The two fold into one type once orbx_image.hip may be touched again.) */
template <typename T> struct OrbxOwnedBuf : OrbxDevBuf<T> {
    OrbxOwnedBuf() = default;
    OrbxOwnedBuf(const OrbxOwnedBuf &) = delete;
    OrbxOwnedBuf &operator=(const OrbxOwnedBuf &) = delete;
    ~OrbxOwnedBuf() { this->release(); }
};

struct OrbxHandle {
    int device = 0;
    hipStream_t stream = nullptr;
    OrbxHandle() = default;
    OrbxHandle(const OrbxHandle &) = delete;
    OrbxHandle &operator=(const OrbxHandle &) = delete;
    /* head of a *_create: ORBX_ERR_NODEVICE / ORBX_ERR_ARG from orbx_select_device, else the handle's non-blocking stream */
    int open(int dev)
    {
        if (const int rc = orbx_select_device(dev)) return rc;
        device = dev;
        ORBX_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return ORBX_OK;
    }
    void quiesce()
    {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
    }
    ~OrbxHandle() { if (stream) (void)hipStreamDestroy(stream); }
};

/* *_destroy: drain the stream, then delete.  The derived struct's members go before this base, i.e. they free their memory after the stream
 * has drained and before it is destroyed; their destructors accept the half-built state a failed *_create leaves (null pointers). */
template <class H> void orbx_destroy_handle(H *h)
{
    if (!h) return;
    h->quiesce();
    delete h;
}

static inline int orbx_event_create(hipEvent_t *e, unsigned flags = hipEventDefault)
{
    ORBX_HIP_CHECK(hipEventCreateWithFlags(e, flags));
    return ORBX_OK;
}

/* The two events around a call's launches and the launch count, read by *_last_timing.  A member, not a base: handles without timing take none. */
struct OrbxCallTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool timed = false;
    int launches = 0;
    OrbxCallTimer() = default;
    OrbxCallTimer(const OrbxCallTimer &) = delete;
    OrbxCallTimer &operator=(const OrbxCallTimer &) = delete;
    ~OrbxCallTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    int create()      // (again after a failure, or on first use: makes what is missing)
    {
        for (hipEvent_t &e : ev)
            if (!e) { const int rc = orbx_event_create(&e); if (rc != ORBX_OK) return rc; }
        return ORBX_OK;
    }
    int begin(hipStream_t st)
    {
        launches = 0;
        ORBX_HIP_CHECK(hipEventRecord(ev[0], st));
        return ORBX_OK;
    }
    int end(hipStream_t st)
    {
        ORBX_HIP_CHECK(hipEventRecord(ev[1], st));
        timed = true;
        return ORBX_OK;
    }
    /* *_last_timing.  A handle that never ran: ORBX_ERR_STATE with the text `neverRan`, or - neverRan == nullptr - zeros and ORBX_OK. */
    int read(int device, float *ms, int *nLaunches, const char *neverRan)
    {
        float t = 0.f;
        if (!timed) {
            if (neverRan) { orbx_set_error("%s", neverRan); return ORBX_ERR_STATE; }
        } else {
            ORBX_HIP_CHECK(hipSetDevice(device));
            ORBX_HIP_CHECK(hipEventSynchronize(ev[1]));
            ORBX_HIP_CHECK(hipEventElapsedTime(&t, ev[0], ev[1]));
        }
        if (ms) *ms = t;
        if (nLaunches) *nLaunches = timed ? launches : 0;
        return ORBX_OK;
    }
};

/* after a kernel launch, in a function that returns an ORBX_* code */
#define ORBX_LAUNCH_CHECK()                                                                                                                   \
    do {                                                                                                                                      \
        const hipError_t le_ = hipGetLastError();                                                                                             \
        if (le_ != hipSuccess) { orbx_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(le_), __FILE__, __LINE__); return ORBX_ERR_HIP; } \
    } while (0)
/* ... and one more launch on the call's timer */
#define ORBX_LAUNCH_COUNT(timer) \
    do {                         \
        ORBX_LAUNCH_CHECK();     \
        (timer).launches++;      \
    } while (0)

#endif
