// batch_host.h -- the buffers a handle owns: the kinds a fleet handle shares with the device (Pinned, PinnedDefault, Staging) and the
// two that copies run between (Device, Host).  Each knows how its memory was taken: what alloc() took, release() gives back the same
// way, and release() of an empty buffer does nothing.  Plain aggregates: a handle holds them by value and releases them when it is
// destroyed; nothing copies them (two of a handle's buffers may change places: std::swap).  LinkEvents, the two events of a
// producer's rlink, is released the same way.
#pragma once
#include "host_visible.h"

#include <hip/hip_runtime.h>

namespace batch_host {
namespace {   // (a handle's translation unit exports its C functions and nothing else)

// n elements of pinned host memory, mapped and coherent: the host reads and writes `h`, the device `dv`, both in place
template <typename T, unsigned FLAGS = hipHostMallocMapped | hipHostMallocCoherent>
struct Pinned {
    T *h = nullptr, *dv = nullptr;
    // all or nothing: a buffer whose device pointer cannot be had is given back
    hipError_t alloc(size_t n)
    {
        hipError_t e = hipHostMalloc((void **)&h, sizeof(T) * n, FLAGS);
        if (e != hipSuccess) { h = nullptr; return e; }
        e = hipHostGetDevicePointer((void **)&dv, h, 0);
        if (e != hipSuccess) release();
        return e;
    }
    void release()
    {
        if (h) (void)hipHostFree(h);
        h = dv = nullptr;
    }
};

// the same, taken with the default flags and then asked for its device pointer (the fleet filter's ring, pose slots and reflector rows)
template <typename T>
using PinnedDefault = Pinned<T, hipHostMallocDefault>;

// a staging area the host writes and a kernel reads in place: host-visible device memory where the platform gives it
// (host_visible.h; `in_vram` says so), else pinned host memory
template <typename T>
struct Staging : Pinned<T> {
    bool in_vram = false;
    hipError_t alloc(size_t n)
    {
        this->h = this->dv = static_cast<T *>(host_visible::alloc(sizeof(T) * n));
        in_vram = this->h != nullptr;
        return in_vram ? hipSuccess : alloc_pinned(n);
    }
    hipError_t alloc_pinned(size_t n) { return Pinned<T>::alloc(n); }
    void release()
    {
        if (in_vram) { (void)hipFree(this->h); this->h = this->dv = nullptr; in_vram = false; }
        else Pinned<T>::release();
    }
};

// n elements of device memory
template <typename T>
struct Device {
    T *d = nullptr;
    hipError_t alloc(size_t n) { const hipError_t e = hipMalloc((void **)&d, sizeof(T) * n); if (e != hipSuccess) d = nullptr; return e; }
    void release() { if (d) (void)hipFree(d); d = nullptr; }
};

// n elements of pinned host memory taken with the default flags (neither mapped nor coherent): one end of a copy, never a kernel's argument
template <typename T>
struct Host {
    T *h = nullptr;
    hipError_t alloc(size_t n) { const hipError_t e = hipHostMalloc((void **)&h, sizeof(T) * n, hipHostMallocDefault); if (e != hipSuccess) h = nullptr; return e; }
    void release() { if (h) (void)hipHostFree(h); h = nullptr; }
};

// Grow or replace, the one rule: the new allocation first, then `fill(fresh)` -- everything else that can fail -- and only then is the
// old buffer released and the fresh one put in its place.  On an error the fresh one is released and the old one stays as it was.
template <typename Buf, typename Fill>
hipError_t replace(Buf &old, size_t n, Fill &&fill)
{
    Buf fresh;
    hipError_t e = fresh.alloc(n);
    if (e == hipSuccess) e = fill(fresh);
    if (e != hipSuccess) { fresh.release(); return e; }
    old.release();
    old = fresh;
    return e;
}

// a buffer of `cap` elements holds `need`: grown by doubling, from `first` for an empty one, under replace()'s rule
template <typename Buf>
hipError_t reserve(Buf &b, size_t &cap, size_t need, size_t first)
{
    if (cap >= need) return hipSuccess;
    size_t c = cap ? cap : first;
    while (c < need) c *= 2;
    const hipError_t e = replace(b, c, [](Buf &) { return hipSuccess; });
    if (e == hipSuccess) cap = c;
    return e;
}

// The two events of a producer's rlink (include/rlink.h) and whether a link of its outstanding submit was taken.  `ready` is recorded
// behind the producer's launch, `consumed` by the consumer once everything that reads the records is enqueued; both are made by
// the first link.
struct LinkEvents {
    hipEvent_t ready = nullptr, consumed = nullptr;
    bool taken = false;
    // before a submit: a link of the submit before was taken (*linked) -> the consumer's reads of the records come first, on the stream
    hipError_t wait(hipStream_t stream, bool *linked)
    {
        *linked = taken;
        const hipError_t e = taken ? hipStreamWaitEvent(stream, consumed, 0) : hipSuccess;
        if (e == hipSuccess) taken = false;
        return e;
    }
    // a link is taken: `ready` behind everything the stream holds
    hipError_t record(hipStream_t stream)
    {
        hipError_t e = ready ? hipSuccess : hipEventCreateWithFlags(&ready, hipEventDisableTiming);
        if (e == hipSuccess && !consumed) e = hipEventCreateWithFlags(&consumed, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(ready, stream);
        if (e == hipSuccess) taken = true;
        return e;
    }
    void release()
    {
        if (consumed) { (void)hipEventSynchronize(consumed); (void)hipEventDestroy(consumed); }   // (a consumer may still read the records)
        if (ready) (void)hipEventDestroy(ready);
        ready = consumed = nullptr;
    }
};

// release() of every buffer named: what a handle's destroy calls
template <typename... B>
void release_all(B &...b) { (b.release(), ...); }

}  // namespace
}  // namespace batch_host
