// det_batch_dev.h -- the HIP calls the two fleet detector handles (det2d_batch.hip, det3d_batch.hip) share: what both keep, their
// create / destroy frame, the link protocol (include/rlink.h; batch_host.h's LinkEvents) and collect around det_batch_host.h's rules.
#pragma once
#include "batch_host.h"
#include "det_batch_host.h"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <new>
#include <string>

#define DETB_TRY(h, expr)                                                           \
    do {                                                                            \
        hipError_t e_ = (expr);                                                     \
        if (e_ != hipSuccess) {                                                     \
            if (h) (h)->hip_error = std::string(#expr) + ": " + hipGetErrorString(e_); \
            return RDET_ERR_HIP;                                                    \
        }                                                                           \
    } while (0)

namespace det_batch_dev {
namespace {

// what both handles keep; a handle adds its members `m` and its buffers
struct Handle : det_batch_host::SubmitState {
    int B = 0, device = 0;
    hipStream_t stream = nullptr;
    batch_host::LinkEvents link;
    std::string hip_error;
};

// a handle of B members with their options and sensor_to_base_link, nothing allocated on the device yet (NULL: no memory)
template <typename H, typename Opt>
inline H *make(const Opt *opts, const double *s2b_xyyaw, int B, int device)
{
    H *b = new (std::nothrow) H();
    if (!b) return nullptr;
    b->B = B; b->device = device;
    b->m.resize((size_t)B);
    for (int i = 0; i < B; ++i) {
        b->m[(size_t)i].opt = opts[i];
        std::memcpy(b->m[(size_t)i].s2b, s2b_xyyaw + 3 * i, sizeof(double) * 3);
    }
    b->size(B);
    return b;
}

// waits for the stream and for a consumer that may still read the records, then releases the events, the buffers and the stream
template <typename... Bufs>
inline void destroy(Handle *b, Bufs &...bufs)
{
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    batch_host::release_all(b->link, bufs...);
    if (b->stream) (void)hipStreamDestroy(b->stream);
}

template <typename H>
inline int set_sensor_to_base_link(H *b, int member, const double xyyaw[3])
{
    if (!b || !xyyaw || member < 0 || member >= b->B) return RDET_ERR_INVALID;
    std::memcpy(b->m[(size_t)member].s2b, xyyaw, sizeof(double) * 3);
    return RDET_OK;
}

// the HIP calls in front of a validated submit.  A link of the submit before was taken (*linked): the consumer's reads of the
// records come first, on the stream.  Until then the host leaves the records alone too (what it would clear is never read: collect
// looks at sub_runs first)
inline int begin_submit(Handle *b, bool *linked)
{
    DETB_TRY(b, hipSetDevice(b->device));
    DETB_TRY(b, b->link.wait(b->stream, linked));
    return RDET_OK;
}

// rdet*_batch_link: `records` is the device's address of the handle's out records
template <typename Out>
inline int link(Handle *b, const Out *records, rlink *out)
{
    if (!out || !b->outstanding) return RDET_ERR_INVALID;
    DETB_TRY(b, hipSetDevice(b->device));
    DETB_TRY(b, b->link.record(b->stream));
    det_batch_host::fill_link(*b, b->device, records, (long)sizeof(Out), (int)offsetof(Out, K), (int)offsetof(Out, err),
                              (int)offsetof(Out, centers), b->link.ready, b->link.consumed, out);
    return RDET_OK;
}

// rdet*_batch_collect: `records` is the host's address of the same
template <typename Out, typename Each>
inline int collect(Handle *b, const Out *records, int *status, int *K, float *centers_xy, int max_centers, double *obs_time, Each &&each)
{
    if (!b->outstanding || !det_batch_host::collect_args_ok(b->sub_count, status, K, centers_xy, max_centers)) return RDET_ERR_INVALID;
    b->outstanding = false;
    DETB_TRY(b, hipSetDevice(b->device));
    DETB_TRY(b, hipStreamSynchronize(b->stream));
    det_batch_host::collect(*b, records, status, K, centers_xy, max_centers, obs_time, each);
    return RDET_OK;
}

}  // namespace
}  // namespace det_batch_dev
