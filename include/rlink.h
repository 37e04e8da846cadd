/*
 * rlink.h -- one outstanding submit of a fleet detector, as a consumer on the same device needs to see it.
 *
 * librdet.so (rdet2d_batch_link / rdet3d_batch_link of rdet.h) fills an rlink, librfleet.so (rfleet_submit_linked of rfleet.h)
 * reads one: neither library includes the other's header, and this one names no type of either.  Plain C, no HIP type: the two
 * events are hipEvent_t carried as void *.
 *
 * Entry i is scan / cloud i of the detector's submit.  What the detector's HOST knows of it lies in four host arrays, valid until
 * the detector's next submit: whose it is, its stamp, the status the host alone would report, and which output record the launch
 * fills for it.  What only the launch knows -- K, the kernel's own error, the centres -- lies in that record, in memory the device
 * can address: record r starts at records + r * record_bytes and holds an int K at k_off, an int err at err_off and max_centers
 * (x, y) float pairs at centers_off.
 *
 * The two events order the streams without the host: the producer records `ready` on its stream behind its launch, the consumer
 * makes its stream wait for it before it reads a record, and records `consumed` on its own stream once everything that reads the
 * records is enqueued; the producer's next submit makes its stream wait for `consumed` before its kernel overwrites them.  Either
 * may be NULL: nothing to wait for / nobody to tell (a link whose records somebody planted by hand).
 */
#ifndef RLINK_H_
#define RLINK_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rlink {
    int count;                 /* entries */
    int device;                /* the HIP device of the records and the events */
    const int *member;         /* [count] */
    const double *stamp;       /* [count]: observation.time_ of entry i */
    const int *host_status;    /* [count]: 0, or what collect will report from the host alone (a malformed scan) */
    const int *record;         /* [count]: the entry's output record, or -1: no workgroup runs for it, K = 0 is known */
    const void *records;       /* device-visible base address of the records */
    long record_bytes;         /* stride */
    int k_off, err_off, centers_off;   /* byte offsets inside a record; centers_off is a multiple of 8 */
    int max_centers;           /* pairs a record holds */
    void *ready;               /* hipEvent_t or NULL */
    void *consumed;            /* hipEvent_t or NULL */
} rlink;

#ifdef __cplusplus
}
#endif
#endif /* RLINK_H_ */
