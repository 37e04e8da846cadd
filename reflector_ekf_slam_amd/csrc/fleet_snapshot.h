// fleet_snapshot.h -- one launch of k_fleet_pack / k_fleet_unpack (fleet_snapshot.hip) as rfleet_snapshot / rfleet_restore
// (rfleet_api.hip) describe them.
#pragma once
#include "fleet_dev.h"

#define RFLEET_SNAP_THREADS 256          // four waves: each takes every fourth column of its panel
#define RFLEET_SNAP_PANEL 16             // columns per workgroup

// One workgroup's work, built by the host: a panel of RFLEET_SNAP_PANEL columns of one listed member.
struct FleetSnapRec {
    int member;              // pack: the member read; unpack: the member written
    int panel;               // columns [16 panel, 16 panel + 16)
    int n;                   // the state dimension of the member's payload (pack: as the pose slot says; unpack: as the blob says)
    int flags;               // unpack: the sticky flags the member gets
    long off;                // index in doubles of the member's payload in `buf`: mu[0:n], then the packed lower triangle
};
static_assert(sizeof(FleetSnapRec) == 24, "the host packs the table as 24-byte records");

struct FleetSnapLaunch {
    const FleetSnapRec *rec; // [count] (device memory)
    double *buf;             // the staging buffer's payload part (device memory)
    long cap;                // doubles `buf` holds: a record whose payload does not end inside it moves nothing
    int count, pad_;
};

// doubles of one member's payload
static inline long fleet_snap_doubles(long n) { return n + n * (n + 1) / 2; }

hipError_t rfleet_launch_pack(const FleetDev &d, const FleetSnapLaunch &l, hipStream_t s);
hipError_t rfleet_launch_unpack(const FleetDev &d, const FleetSnapLaunch &l, hipStream_t s);
