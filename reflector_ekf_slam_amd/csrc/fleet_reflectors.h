// fleet_reflectors.h -- one launch of k_fleet_reflectors (fleet_reflectors.hip) as rfleet_get_reflectors (rfleet_api.hip) describes it.
#pragma once
#include "fleet_dev.h"

#define RFLEET_REFLECTOR_THREADS 128     // one lane per reflector: RFLEET_MAX_LANDMARKS

struct FleetReflectorsLaunch {
    const int *members;      // [count] the listed members, in the caller's order (pinned host memory); NULL: member g is g
    int count, pad_;
    long cap_rows;           // a row at or beyond it is not written (never more than the buffers hold)
    int *counts;             // [count] reflectors of each listed member (pinned)
    double *ell5;            // [rows][5] mx, my, angle, x_len, y_len (pinned); NULL: not asked for
    double *xy2;             // [rows][2] the reflector's mean
    double *cov4;            // [rows][4] its covariance block, row-major (a, b, c, d) with b = c
};

hipError_t rfleet_launch_reflectors(const FleetDev &d, const FleetReflectorsLaunch &l, hipStream_t s);
