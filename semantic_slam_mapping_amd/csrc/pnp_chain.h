// pnp_chain.h -- interface between the tracker's device leg (ssm_track.hip: the hooks the host state machine in ssm_track_host.cpp calls) and the device pose chain
// (kernels_pnp.hip).  The chain's state block, which the host source shares, is pnp_state.h.  Not installed.
#pragma once
#include "ssm_internal.h"
#include "pnp_state.h"
#include "../../include/ssm/pnp_core.h"
struct PnpChainArgs {
    const ssm_keypoint* kps; const float* pos3d; const ssm_dmatch* matches; const int32_t* nmatch;     // the call's outputs (device)
    const float* hist_pos3d;                         // R x cap x 3: positions of the deque members that precede the call, row idx + R
    int cap, R, f_begin, f_end, max_lost;
    ssm_pnp::Camera cam;
    PnpState* state; double* pose_out; ssm_track_info* info_out;
    float *img, *obj; uint8_t *inl, *dec;                                                              // scratch for R * cap correspondences
    struct LEdge* ledges; double2* err;              // the edge list when it does not fit in LDS (k_pnp_edge_bytes() each), and every edge's error
    int edges_in_lds;                                // set by k_pnp_chain
    // the cluster form: `blocks` (1, 2, 4 or 8) blocks run the chain together; state, img / obj / inl / dec / ledges / err hold `blocks` slices (slice b is block b's
    // private copy; the host fills every state slice and reads slice 0); xchg: k_pnp_xchg_bytes() of device memory, xfail = the word behind its ring
    int blocks; unsigned long long* xchg; unsigned* xfail;
};
size_t k_pnp_xchg_bytes(void);
hipError_t k_pnp_chain(const PnpChainArgs& a, hipStream_t s);
// one solvePnP on the device (ssm_pnp_solve): n correspondences, T (16 doubles, device) in / out
struct PnpSolveArgs {
    const float *img, *obj; int n; ssm_pnp::Camera cam; double* T; uint8_t *inl, *dec; struct LEdge* ledges; double2* err; int32_t* n_inliers;
    int edges_in_lds;                                // set by k_pnp_solve
    // the cluster form (round 6): `blocks` (1 or 8) blocks solve the list together like a chain's cluster does -- inl / dec / ledges / err hold `blocks` slices of
    // `slice` entries (block b's private copy; slice 0 is the result), xchg / xfail as in PnpChainArgs; T and n_inliers are written by block 0
    int blocks; size_t slice; unsigned long long* xchg; unsigned* xfail;
    unsigned seq_base;                               // first pass number of this launch: the ring is NOT zeroed per launch -- pass tags keep rising from launch to launch (the caller zeroes the ring when the numbers wrap), and xfail is a word the caller uploads as 0
};
hipError_t k_pnp_solve(const PnpSolveArgs& a, hipStream_t s);
size_t k_pnp_edge_bytes(void);
size_t k_pnp_lds_edge_capacity(void);               // the largest n (k_pnp_solve) / R * cap (k_pnp_chain) whose edge list the kernels keep in LDS
