// pnp_state.h -- the ONE definition of the pose chain's state block: what the tracker's host state machine (ssm_track_host.cpp, through ssm_host.h) fills and adopts,
// the device leg (ssm_track.hip) moves and the chain kernel (kernels_pnp.hip, through pnp_chain.h) walks.  Plain C: no HIP header.  Not installed.
// SSM_PNP_PROF changes the layout: an ablation build defines it for every source that includes this (scripts/build_pnp_prof.sh).
#pragma once
#include <stdint.h>
#define SSM_TRACK_MAXREF 64
// the Tracker's state while the chain runs on the device (device memory; the host uploads it before a run and reads it back after)
struct PnpState {
    double speed[16], last_pose[16];                 // column-major 4 x 4
    double ref_pose[SSM_TRACK_MAXREF][16];           // refFrames deque, oldest first
    int32_t ref_idx[SSM_TRACK_MAXREF];               // their frame indices relative to the current ssm_seq_process call (negative: frames of the previous call)
    int32_t nref, cnt_lost, stopped_at, pad;
    long long work[4];                               // out: fused passes, chi2 passes, active edges evaluated by the fused / by the chi2 passes of this launch
#ifdef SSM_PNP_PROF
    long long prof[32];                              // shader clocks per section (thread 0), ablation builds only
#endif
};
