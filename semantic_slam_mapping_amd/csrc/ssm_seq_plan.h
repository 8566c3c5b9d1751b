// ssm_seq_plan.h -- the schedule of the two sequence calls as host arithmetic (ssm_seq_plan.cpp): which lane of the context every ORB -> match chain, the map stage
// and SGBM of a sub-batch run on, which chains' events a matcher waits for, which lanes a call forks and joins.  Plain C++ without a HIP header and without
// ssm_ctx.h: a plan is a function of the call's shape, and nothing here launches, records or waits -- ssm_seq_process (ssm_abi.hip) and stereo_seq_run
// (ssm_stereo_abi.hip) carry it out.  host/test_seq_plan.cpp checks the decisions and, over a model of streams and events, the ordering they give.  Not installed.
#pragma once
#include "../../include/ssm_hip.h"
#include <vector>
#ifndef SSM_HIDDEN
#define SSM_HIDDEN __attribute__((visibility("hidden")))
#endif

// The lanes of a context (ssm_ctx::main, side[0..2]; ssm_ctx.h lane()).  Who runs where is decided here and nowhere else:
//   LANE_MAIN   every per-call entry point; chain 0 of ssm_seq_process; the quad matcher + VO chain of the stereo path
//   LANE_SIDE0  chain 1; beside a single chain the (SegNet ->) map stage of every sub-batch.  Stereo: SGBM, first workspace
//   LANE_SIDE1  with several chains the map stage on a stream of its own (SSM_MAP_STREAM=0: on the chains' lanes in turn).  Stereo: SGBM, second workspace
//   LANE_SIDE2  chain 2, from three sub-batches on.  Stereo: SGBM, third workspace
enum SeqLane { LANE_NONE = -1, LANE_MAIN, LANE_SIDE0, LANE_SIDE1, LANE_SIDE2 };
// the side lanes a call forks from the main lane and joins into it, in that order
struct LaneList { int n = 0; SeqLane lane[3] = {LANE_NONE, LANE_NONE, LANE_NONE}; void add(SeqLane l) { lane[n++] = l; } };

// what ssm_seq_process' schedule depends on: frames, frames per sub-batch (max_batch), SSM_STAGE_* bits, profiling mode 2, width a multiple of 16, SSM_MAP_STREAM
struct SeqShape { int n, B, stages; bool serialize, wide16; int map_own_stream; };
// one sub-batch: frames [f0, f0 + nb) on ORB chain `chain`, which runs on `lane`
struct SeqStep {
    int f0, nb, chain; SeqLane lane;
    SeqLane map_lane;             // the lane of its (SegNet ->) map stage; LANE_NONE: the call has neither
    bool map_first;               // enqueue that stage in front of ORB -> match
    bool record_orb_done;         // record the chain's orb_done behind ORB + expand, then wait for orb_done of wait_chain[0 .. nwait) in that order, then match
    int nwait, wait_chain[2];
};
struct SeqPlan {
    int nch = 1;                                                    // ORB chains in use
    bool needs_side_streams = false, needs_alt_work = false;        // the side lanes exist / chains 1, 2 have workspaces before anything is enqueued
    LaneList forked;
    SeqLane map_tail = LANE_MAIN;                                   // where the map's newest work sits once the call is enqueued (MapDev::tail; LANE_MAIN: joined)
    std::vector<SeqStep> steps;
};
SSM_HIDDEN SeqPlan seq_plan(const SeqShape& s);

// the stereo sequence path: the quad matcher + VO chain stays on the main lane, SGBM of sub-batch k runs on lane(k) with workspace work(k)
struct StereoPlan {
    bool two = false; int nsg = 1;                                  // SGBM beside the chain; SGBM lanes (and workspaces) in use
    LaneList forked;
    SeqLane sgbm[3] = {LANE_MAIN, LANE_SIDE1, LANE_SIDE2};
    int work(int k) const { return k % nsg; }
    SeqLane lane(int k) const { return sgbm[k % nsg]; }
};
SSM_HIDDEN StereoPlan stereo_plan(int n, int B, int stages, bool serialize, int sgbm_streams);
