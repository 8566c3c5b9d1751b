// ssm_seq_plan.cpp -- the schedule of the sequence calls (ssm_seq_plan.h): no HIP header, no context; ssm_abi.hip and ssm_stereo_abi.hip carry it out.
#include "ssm_seq_plan.h"

SeqPlan seq_plan(const SeqShape& s)
{
    SeqPlan p;
    const bool orb = (s.stages & SSM_STAGE_ORB) != 0, segnet = (s.stages & SSM_STAGE_SEGNET) != 0;
    // Beside: the ORB -> match chain of a sub-batch and its (SegNet ->) map stage share no data, only the inputs, so the map side runs on a side lane.  The
    // chain's latency-bound kernels (pyramid, octree, describe) then overlap VALU/MFMA-bound map / SegNet work.
    const bool side_work = (s.stages & (SSM_STAGE_MAP | SSM_STAGE_SEGNET)) != 0;
    // Chains: without the SegNet stage (one activation workspace) and with two or more sub-batches, successive sub-batches run their whole ORB -> match chain on
    // the main lane, on side 0 and (from three sub-batches on, +2 %) on side 2 with an ORB workspace each, so that one chain's latency-bound kernels (quad-tree,
    // pyramid launches, block tails) overlap the other chains' VALU-bound ones (+6 % from the second chain).  Profiling mode 2 (serialize) keeps everything on
    // the main lane; the chains go with the streaming fused map kernels, i.e. widths that are a multiple of 16.
    const bool chains = !s.serialize && !segnet && s.n > s.B && orb && s.wide16;
    const bool beside = side_work && !s.serialize && !chains;
    p.nch = chains ? (s.n > 2 * s.B ? 3 : 2) : 1;
    // With several chains the map stage, which shares no data with them, runs on a lane of its own (all sub-batches in order, one workspace), so that the
    // chains' latency-bound kernels (pyramid, quad-tree, orientation / BRIEF gathers) always have VALU-bound map work beside them: +4 % over map-after-match on
    // the chain's own lane, which SSM_MAP_STREAM=0 keeps.
    const bool map_own = chains && s.map_own_stream == 1;
    p.needs_side_streams = beside || chains;
    p.needs_alt_work = chains;
    if (p.needs_side_streams) {
        p.forked.add(LANE_SIDE0);
        if (p.nch == 3) p.forked.add(LANE_SIDE2);
        if (map_own) p.forked.add(LANE_SIDE1);          // (whether or not the call has map work)
    }
    // one side lane, or the main lane: serialised, no map stage, or the chains' own lanes in turn, which the join puts behind the main lane
    p.map_tail = map_own ? LANE_SIDE1 : beside ? LANE_SIDE0 : LANE_MAIN;
    static const SeqLane chain_lane[3] = {LANE_MAIN, LANE_SIDE0, LANE_SIDE2};
    int bi = 0;
    for (int f0 = 0; f0 < s.n; f0 += s.B, bi++) {
        SeqStep st = {};
        st.f0 = f0; st.nb = s.n - f0 < s.B ? s.n - f0 : s.B;
        st.chain = bi % p.nch; st.lane = chain_lane[st.chain];
        st.map_lane = !side_work ? LANE_NONE : map_own ? LANE_SIDE1 : beside ? LANE_SIDE0 : st.lane;
        // Chain 1 enqueues its map stage FIRST: with the map stage on the chain's own lane that puts the chains half a sub-batch out of step (+2.4 %)
        st.map_first = chains && st.chain == 1;
        // The matcher of sub-batch bi reads the descriptor rows of the R preceding FRAMES, with max_batch < tracker_ref_frames those of several preceding
        // sub-batches.  It waits for the newest ORB + expand of every other chain, i.e. of sub-batches bi-1 .. bi-(nch-1); an older sub-batch sits on one of those
        // lanes, or on this one, in front of that.  (host/test_seq_plan.cpp checks this over every shape.)
        st.record_orb_done = chains;
        for (int k = 1; chains && k < p.nch && k <= bi; k++) st.wait_chain[st.nwait++] = (bi - k) % p.nch;
        p.steps.push_back(st);
    }
    return p;
}

StereoPlan stereo_plan(int n, int B, int stages, bool serialize, int sgbm_streams)
{
    StereoPlan p;
    // The quad matcher + VO chain (many small latency-bound kernels) and SGBM (volume kernels) of a sub-batch share nothing but the input images: SGBM runs on
    // the first side lane beside the chain; sub-batches follow each other on both without a join in between
    p.two = (stages & SSM_STEREO_DEPTH) && (stages & SSM_STEREO_QUAD) && !serialize;
    // ... and with more than one sub-batch SGBM alternates between TWO (sgbm_streams: up to three) lanes with a workspace each: the cost kernel and the small
    // kernels of one sub-batch (LDS / latency-bound) run beside the scan-direction and winner-takes-all kernels of the other (HBM-bound)
    const int nsub = (n + B - 1) / B;
    p.nsg = p.two ? (sgbm_streams < nsub ? sgbm_streams : nsub) : 1;
    if (p.two) { p.sgbm[0] = LANE_SIDE0; for (int k = 0; k < 3 && (k == 0 || k < p.nsg); k++) p.forked.add(p.sgbm[k]); }
    return p;
}
