// cloud_table.h -- the cloud-segment table of the stages that walk one thread per point over the concatenation of m device-resident clouds:
// free-space carving, map rendering and dense alignment.  HIP-free for the host's half (ssm_cloud_table.cpp builds it, ssm_cloud_list.hip checks a call's clouds
// and uploads it); the device's half below.  A call's used points are numbered through, cloud after cloud; a BLOCK is T consecutive numbers (a thread block, or a
// chunk of alignment's persistent blocks).  In device memory: CloudSeg[m], then blk[blocks], the cloud of each block's first point.  When the whole block lies in
// that cloud (all but at most m - 1 blocks do) the cloud's index is uniform: the test reads the record's off and n through scalar loads, and every lane then reads
// the same record; a block that a cloud boundary crosses takes the same code with a per-lane index.  An empty cloud shares its off with the cloud behind it and is
// stepped over: never a block's first cloud.
#pragma once
#include <stdint.h>
#include "../../include/ssm_hip.h"

// pts: the cloud's points (every stage; carving writes the kept ones back).  run: their run counters -- carving alone, null otherwise.  off: the number of its
// first USED point; n: how many are used; stride: the step between them -- alignment alone, 1 otherwise.  M: the relative pose view <- cloud (carve_core.h rel_pose)
struct CloudSeg { ssm_point* pts; uint8_t* run; int64_t off; int32_t n, stride; double M[12]; };
static_assert(sizeof(CloudSeg) == 128, "a record is 128 bytes: seg[k] is a shift, M starts on a 32-byte boundary");

#ifdef __HIPCC__
// I, the type of a point's number: int64_t, but int in carving, whose calls end at 2^30 points -- its kernels number, compare and address in 32 bits as before the
// record was shared (off is converted where it is read), which keeps their registers and instruction counts.
// Is the block of T points that starts at `first` wholly inside cloud k0, the cloud of its first point?  (total: the points of the call)
template <class I> __device__ inline bool cloud_block_uniform(const CloudSeg* __restrict__ seg, int k0, I first, int T, I total) { return min(total, first + T) - 1 < (I)seg[k0].off + seg[k0].n; }
// the cloud of point g (g < total) of a block whose first point is in cloud k0
template <class I> __device__ inline int cloud_of(const CloudSeg* __restrict__ seg, int k0, bool uniform, I g)
{
    int k = k0;
    if (!uniform) while (g >= (I)seg[k].off + seg[k].n) k++;          // (ends: g < total = the last cloud's off + n; empty clouds are stepped over)
    return k;
}
#endif
