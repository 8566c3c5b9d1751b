// ssm_map_plan.h -- the growth and redo protocol of the context's voxel map as host arithmetic (ssm_map_plan.cpp): how many frames a fused map launch takes, when
// the table is settled, grown or refused at its cap, which self-skipped blocks are run again and against which launch's arguments.  Plain C++ without a HIP header
// and without ssm_ctx.h: every decision is a function of MapGov and the counter block it is shown, and returns what the device leg (ssm_map.hip) is to do; nothing
// here copies, waits or launches.  host/test_map_plan.cpp drives it over a model device.  Not installed.
#pragma once
#include <cstdint>
#include <vector>
#ifndef SSM_HIDDEN
#define SSM_HIDDEN __attribute__((visibility("hidden")))
#endif

static const int VOX_OVF_RECORDS = 1 << 18;          // 29 MB per context; a context that runs the fused map stage (ssm_seq_process) trades it for the large list of map_ensure_stream_list
// one launch of the fused map stage, kept so that blocks it skipped can be run again (MapGov::redo_batch)
struct MapLaunch { const uint16_t* depth; const uint8_t* rgb; const uint8_t* sem; const double* pose; int n, w, h; int32_t* npoints; };
// what the map kernel fixes (kernels_map.hip k_map_fuse_*()): ints in the skip list, overflow records one block appends at most, blocks the device holds at a time;
// and the records of the small overflow list
struct MapDims { int skip_cap = 0, block_records = 1, resident_blocks = 0, small_records = VOX_OVF_RECORDS; };
// The fused map stage needs an overflow list that can take what every resident block may still append after the last block passed its high-water check
// (kernels_map.hip map_stream2_kernel): the small list as head room + resident blocks x records per block (2^18 + 1024 x 12288 records of 112 B: 1.4 GB of the
// device's 288).  small: SSM_MAP_TEST_SMALL_LIST -- keep the small list: every block then skips itself and is run again, 21 at a time
SSM_HIDDEN int64_t map_list_records(const MapDims& d, bool small);
SSM_HIDDEN int64_t map_high_water(const MapDims& d, int64_t ovf_cap, int64_t blocks);          // a block of a launch of `blocks` blocks that starts with more records in the list skips itself

// one round of map_settle: what to do with the counter block just read
struct MapStep {
    enum Kind {
        TAKE_SKIPS,        // blocks skipped themselves: copy `ids` ids from the device list, reset its count, MapGov::take_skips, ask again with cnt[6] = 0
        REFUSE,            // at the cap, more than half full, something still to place: SSM_E_CAPACITY -- after raising flag bit 0 when write_lost (records have no table to go to)
        REST,              // the map is at rest (reset_list: write 0 to cnt[2] first)
        REDO,              // at rest, but skipped blocks are pending (reset_list as for REST): MapGov::redo_batch, launch, next round
        GROW,              // re-hash into a table of 2^new_log2 slots, next round
        MERGE              // merge the overflow records [lo, hi); brim: the list was full to its end, empty it before anything can be appended again
    } kind;
    int ids = 0, new_log2 = 0, lo = 0, hi = 0; bool write_lost = false, reset_list = false, brim = false;
};
// map_before_launch: the frames the launch takes and what has to happen in front of it
struct MapBefore { int nq; enum Act { NONE, SETTLE, SETTLE_EXACT } act; int64_t reserve; };

// All host state of the protocol.  THE RING: every fused launch gets a serial (1, 2, ..) and its arguments go into slot serial & 7 -- the tag its skipped blocks
// carry on the device, (tag << 24) | block.  An id taken over from the device is stored with the serial its slot held at that moment, and redo_batch refuses ids
// whose slot holds another serial by then.  Invariant: a slot is overwritten only when the host has looked at the counters behind its launch (seen) and holds no
// id of it; launch_needs_settle() says when a launch has to settle first (ssm_seq_process looks at the counters at most a few launches late: it never does there).
struct SSM_HIDDEN MapGov {
    static const int SETTLE_ROUNDS = 4096;
    MapDims dims; int vox_max_log2 = 28;
    MapLaunch ring[8] = {}; uint64_t ring_serial[8] = {};          // launches that may still have skipped blocks (0: arguments not known)
    uint64_t serial = 0, seen = 0;                                  // launches begun; the newest the host has seen the counters behind
    struct Skipped { int32_t id; uint64_t serial; };
    std::vector<Skipped> skipped;                                   // ids to run again
    bool unexamined = false;                                        // a fused map launch was queued since the counters were last read on a drained stream
    bool full_reported = false;                                     // table-full already reported by check_device_flags (reset by clear)
    int grown = 0; long redone = 0;                                 // re-hashes and blocks run again so far (ssm_map_stats)
    double vpf = -1.0;                                              // voxels (+ overflow records) per fused frame, the largest rate seen on this context; < 0: none yet
    uint64_t launches = 0;                                          // snapshots queued since the map was last settled exactly
    int64_t frames = 0, snap_frames[2] = {0, 0}, known_total = 0, known_frames = 0;      // frames fused since the last clear; at the ring's snapshots; the last count the host has seen and when
    uint64_t snap_serial[2] = {0, 0};                               // the newest launch in front of each snapshot

    // ---- a fused launch
    bool launch_needs_settle() const;                               // the slot the next launch takes still belongs to a launch with ids pending or counters unseen
    int begin_launch(const MapLaunch& L, int64_t blocks);           // -> its tag, or -1: more than skip_cap / 4 blocks (nothing recorded)
    // ---- map_settle
    bool needs_drained_read(const int32_t cnt[8]) const { return unexamined || cnt[6] > 0; }      // the counters count only once every launch stream has drained: read them again then
    void read_drained() { unexamined = false; seen = serial; }
    MapStep settle_step(const int32_t cnt[8], int lo, int64_t reserve, int cap_log2, int ovf_cap) const;
    void take_skips(const int32_t* ids, int n);
    // the next batch of skipped blocks: those of the newest id's launch, newest first, as many as the list can take whole.  false: its arguments are no longer known
    bool redo_batch(int ovf_cap, std::vector<int32_t>& batch, MapLaunch& L, int& tag);
    void settled_exact(int64_t voxels);                             // map_settle_exact: the count just read is the newest the host knows, the estimates start from it
    // ---- map_before_launch / map_after_launch
    int snapshot_to_read(int cap_log2) const;                       // the snapshot slot before_launch needs (wait for its event first), or -1
    MapBefore before_launch(int cap_log2, int remaining, const int32_t* snap);      // snap: that slot's 8 counters (null: none needed)
    void first_frames(int64_t voxels);                              // the context's first frames are settled exactly: a rate of 1 if they fused nothing
    int begin_snapshot();                                           // -> the slot the counters behind the launch just queued are copied to
    void clear();                                                   // ssm_map_clear (the rate is the stream's: kept)
private:
    void learn_rate(int64_t total, int64_t at_frames);
};
