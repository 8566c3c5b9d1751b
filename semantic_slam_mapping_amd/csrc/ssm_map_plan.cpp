// ssm_map_plan.cpp -- the decisions of the growable voxel map (ssm_map_plan.h): no HIP header, no context; ssm_map.hip carries them out.
#include "ssm_map_plan.h"
#include <algorithm>

int64_t map_list_records(const MapDims& d, bool small) { return small ? (int64_t)d.small_records : (int64_t)d.small_records + (int64_t)d.resident_blocks * d.block_records; }
int64_t map_high_water(const MapDims& d, int64_t ovf_cap, int64_t blocks) { return ovf_cap - std::min<int64_t>(d.resident_blocks, blocks) * d.block_records; }

bool MapGov::launch_needs_settle() const
{
    const uint64_t old = ring_serial[serial & 7u];
    if (!old) return false;
    if (old > seen) return true;
    for (const Skipped& k : skipped) if (k.serial == old) return true;
    return false;
}
// The arguments go into a ring of eight; the ring slot is the tag the launch's skipped blocks carry
int MapGov::begin_launch(const MapLaunch& L, int64_t blocks)
{
    if (blocks > dims.skip_cap / 4) return -1;
    const int tag = (int)(serial++ & 7u);
    ring[tag] = L; ring_serial[tag] = serial;
    unexamined = true;
    return tag;
}
// The table is re-hashed into a larger one whenever 4 x (voxels + overflow records + reserve) exceeds its slots -- `reserve` = new voxels the caller is about to
// add at most, so that an insert / merge of a known size can never overflow.  lo: overflow records [0, lo) are merged already
MapStep MapGov::settle_step(const int32_t cnt[8], int lo, int64_t reserve, int cap_log2, int ovf_cap) const
{
    MapStep a;
    if (cnt[6] > 0) { a.kind = MapStep::TAKE_SKIPS; a.ids = cnt[6] < dims.skip_cap ? cnt[6] : dims.skip_cap; return a; }
    const int64_t n = cnt[0], hi = cnt[2] < ovf_cap ? cnt[2] : ovf_cap, m = hi - lo;
    const int64_t slots = (int64_t)1 << cap_log2;
    const bool grow = 4 * (n + m + reserve) > slots && cap_log2 < vox_max_log2;
    if (!grow && 2 * (n + m + reserve) > slots && (m > 0 || reserve > 0)) {
        // at voxel_max_capacity_log2 and more than half full with something still to place.  A caller that announced its insert (reserve) is refused before
        // anything is added; records waiting in the overflow list have no table to go to: the map is incomplete from here on (flag bit 0, reported until
        // ssm_map_clear).  (A complete map that is merely more than half full at the cap stays readable: nothing to place, nothing refused -- ADVICE r05.)
        a.kind = MapStep::REFUSE; a.write_lost = m > 0;
        return a;
    }
    if (m <= 0 && !grow) { a.kind = skipped.empty() ? MapStep::REST : MapStep::REDO; a.reset_list = cnt[2] != 0; return a; }
    if (grow) {
        int L = cap_log2; while (L < vox_max_log2 && 4 * (n + m + reserve) > ((int64_t)1 << L)) L++;
        a.kind = MapStep::GROW; a.new_log2 = L;
        return a;
    }
    a.kind = MapStep::MERGE; a.lo = lo; a.hi = (int)hi; a.brim = hi >= ovf_cap;
    return a;
}
void MapGov::take_skips(const int32_t* ids, int n)
{
    for (int i = 0; i < n; i++) skipped.push_back({ids[i], ring_serial[(ids[i] >> 24) & 7]});
}
// The map is at rest and its list is empty: the batch adds to the table what it can and the rest to the list; map_settle then merges, grows, goes on
bool MapGov::redo_batch(int ovf_cap, std::vector<int32_t>& batch, MapLaunch& L, int& tag)
{
    const Skipped newest = skipped.back();
    tag = (newest.id >> 24) & 7;
    if (!newest.serial || ring_serial[tag] != newest.serial) return false;
    L = ring[tag];
    const size_t room = (size_t)(ovf_cap / dims.block_records);
    batch.clear();
    for (size_t i = skipped.size(); i-- > 0 && batch.size() < room; )
        if (((skipped[i].id >> 24) & 7) == tag && skipped[i].serial == newest.serial) { batch.push_back(skipped[i].id); skipped.erase(skipped.begin() + (long)i); }
    redone += (long)batch.size();
    return true;
}
void MapGov::learn_rate(int64_t total, int64_t at_frames) { if (at_frames > 0 && total > 0) { const double v = (double)total / (double)at_frames; if (v > vpf) vpf = v; } }
void MapGov::settled_exact(int64_t voxels)
{
    learn_rate(voxels, frames);
    launches = 0; known_total = voxels; known_frames = frames;
}
// The expectation is the stream's own rate: voxels (+ overflow records) per frame fused since the last clear, the largest value seen (vpf); x 1.5 is what a launch
// is granted.
//   * a context that has no rate yet takes ONE frame and is settled behind it (the one wait of its lifetime): a first launch of a whole sub-batch at a leaf far below
//     the pixel footprint would add more than table + overflow list hold, and what is dropped cannot be recovered;
//   * a small table (< 2^20 slots) is settled exactly in front of every launch, grown for the launch's expectation, and takes at most slots / 4096 frames;
//   * a large one is looked at through the counters of the launch BEFORE the previous one (a two-slot ring of asynchronous copies: the host never waits for the
//     launch it has just queued) and settled -- grown for the expectation -- when it is a quarter full, when its overflow list is in use, or when the frames queued
//     since that snapshot plus this launch are expected to fill it beyond a half.
int MapGov::snapshot_to_read(int cap_log2) const { return vpf >= 0 && cap_log2 >= 20 && launches >= 2 ? (int)(launches & 1) : -1; }
MapBefore MapGov::before_launch(int cap_log2, int remaining, const int32_t* snap)
{
    if (vpf < 0) return {1, MapBefore::SETTLE, 0};                 // no rate yet (first_frames learns it behind this frame)
    const double grant = vpf * 1.5;
    const int64_t slots = (int64_t)1 << cap_log2;
    if (cap_log2 < 20) {
        int f = (1 << cap_log2) >> 12; f = f < 1 ? 1 : (f > remaining ? remaining : f);
        return {f, MapBefore::SETTLE_EXACT, (int64_t)(f * grant)};
    }
    const MapBefore exact = {remaining, MapBefore::SETTLE_EXACT, (int64_t)(remaining * grant)}, go = {remaining, MapBefore::NONE, 0};
    if (launches < 2)          // no snapshot of this run of launches yet: the table was settled when the run began (frames counts what has been queued since)
        return 2.0 * ((double)known_total + (double)(frames - known_frames + remaining) * grant) > (double)slots ? exact : go;
    const int slot = (int)(launches & 1);
    const int64_t total = (int64_t)snap[0] + snap[2], at = snap_frames[slot];
    learn_rate(total, at);
    known_total = total; known_frames = at;
    if (snap[6] == 0 && snap_serial[slot] > seen) seen = snap_serial[slot];          // (with skipped blocks in sight the settle below takes them over)
    const double expect = (double)total + (double)(frames - at + remaining) * grant;
    return snap[2] > 0 || snap[6] > 0 || 4 * (int64_t)snap[0] > slots || 2.0 * expect > (double)slots ? exact : go;      // (snap[6]: blocks skipped themselves)
}
void MapGov::first_frames(int64_t voxels)
{
    if (vpf < 0) vpf = 1.0;                                          // (nothing was fused: every pixel gated; the next launches are granted little and watched)
    known_total = voxels; known_frames = frames;
}
int MapGov::begin_snapshot()
{
    const int slot = (int)(launches++ & 1);
    snap_frames[slot] = frames; snap_serial[slot] = serial;
    return slot;
}
void MapGov::clear()
{
    full_reported = false; launches = 0; frames = 0; known_total = 0; known_frames = 0;
    skipped.clear(); for (uint64_t& s : ring_serial) s = 0;         // (blocks that skipped themselves belong to the map that is cleared)
}
