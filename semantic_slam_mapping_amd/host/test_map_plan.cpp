// test_map_plan.cpp -- the voxel map's growth and redo protocol (csrc/ssm_map_plan.cpp over csrc/ssm_map_plan.h) as a stand-alone program: it links that one
// source, so it needs neither libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers (make SAN=asan san; make test_map_plan_san).
//   1. decision tables: every action of before_launch, settle_step, begin_launch and the list sizes on hand-computed inputs (the expected values restate the rules
//      of DESIGN.md s.3 -- 4 x / 2 x (voxels + records + reserve) against the slots, the four regimes in front of a launch -- not the code under test);
//   2. the redo batch: one launch only, newest first, never more than the overflow list takes whole;
//   3. the ring: ids whose slot was given to a later launch are refused, and launch_needs_settle() fires before that can happen;
//   4. a model device (a voxel count, overflow records, a skip list, flags) under the device leg's loops, restated here, over seeded random scripts: every settle
//      ends within the round bound, at rest or in the one refusal, and every contribution offered is in the table.
#include "../csrc/ssm_map_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <deque>
#include <random>
using namespace std;

static int failures = 0; static long checks = 0; static unsigned g_seed = 0;
static void check(bool ok, const char* what)
{
    checks++;
    if (ok) return;
    if (failures++ < 40) printf("FAIL %s (script %u)\n", what, g_seed);
}
static const MapDims REAL = {65536, 12288, 1024, 1 << 18};          // kernels_map.hip: MS2_SKIP_CAP, MS_CH x 4096, 256 x MS2_MINB; VOX_OVF_RECORDS
static MapGov gov(const MapDims& d = REAL, int vox_max = 28) { MapGov g; g.dims = d; g.vox_max_log2 = vox_max; return g; }
static void counters(int32_t c[8], int voxels, int flags, int records, int skipped) { memset(c, 0, 32); c[0] = voxels; c[1] = flags; c[2] = records; c[6] = skipped; }

// ---------------------------------------------------------------- 1. decision tables
static void test_lists_and_begin()
{
    check(map_list_records(REAL, true) == 262144 && map_list_records(REAL, false) == 262144 + (int64_t)1024 * 12288, "list records: small, and head room + resident x per block");
    const int64_t cap = map_list_records(REAL, false);
    check(map_high_water(REAL, cap, 6250) == 262144 && map_high_water(REAL, cap, 25) == cap - 25 * 12288, "high water: resident blocks, or the launch's if fewer");
    check(map_high_water(REAL, 262144, 6250) == 262144 - (int64_t)1024 * 12288, "high water of the small list is negative: every block skips");
    MapGov g = gov();
    MapLaunch L = {}; L.n = 7;
    check(g.begin_launch(L, 16385) == -1 && g.serial == 0 && !g.unexamined && !g.ring_serial[0], "more than skip_cap / 4 blocks: refused, nothing recorded");
    check(g.begin_launch(L, 16384) == 0 && g.serial == 1 && g.unexamined && g.ring_serial[0] == 1 && g.ring[0].n == 7, "first launch: tag 0, serial 1");
    for (int k = 1; k < 8; k++) { g.read_drained(); check(g.begin_launch(L, 1) == k, "tags count up"); }
    g.read_drained();
    check(!g.launch_needs_settle() && g.begin_launch(L, 1) == 0 && g.ring_serial[0] == 9, "the ninth launch takes slot 0 again");
}
static bool is(const MapBefore& b, int nq, MapBefore::Act act, int64_t reserve) { return b.nq == nq && b.act == act && b.reserve == reserve; }
static void test_before_launch()
{
    { MapGov g = gov(); check(g.snapshot_to_read(24) == -1 && is(g.before_launch(24, 250, nullptr), 1, MapBefore::SETTLE, 0), "no rate: one frame, settle(0)"); }
    { MapGov g = gov(); g.vpf = 100; check(g.snapshot_to_read(10) == -1 && is(g.before_launch(10, 250, nullptr), 1, MapBefore::SETTLE_EXACT, 150), "2^10: one frame, exact 150"); }
    { MapGov g = gov(); g.vpf = 100; check(is(g.before_launch(16, 250, nullptr), 16, MapBefore::SETTLE_EXACT, 2400), "2^16: 16 frames"); }
    { MapGov g = gov(); g.vpf = 100; check(is(g.before_launch(19, 100, nullptr), 100, MapBefore::SETTLE_EXACT, 15000), "2^19: 128 frames at most, 100 remain"); }
    { MapGov g = gov(); g.vpf = 100; g.launches = 5; check(g.snapshot_to_read(19) == -1, "a small table reads no snapshot"); }
    // no snapshot yet: 2 x (known + (queued + remaining) x 1.5 rate) against 2^20
    { MapGov g = gov(); g.vpf = 1398; check(g.snapshot_to_read(20) == -1 && is(g.before_launch(20, 250, nullptr), 250, MapBefore::NONE, 0), "2 x 250 x 2097 = 1048500 <= 2^20: nothing"); }
    { MapGov g = gov(); g.vpf = 1399; check(is(g.before_launch(20, 250, nullptr), 250, MapBefore::SETTLE_EXACT, 524625), "rate 1399: exact 524625"); }
    { MapGov g = gov(); g.vpf = 1000; g.known_total = 149288; g.frames = 300; g.known_frames = 100; g.launches = 1;          // 200 frames queued since the count, 50 remain
      check(is(g.before_launch(20, 50, nullptr), 50, MapBefore::NONE, 0), "known total + queued frames, at the threshold: 2 x (149288 + 250 x 1500) = 2^20");
      g.known_total = 149289; check(is(g.before_launch(20, 50, nullptr), 50, MapBefore::SETTLE_EXACT, 75000), "one voxel more: settle"); }
    // snapshot regime: slot launches & 1; each trigger alone, at and below its threshold.  rate 10 -> grant 15; snapshot at frame 90 of 100, 10 remain: 20 frames x 15 = 300
    struct { int voxels, records, skipped; bool settle; const char* what; } T[] = {
        {1000, 0, 0, false, "nothing"}, {1000, 1, 0, true, "cnt[2] > 0"}, {1000, 0, 1, true, "cnt[6] > 0"},
        {262144, 0, 0, false, "4 x cnt[0] = slots"}, {262145, 0, 0, true, "4 x cnt[0] > slots"} };
    for (auto& t : T) {
        MapGov g = gov(); g.vpf = 10; g.launches = 3; g.frames = 100; g.snap_frames[1] = 90; g.snap_serial[1] = 2; g.serial = 3;
        int32_t c[8]; counters(c, t.voxels, 0, t.records, t.skipped);
        check(g.snapshot_to_read(20) == 1, "snapshot slot");
        const MapBefore b = g.before_launch(20, 10, c);
        check(t.settle ? is(b, 10, MapBefore::SETTLE_EXACT, 150) : is(b, 10, MapBefore::NONE, 0), t.what);
        check(g.known_total == t.voxels + t.records && g.known_frames == 90, "the snapshot becomes the known count");
        check(g.seen == (t.skipped ? 0u : 2u), "a snapshot without skips is a look at the launches in front of it");
    }
    for (int over = 0; over < 2; over++) {          // 2 x expect alone: rate 13512 -> grant 20268; snapshot at frame 94 of 100, 10 remain: 16 frames x 20268 = 324288 = 2^19 - 200000
        MapGov g = gov(); g.vpf = 13512; g.launches = 2; g.frames = 100; g.snap_frames[0] = 94;
        int32_t c[8]; counters(c, 200000 + over, 0, 0, 0);
        check(g.snapshot_to_read(20) == 0, "snapshot slot");
        const MapBefore b = g.before_launch(20, 10, c);
        check(over ? is(b, 10, MapBefore::SETTLE_EXACT, 202680) : is(b, 10, MapBefore::NONE, 0), over ? "2 x expect > slots" : "2 x expect = slots");
        check(g.vpf == 13512, "a snapshot's lower rate does not replace the largest seen");
    }
    { MapGov g = gov(); g.frames = 40; g.settled_exact(6000); check(g.vpf == 150 && g.launches == 0 && g.known_total == 6000 && g.known_frames == 40, "settled_exact learns 150 per frame");
      g.frames = 80; g.settled_exact(8000); check(g.vpf == 150 && g.known_total == 8000, "the rate is the largest seen"); g.settled_exact(0); check(g.vpf == 150, "no voxels: no rate learnt"); }
    { MapGov g = gov(); g.frames = 1; g.first_frames(0); check(g.vpf == 1.0 && g.known_frames == 1, "first frames that fused nothing: rate 1");
      check(g.begin_snapshot() == 0 && g.begin_snapshot() == 1 && g.begin_snapshot() == 0 && g.launches == 3 && g.snap_frames[1] == 1, "snapshot slots alternate"); }
    { MapGov g = gov(); MapLaunch L = {}; g.begin_launch(L, 1); g.read_drained(); const int32_t id = 5; g.take_skips(&id, 1); g.full_reported = true; g.frames = 9; g.launches = 4; g.known_total = 3; g.vpf = 7; g.grown = 2;
      g.clear(); check(g.skipped.empty() && !g.ring_serial[0] && !g.full_reported && !g.frames && !g.launches && !g.known_total && g.vpf == 7 && g.grown == 2 && g.serial == 1, "clear keeps the rate, the growth count and the serial"); }
}
static void test_settle_step()
{
    struct { int cap, vmax, voxels, records, lo, ovf; int64_t reserve; MapStep::Kind kind; int arg; bool flag; const char* what; } T[] = {
        // at rest
        {10, 28, 256, 0, 0, 1000, 0, MapStep::REST, 0, false, "a quarter full, nothing to place: at rest"},
        {10, 28, 100, 300, 300, 1000, 0, MapStep::REST, 0, true, "everything merged, the count still set: at rest behind a reset"},
        {10, 10, 900, 0, 0, 1000, 0, MapStep::REST, 0, false, "complete, more than half full at the cap, nothing to place: at rest"},
        // grow: 4 x (n + m + reserve) > slots, to the smallest L that fits or the cap
        {10, 28, 257, 0, 0, 1000, 0, MapStep::GROW, 11, false, "4 x 257 > 1024: 2^11"},
        {10, 28, 100, 100, 0, 1000, 57, MapStep::GROW, 11, false, "voxels + records + reserve = 257"},
        {8, 28, 0, 0, 0, 1000, 17000, MapStep::GROW, 17, false, "reserve 17000: 68000 <= 2^17"},
        {8, 28, 0, 0, 0, 1000, 16384, MapStep::GROW, 16, false, "reserve 16384: exactly 2^16"},
        {10, 12, 100000, 0, 0, 1000, 0, MapStep::GROW, 12, false, "no L fits: the cap"},
        {10, 28, 150, 500, 400, 1000, 0, MapStep::MERGE, 0, false, "records [0, 400) are merged already and count as voxels only: 4 x 250 <= 1024, no growth"},
        // refuse: at the cap, 2 x (..) > slots, something to place
        {10, 10, 500, 0, 0, 1000, 13, MapStep::REFUSE, 0, false, "announced insert at the cap: refused, no flag"},
        {10, 10, 500, 0, 0, 1000, 12, MapStep::REST, 0, false, "2 x 512 = slots: not refused"},
        {10, 10, 500, 13, 0, 1000, 0, MapStep::REFUSE, 0, true, "records without a table: refused, lost flag"},
        {10, 10, 400, 13, 0, 1000, 200, MapStep::REFUSE, 0, true, "records and reserve: lost flag (m > 0)"},
        // merge
        {10, 28, 100, 50, 0, 1000, 0, MapStep::MERGE, 0, false, "records to merge"},
        {10, 10, 400, 112, 0, 1000, 0, MapStep::MERGE, 0, false, "at the cap, half full with the records: merged"},
        {12, 28, 0, 1000, 0, 1000, 0, MapStep::MERGE, 0, true, "the list full to the brim"},
        {12, 28, 0, 5000, 0, 1000, 0, MapStep::MERGE, 0, true, "the count beyond the list's end: clamped, brim"},
        {12, 28, 0, 5000, 1000, 1000, 0, MapStep::REST, 0, true, "clamped count merged: at rest behind a reset"},
    };
    for (auto& t : T) {
        MapGov g = gov(REAL, t.vmax);
        int32_t c[8]; counters(c, t.voxels, 0, t.records, 0);
        const MapStep a = g.settle_step(c, t.lo, t.reserve, t.cap, t.ovf);
        bool ok = a.kind == t.kind;
        if (t.kind == MapStep::GROW) ok = ok && a.new_log2 == t.arg;
        if (t.kind == MapStep::REFUSE) ok = ok && a.write_lost == t.flag;
        if (t.kind == MapStep::REST) ok = ok && a.reset_list == t.flag;
        if (t.kind == MapStep::MERGE) ok = ok && a.lo == t.lo && a.hi == min(t.records, t.ovf) && a.brim == t.flag;
        check(ok, t.what);
    }
    MapGov g = gov();
    int32_t c[8]; counters(c, 100, 0, 50, 70000);
    MapStep a = g.settle_step(c, 0, 0, 10, 1000);
    check(a.kind == MapStep::TAKE_SKIPS && a.ids == 65536, "skips come first, at most the list's capacity");
    c[6] = 3; a = g.settle_step(c, 0, 0, 10, 1000); check(a.kind == MapStep::TAKE_SKIPS && a.ids == 3, "three skips");
    MapLaunch L = {}; g.begin_launch(L, 10); const int32_t ids[3] = {1, 2, 3}; g.take_skips(ids, 3);
    counters(c, 100, 0, 0, 0); a = g.settle_step(c, 0, 0, 10, 1000); check(a.kind == MapStep::REDO && !a.reset_list, "at rest with ids pending: redo");
    counters(c, 100, 0, 50, 0); a = g.settle_step(c, 0, 0, 10, 1000); check(a.kind == MapStep::MERGE, "records are merged before a redo");
    check(!g.needs_drained_read(c) || g.unexamined, "drained read: only unexamined or skips"); g.read_drained(); check(!g.needs_drained_read(c), "examined, no skips: one read"); c[6] = 1; check(g.needs_drained_read(c), "skips: read again");
}
// ---------------------------------------------------------------- 2. the redo batch, 3. the ring
static void test_redo_and_ring()
{
    MapDims d = REAL; d.block_records = 100;
    MapGov g = gov(d);
    MapLaunch A = {}, B = {}; A.n = 1; B.n = 2;
    const int ta = g.begin_launch(A, 50), tb = g.begin_launch(B, 50);
    g.read_drained();
    vector<int32_t> ids;
    for (int b = 0; b < 5; b++) { ids.push_back((ta << 24) | b); ids.push_back((tb << 24) | (10 + b)); }      // interleaved: a0 b10 a1 b11 ...
    g.take_skips(ids.data(), (int)ids.size());
    vector<int32_t> batch; MapLaunch L; int tag;
    check(g.redo_batch(350, batch, L, tag) && tag == tb && L.n == 2 && batch == vector<int32_t>({(tb << 24) | 14, (tb << 24) | 13, (tb << 24) | 12}), "the newest id's launch, newest first, 350 / 100 = 3");
    check(g.redo_batch(10000, batch, L, tag) && tag == ta && L.n == 1 && batch == vector<int32_t>({(ta << 24) | 4, (ta << 24) | 3, (ta << 24) | 2, (ta << 24) | 1, (ta << 24) | 0}) && g.skipped.size() == 2,
          "then the launch of the newest id left: all of A's, B's older ids stay");
    check(g.redo_batch(199, batch, L, tag) && tag == tb && L.n == 2 && batch == vector<int32_t>({(tb << 24) | 11}) && g.redone == 9, "one at a time when the list takes one block");
    check(g.skipped.size() == 1 && g.skipped[0].id == ((tb << 24) | 10) && g.skipped[0].serial == 2, "the id left is launch B's, with its serial");
    // ids taken over, then a failed settle (they stay), then eight launches that do not heed launch_needs_settle: the ids are refused, not run against the new launch
    int asked = 0;
    for (int k = 0; k < 8; k++) { if (g.launch_needs_settle()) { asked++; check((g.serial & 7) == (unsigned)tb, "the forced settle is asked for in front of B's slot"); } g.begin_launch(A, 1); g.read_drained(); }
    check(asked == 1, "exactly the launch that takes B's slot is asked to settle first");
    check(g.ring_serial[tb] == 10 && g.ring[tb].n == 1 && !g.redo_batch(10000, batch, L, tag) && g.skipped.size() == 1, "ids of a launch whose slot was given away: arguments no longer known, no batch");
    // ids that arrive after their slot was cleared carry serial 0
    MapGov h = gov(d); h.begin_launch(A, 1); h.clear(); const int32_t late = 0; h.take_skips(&late, 1);
    check(!h.redo_batch(1000, batch, L, tag), "ids of a cleared launch are refused");
    // a script that withholds every look at the counters: the ninth launch must ask for a settle (its slot's launch is unseen); after a look it does not
    MapGov w = gov(d);
    for (int k = 0; k < 8; k++) { check(!w.launch_needs_settle(), "eight launches fit the ring"); w.begin_launch(A, 1); }
    check(w.launch_needs_settle(), "the ninth launch without a look at the counters asks for a settle");
    w.read_drained(); check(!w.launch_needs_settle(), "a drained read is a look");
    w.begin_launch(A, 1);          // serial 9 in slot 0
    w.vpf = 1; w.launches = 2; w.snap_serial[0] = 2; int32_t c[8]; counters(c, 0, 0, 0, 0); w.seen = 0; w.before_launch(20, 1, c);
    check(w.seen == 2 && !w.launch_needs_settle(), "a snapshot behind launch 2 frees slot 1 (serial 2)");
    w.begin_launch(A, 1); check(w.launch_needs_settle(), "but not slot 2 (serial 3)");
}
// ---------------------------------------------------------------- 4. the model device
// Every contribution opens a voxel of its own.  The table takes contributions while fewer than 5/8 of its slots are taken, the rest is appended to the list
// (counted beyond its end, kept up to it: flag bit 0 beyond).  Blocks of a fused launch start `resident` at a time: all of them look at the list before any appends.
struct ModelLaunch { vector<int> per_block; vector<uint8_t> state; };          // state: 0 not run, 1 skipped (id on its way), 2 done
struct Model {
    MapDims d; int cap_log2 = 8, ovf_cap = 0, flags = 0; bool has_skip = false;
    int64_t voxels = 0, list = 0, pending = 0, offered = 0, dropped = 0;      // list: cnt[2]; pending: records appended and not merged yet
    vector<int32_t> skip;
    void add(int64_t k)
    {
        const int64_t limit = ((int64_t)5 << cap_log2) / 8, fit = max<int64_t>(0, min(k, limit - voxels)), rest = k - fit, room = max<int64_t>(0, ovf_cap - list);
        voxels += fit; list += rest; pending += min(rest, room);
        if (rest > room) { dropped += rest - room; flags |= 1; }
    }
    void merge(int64_t m) { pending -= m; add(m); }
    void fuse(ModelLaunch& ml, int64_t hw, int tag)
    {
        const int nb = (int)ml.per_block.size();
        for (int b0 = 0; b0 < nb; b0 += d.resident_blocks) {
            const int64_t at_start = list;
            for (int b = b0; b < nb && b < b0 + d.resident_blocks; b++) {
                offered += ml.per_block[b];
                if (at_start > hw) { skip.push_back((tag << 24) | b); ml.state[b] = 1; }
                else { add(ml.per_block[b]); ml.state[b] = 2; }
            }
        }
    }
    void redo(ModelLaunch& ml, const vector<int32_t>& ids)
    {
        for (int32_t id : ids) { const int b = id & 0xFFFFFF; check(b < (int)ml.state.size() && ml.state[b] == 1, "a redo runs a block that skipped itself, once, with its own launch"); if (b < (int)ml.state.size()) { add(ml.per_block[b]); ml.state[b] = 2; } }
    }
};
enum { OK = 0, E_INVAL = -1, E_CAPACITY = -4, E_STALE = -2, E_ROUNDS = -99 };
struct Leg {          // the device leg's loops (ssm_map.hip) over the model
    MapGov g; Model m; deque<ModelLaunch> launches; int32_t snap[16] = {}; bool small = false; int gx = 25; int max_rounds = 0, forced = 0;
    void read(int32_t c[8]) { counters(c, (int)m.voxels, m.flags, (int)min<int64_t>(m.list, 0x7fffffff), (int)m.skip.size()); }
    int settle(int64_t reserve)
    {
        int lo = 0;
        for (int round = 0; round < MapGov::SETTLE_ROUNDS; round++) {
            max_rounds = max(max_rounds, round + 1);
            int32_t c[8]; read(c);
            if (g.needs_drained_read(c)) { read(c); g.read_drained(); }
            MapStep a = g.settle_step(c, lo, reserve, m.cap_log2, m.ovf_cap);
            if (a.kind == MapStep::TAKE_SKIPS) {
                check(a.ids == (int)m.skip.size() && a.ids <= m.d.skip_cap, "the skip list is taken over whole");
                g.take_skips(m.skip.data(), a.ids); m.skip.clear(); c[6] = 0;
                a = g.settle_step(c, lo, reserve, m.cap_log2, m.ovf_cap);
                check(a.kind != MapStep::TAKE_SKIPS, "one take-over per round");
            }
            switch (a.kind) {
            case MapStep::REFUSE:
                check(m.cap_log2 == g.vox_max_log2, "a refusal only at the cap");
                check(a.write_lost == (m.pending > 0), "the lost flag exactly when records have no table to go to");
                if (a.write_lost) { m.flags |= 1; m.dropped += m.pending; m.pending = 0; m.list = 0; }
                return E_CAPACITY;
            case MapStep::REST: case MapStep::REDO: {
                check(a.reset_list == (m.list != 0), "the count is reset when it is set");
                if (a.reset_list) { check(m.pending == 0 || (m.flags & 1), "a reset never discards records still to merge"); m.list = 0; }
                lo = 0;
                if (a.kind == MapStep::REST) { check(g.skipped.empty() && m.skip.empty() && m.list == 0, "at rest: no ids, no records"); return OK; }
                vector<int32_t> batch; MapLaunch L; int tag;
                if (!g.redo_batch(m.ovf_cap, batch, L, tag)) return E_STALE;
                check(!batch.empty() && (int64_t)batch.size() * m.d.block_records <= m.ovf_cap, "a batch the empty list takes whole");
                for (int32_t id : batch) check(((id >> 24) & 7) == tag, "one tag per batch");
                m.redo(*const_cast<ModelLaunch*>(reinterpret_cast<const ModelLaunch*>(L.depth)), batch);
                break;
            }
            case MapStep::GROW:
                check(a.new_log2 > m.cap_log2 && a.new_log2 <= g.vox_max_log2, "a larger table, within the cap");
                check(a.new_log2 == g.vox_max_log2 || ((int64_t)1 << a.new_log2) >= 4 * (m.voxels + m.pending + reserve), "grown to fit 4 x what is known");
                check(a.new_log2 == m.cap_log2 + 1 || ((int64_t)1 << (a.new_log2 - 1)) < 4 * (m.voxels + m.pending + reserve), "and no further");
                m.cap_log2 = a.new_log2; g.grown++;
                break;
            default:
                check(a.lo == lo && a.hi > a.lo && a.hi <= m.ovf_cap && a.hi - a.lo == m.pending, "the merge takes exactly the records not merged yet");
                m.merge(a.hi - a.lo); lo = a.hi;
                check(a.brim == (lo >= m.ovf_cap), "brim");
                if (a.brim) { if (m.list > m.ovf_cap && !(m.flags & 1)) return E_CAPACITY; check(m.pending == 0, "nothing re-appended behind a full list"); m.list = 0; lo = 0; }
            }
        }
        return E_ROUNDS;
    }
    int settle_exact(int64_t reserve) { const int r = settle(reserve); if (r) return r; g.settled_exact(m.voxels); return OK; }
    int fuse_launch(int frames, int per_frame)
    {
        const int64_t want = map_list_records(m.d, small);
        if (!m.has_skip || m.ovf_cap < want) {
            const int r = settle(0); if (r) return r;
            m.has_skip = true;
            if (m.ovf_cap < want) { check(m.list == 0 && m.pending == 0, "the list is traded while empty"); m.ovf_cap = (int)want; }
        }
        const int64_t blocks = (int64_t)gx * frames;
        if (g.launch_needs_settle()) { forced++; const int r = settle(0); if (r) return r; }
        launches.emplace_back(); ModelLaunch& ml = launches.back();
        for (int f = 0; f < frames; f++) for (int b = 0; b < gx; b++) ml.per_block.push_back(per_frame / gx + (b < per_frame % gx));
        ml.state.assign(ml.per_block.size(), 0);
        MapLaunch L = {}; L.depth = reinterpret_cast<const uint16_t*>(&ml); L.n = frames;
        const int tag = g.begin_launch(L, blocks);
        if (tag < 0) { launches.pop_back(); return E_INVAL; }
        m.fuse(ml, map_high_water(m.d, m.ovf_cap, blocks), tag);
        check(m.dropped == 0, "a fused launch never drops: blocks beyond the high-water mark skip");
        return OK;
    }
    int before(int remaining, int* nq)
    {
        const int slot = g.snapshot_to_read(m.cap_log2);
        const MapBefore b = g.before_launch(m.cap_log2, remaining, slot >= 0 ? snap + 8 * slot : nullptr);
        *nq = b.nq;
        check(b.nq >= 1 && b.nq <= remaining, "a launch takes at least one frame and no more than remain");
        return b.act == MapBefore::SETTLE ? settle(b.reserve) : b.act == MapBefore::SETTLE_EXACT ? settle_exact(b.reserve) : OK;
    }
    int after(int frames, bool inputs_volatile)
    {
        g.frames += frames;
        if (inputs_volatile && g.vpf >= 0) { const int r = settle(0); if (r) return r; }
        if (g.vpf < 0) { const int r = settle_exact(0); if (r) return r; g.first_frames(m.voxels); return OK; }
        read(snap + 8 * g.begin_snapshot());
        return OK;
    }
    int sequence(int n, int B, int per_frame, bool inputs_volatile)          // ssm_seq_process' map stage
    {
        if (g.unexamined) { const int r = settle(0); if (r) return r; }
        for (int f0 = 0; f0 < n; f0 += B)
            for (int nb = min(B, n - f0), q0 = 0, nq; q0 < nb; q0 += nq) {
                int r = before(nb - q0, &nq); if (r) return r;
                r = fuse_launch(nq, per_frame); if (r) return r;
                r = after(nq, inputs_volatile); if (r) return r;
            }
        return OK;
    }
    int insert(int n, int distinct_pct)          // ssm_map_insert: chunks the table is grown for beforehand
    {
        for (int a = 0; a < n; ) {
            int64_t chunk = ((int64_t)1 << m.cap_log2) / 8; if (chunk < 4096) chunk = 4096; if (chunk > n - a) chunk = n - a;
            const int64_t before_v = m.voxels; const bool at_rest = m.pending == 0 && m.skip.empty() && g.skipped.empty();
            const int r = settle(chunk);
            if (r) { check(r != E_CAPACITY || !at_rest || (m.voxels == before_v && !(m.flags & 1)), "an announced insert into a map at rest is refused before anything is added, without a flag"); return r; }
            const int64_t k = chunk * distinct_pct / 100; m.offered += k; m.add(k);
            check(m.list == 0 && m.dropped == 0, "an announced insert never reaches the list");
            a += (int)chunk;
        }
        return OK;
    }
};
static long scripts_ok = 0, scripts_refused = 0, scripts_grown = 0, scripts_redone = 0; static int worst_rounds = 0;
static void run_script(unsigned seed)
{
    g_seed = seed;
    mt19937 rng(seed);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    const bool tiny = pick(0, 1) == 1;          // a device of small numbers, where blocks skip in the normal course of things
    Leg t;
    t.m.d = tiny ? MapDims{4096, 64, 8, 512} : REAL; t.gx = tiny ? 4 : 25;
    t.m.cap_log2 = pick(8, 12); t.m.ovf_cap = t.m.d.small_records;
    const int above = pick(0, 3);
    t.g = gov(t.m.d, above == 0 ? t.m.cap_log2 : above == 1 ? t.m.cap_log2 + pick(1, 4) : pick(20, 24));
    t.small = pick(0, 3) == 0;
    int rate = tiny ? pick(1, 25) : pick(50, 3000);
    const bool inputs_volatile = pick(0, 5) == 0;
    int r = OK;
    for (int step = 0, steps = pick(3, 9); step < steps && r == OK; step++) {
        const int what = pick(0, 9);
        if (what == 0) r = t.insert(pick(1, 40000), pick(10, 100));
        else if (what == 1) { const int n = pick(1, 30000); r = t.settle(n); if (r == OK) { t.m.offered += n; t.m.add(n); check(t.m.list == 0, "an announced merge never reaches the list"); } }          // ssm_map_merge_table
        else if (what == 2) r = t.settle(0);                                                                                                                            // a read of the map
        else {
            if (pick(0, 2) == 0) rate = pick(0, 1) ? min(rate * 10, t.gx * t.m.d.block_records) : max(1, rate / 10);          // the camera leaves a near wall, or returns to it (a block adds a record per pixel at most)
            const int B = pick(0, 3) == 0 ? 250 : pick(1, 16);
            r = t.sequence(pick(1, 3) * B + pick(0, B - 1), B, rate, inputs_volatile);
        }
        check(t.m.skip.size() <= (size_t)t.m.d.skip_cap, "the device skip list never overflows");
    }
    if (r == OK) r = t.settle(0);
    worst_rounds = max(worst_rounds, t.max_rounds);
    check(t.forced == 0, "with the library's call pattern no launch has to settle for its ring slot");
    check(r == OK || r == E_CAPACITY, "a script ends at rest or in the refusal at the cap");
    int64_t outstanding = 0;
    for (auto& ml : t.launches) for (size_t b = 0; b < ml.state.size(); b++) { check(ml.state[b] != 0, "every block ran or skipped"); if (ml.state[b] == 1) outstanding += ml.per_block[b]; }
    check(t.m.voxels + t.m.pending + t.m.dropped + outstanding == t.m.offered, "every contribution is accounted for");
    if (r == OK) {
        scripts_ok++;
        check(t.m.voxels == t.m.offered && t.m.dropped == 0 && outstanding == 0 && !(t.m.flags & 1), "nothing is lost: the table holds what was offered");
        check(t.g.redone == 0 || !t.launches.empty(), "redos only of launches");
    } else {
        scripts_refused++;
        check(t.m.cap_log2 == t.g.vox_max_log2, "refused at the cap only");
        check((t.m.dropped > 0) == ((t.m.flags & 1) != 0), "what was given up is flagged");
    }
    if (t.g.grown) scripts_grown++;
    if (t.g.redone) scripts_redone++;
}

int main()
{
    test_lists_and_begin();
    test_before_launch();
    test_settle_step();
    test_redo_and_ring();
    for (unsigned seed = 1; seed <= 1500; seed++) run_script(seed);
    printf("%ld checks; scripts: %ld at rest, %ld refused at the cap, %ld grew, %ld ran blocks again; most rounds in one settle: %d of %d\n",
           checks, scripts_ok, scripts_refused, scripts_grown, scripts_redone, worst_rounds, MapGov::SETTLE_ROUNDS);
    if (scripts_ok < 300 || scripts_refused < 100 || scripts_grown < 300 || scripts_redone < 100) { printf("FAIL the scripts do not cover what they are for\n"); failures++; }
    if (failures) { printf("%d FAILED\n", failures); return 1; }
    printf("ALL PASSED\n");
    return 0;
}
