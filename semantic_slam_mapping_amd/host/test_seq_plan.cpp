// test_seq_plan.cpp -- the schedule of the sequence calls (csrc/ssm_seq_plan.cpp over csrc/ssm_seq_plan.h) as a stand-alone program: it links that one source, so
// it needs neither libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers (make SAN=asan san; make test_seq_plan_san).
//   1. decision tables: the exact plan of hand-written shapes against values written out here from the rules, not computed by a copy of the code;
//   2. the ordering model: the two executors' loops (ssm_seq_process, stereo_seq_run) restated over a model device -- four streams, events with HIP's semantics
//      (a wait takes the event's most recent record at the time the wait is enqueued), happens-before as one knowledge set per stream -- over the whole grid of
//      shapes: every matcher behind every descriptor row it reads, one stream per workspace, work on side lanes only between fork and join, the map's tail;
//   3. a seeded negative: one wait deleted from a three-chain plan, and the model has to say so.
#include "../csrc/ssm_seq_plan.h"
#include <bitset>
#include <cstdio>
#include <string>
#include <vector>
using namespace std;

static int failures = 0; static long checks = 0;
static void check(bool ok, const string& what)
{
    checks++;
    if (ok) return;
    if (failures++ < 40) printf("FAIL %s\n", what.c_str());
}
static const int ORB = SSM_STAGE_ORB, MATCH = SSM_STAGE_MATCH, MAP = SSM_STAGE_MAP, SEGNET = SSM_STAGE_SEGNET, DEF = ORB | MATCH | MAP;
static const SeqLane M = LANE_MAIN, S0 = LANE_SIDE0, S1 = LANE_SIDE1, S2 = LANE_SIDE2, NO = LANE_NONE;
static SeqShape shape(int B, int n, int stages = DEF, bool serialize = false, bool wide16 = true, int map_own_stream = 1) { return {n, B, stages, serialize, wide16, map_own_stream}; }

// ---------------------------------------------------------------- 1. decision tables
struct WantStep { int f0, nb, chain; SeqLane lane, map_lane; bool map_first, record; vector<int> waits; };
struct Want { int nch; bool side_streams, alt_work; vector<SeqLane> forked; SeqLane tail; vector<WantStep> steps; };
static bool same_list(const LaneList& l, const vector<SeqLane>& w) { if (l.n != (int)w.size()) return false; for (int i = 0; i < l.n; i++) if (l.lane[i] != w[i]) return false; return true; }
static void expect(const string& name, const SeqShape& s, const Want& w)
{
    const SeqPlan p = seq_plan(s);
    check(p.nch == w.nch && p.needs_side_streams == w.side_streams && p.needs_alt_work == w.alt_work, name + ": chains, side streams, workspaces");
    check(same_list(p.forked, w.forked), name + ": fork / join list");
    if (s.stages & MAP) check(p.map_tail == w.tail, name + ": map tail");
    check(p.steps.size() == w.steps.size(), name + ": sub-batches");
    for (size_t i = 0; i < p.steps.size() && i < w.steps.size(); i++) {
        const SeqStep& a = p.steps[i]; const WantStep& b = w.steps[i]; const string at = name + ": step " + to_string(i);
        check(a.f0 == b.f0 && a.nb == b.nb && a.chain == b.chain && a.lane == b.lane, at + " frames, chain, lane");
        check(a.map_lane == b.map_lane && a.map_first == b.map_first, at + " map lane, map first");
        bool waits = a.record_orb_done == b.record && a.nwait == (int)b.waits.size();
        for (int k = 0; waits && k < a.nwait; k++) waits = a.wait_chain[k] == b.waits[k];
        check(waits, at + " record, waits");
    }
}
static void test_seq_table()
{
    // three chains: n > 2 B.  Chain 0 main, 1 side 0, 2 side 2, the map on side 1; sub-batch bi waits for chains (bi-1) % 3, (bi-2) % 3
    expect("B4 n14", shape(4, 14), {3, true, true, {S0, S2, S1}, S1, {
        {0, 4, 0, M, S1, false, true, {}}, {4, 4, 1, S0, S1, true, true, {0}}, {8, 4, 2, S2, S1, false, true, {1, 0}}, {12, 2, 0, M, S1, false, true, {2, 1}}}});
    expect("B4 n9", shape(4, 9), {3, true, true, {S0, S2, S1}, S1, {
        {0, 4, 0, M, S1, false, true, {}}, {4, 4, 1, S0, S1, true, true, {0}}, {8, 1, 2, S2, S1, false, true, {1, 0}}}});
    expect("B2 n7", shape(2, 7), {3, true, true, {S0, S2, S1}, S1, {
        {0, 2, 0, M, S1, false, true, {}}, {2, 2, 1, S0, S1, true, true, {0}}, {4, 2, 2, S2, S1, false, true, {1, 0}}, {6, 1, 0, M, S1, false, true, {2, 1}}}});
    // two chains: B < n <= 2 B
    expect("B4 n7", shape(4, 7), {2, true, true, {S0, S1}, S1, {{0, 4, 0, M, S1, false, true, {}}, {4, 3, 1, S0, S1, true, true, {0}}}});
    expect("B4 n8", shape(4, 8), {2, true, true, {S0, S1}, S1, {{0, 4, 0, M, S1, false, true, {}}, {4, 4, 1, S0, S1, true, true, {0}}}});
    // one sub-batch: one chain, the map beside it on side 0
    expect("B4 n3", shape(4, 3), {1, true, false, {S0}, S0, {{0, 3, 0, M, S0, false, false, {}}}});
    expect("B2 n2", shape(2, 2), {1, true, false, {S0}, S0, {{0, 2, 0, M, S0, false, false, {}}}});
    expect("n0", shape(4, 0), {1, true, false, {S0}, S0, {}});
    // SSM_MAP_STREAM=0: the map on the chains' lanes in turn, side 1 unused, the tail on main
    expect("B4 n14 map stream 0", shape(4, 14, DEF, false, true, 0), {3, true, true, {S0, S2}, M, {
        {0, 4, 0, M, M, false, true, {}}, {4, 4, 1, S0, S0, true, true, {0}}, {8, 4, 2, S2, S2, false, true, {1, 0}}, {12, 2, 0, M, M, false, true, {2, 1}}}});
    expect("B4 n7 map stream 0", shape(4, 7, DEF, false, true, 0), {2, true, true, {S0}, M, {{0, 4, 0, M, M, false, true, {}}, {4, 3, 1, S0, S0, true, true, {0}}}});
    expect("B4 n3 map stream 0", shape(4, 3, DEF, false, true, 0), {1, true, false, {S0}, S0, {{0, 3, 0, M, S0, false, false, {}}}});
    // ORB | MATCH: the chains as before, no map stage; side 1 stays in the fork list
    expect("B4 n14 orb match", shape(4, 14, ORB | MATCH), {3, true, true, {S0, S2, S1}, M, {
        {0, 4, 0, M, NO, false, true, {}}, {4, 4, 1, S0, NO, true, true, {0}}, {8, 4, 2, S2, NO, false, true, {1, 0}}, {12, 2, 0, M, NO, false, true, {2, 1}}}});
    expect("B4 n14 orb match map stream 0", shape(4, 14, ORB | MATCH, false, true, 0), {3, true, true, {S0, S2}, M, {
        {0, 4, 0, M, NO, false, true, {}}, {4, 4, 1, S0, NO, true, true, {0}}, {8, 4, 2, S2, NO, false, true, {1, 0}}, {12, 2, 0, M, NO, false, true, {2, 1}}}});
    expect("B4 n3 orb match", shape(4, 3, ORB | MATCH), {1, false, false, {}, M, {{0, 3, 0, M, NO, false, false, {}}}});
    // no ORB stage, the SegNet stage, a width that is no multiple of 16: one chain on main, the map stage of every sub-batch on side 0
    const vector<WantStep> beside = {{0, 4, 0, M, S0, false, false, {}}, {4, 4, 0, M, S0, false, false, {}}, {8, 4, 0, M, S0, false, false, {}}, {12, 2, 0, M, S0, false, false, {}}};
    expect("B4 n14 map only", shape(4, 14, MAP), {1, true, false, {S0}, S0, beside});
    expect("B4 n14 segnet", shape(4, 14, DEF | SEGNET), {1, true, false, {S0}, S0, beside});
    expect("B4 n14 segnet map stream 0", shape(4, 14, DEF | SEGNET, false, true, 0), {1, true, false, {S0}, S0, beside});
    expect("B4 n14 odd width", shape(4, 14, DEF, false, false), {1, true, false, {S0}, S0, beside});
    // profiling mode 2: everything on main, nothing forked
    expect("B4 n14 serialize", shape(4, 14, DEF, true), {1, false, false, {}, M, {
        {0, 4, 0, M, M, false, false, {}}, {4, 4, 0, M, M, false, false, {}}, {8, 4, 0, M, M, false, false, {}}, {12, 2, 0, M, M, false, false, {}}}});
    expect("B4 n7 serialize segnet", shape(4, 7, DEF | SEGNET, true), {1, false, false, {}, M, {{0, 4, 0, M, M, false, false, {}}, {4, 3, 0, M, M, false, false, {}}}});
}
static void expect_stereo(const string& name, const StereoPlan& p, bool two, int nsg, const vector<SeqLane>& forked, const vector<SeqLane>& lanes)
{
    check(p.two == two && p.nsg == nsg && same_list(p.forked, forked), name + ": two, lanes in use, fork / join list");
    for (size_t k = 0; k < lanes.size(); k++) check(p.lane((int)k) == lanes[k] && p.work((int)k) == (int)k % nsg, name + ": SGBM lane and workspace of sub-batch " + to_string(k));
}
static void test_stereo_table()
{
    const int Q = SSM_STEREO_QUAD, D = SSM_STEREO_DEPTH, V = SSM_STEREO_VO;
    expect_stereo("n10 B4 two streams", stereo_plan(10, 4, Q | D | V, false, 2), true, 2, {S0, S1}, {S0, S1, S0});
    expect_stereo("n10 B4 three streams", stereo_plan(10, 4, Q | D, false, 3), true, 3, {S0, S1, S2}, {S0, S1, S2});
    expect_stereo("n8 B4 three streams", stereo_plan(8, 4, Q | D, false, 3), true, 2, {S0, S1}, {S0, S1});
    expect_stereo("n10 B4 one stream", stereo_plan(10, 4, Q | D, false, 1), true, 1, {S0}, {S0, S0, S0});
    expect_stereo("n3 B4", stereo_plan(3, 4, Q | D | V, false, 2), true, 1, {S0}, {S0});
    expect_stereo("n0", stereo_plan(0, 4, Q | D | V, false, 2), true, 0, {S0}, {});
    expect_stereo("depth only", stereo_plan(10, 4, D, false, 2), false, 1, {}, {M, M, M});
    expect_stereo("quad only", stereo_plan(10, 4, Q | V, false, 2), false, 1, {}, {M, M, M});
    expect_stereo("serialize", stereo_plan(10, 4, Q | D | V, true, 3), false, 1, {}, {M, M, M});
}

// ---------------------------------------------------------------- 2. the ordering model
typedef bitset<512> Set;
enum OpKind { OP_HIST, OP_ORB /* ORB + expand */, OP_MATCH, OP_SEGNET, OP_MAP, OP_QUAD, OP_SGBM };
struct Op { OpKind kind; int lane, sub, work; Set before; };          // before: the operations this one is ordered behind
struct Event { bool recorded = false; Set snap; };
struct Device {
    Set know[4];                       // per stream: what the next operation enqueued there is ordered behind
    vector<Op> ops; Event forked, joined[4], orb_done[3];
    bool was_forked[4] = {}, was_joined[4] = {}; int violations = 0; string first;
    void fail(const string& what) { if (!violations++) first = what; }
    int launch(OpKind kind, int lane, int sub, int work = 0)
    {
        if (lane != LANE_MAIN && (!was_forked[lane] || was_joined[lane])) fail("work on a side lane outside fork .. join");
        const int id = (int)ops.size();
        if (id >= (int)Set().size()) { fail("the model's sets are too small"); return 0; }
        ops.push_back({kind, lane, sub, work, know[lane]}); know[lane].set(id);
        return id;
    }
    void record(Event& e, int lane) { e.recorded = true; e.snap = know[lane]; }
    void wait(int lane, const Event& e) { if (!e.recorded) { fail("a wait for an event with no record in this call"); return; } know[lane] |= e.snap; }
    void fork(const LaneList& l)
    {
        if (!l.n) return;
        record(forked, LANE_MAIN);
        for (int i = 0; i < l.n; i++) { wait(l.lane[i], forked); was_forked[l.lane[i]] = true; }
    }
    void join(const LaneList& l) { for (int i = 0; i < l.n; i++) { record(joined[l.lane[i]], l.lane[i]); wait(LANE_MAIN, joined[l.lane[i]]); was_joined[l.lane[i]] = true; } }
    // after the join: what was forked is joined, every operation is behind the main stream, every workspace of a kind was used on one stream
    void check_end(bool side_streams)
    {
        for (int l = 1; l < 4; l++) { if (was_forked[l] != was_joined[l]) fail("a forked lane is not joined"); if (was_forked[l] && !side_streams) fail("a side lane without needs_side_streams"); }
        for (size_t i = 0; i < ops.size(); i++) {
            if (!know[LANE_MAIN].test(i)) fail("an operation the main stream is not ordered behind after the join");
            const bool has_work = ops[i].kind == OP_ORB || ops[i].kind == OP_SEGNET || ops[i].kind == OP_SGBM;          // a chain's, SegNet's one, SGBM's k-th
            for (size_t j = 0; has_work && j < i; j++) if (ops[i].kind == ops[j].kind && ops[i].work == ops[j].work && ops[i].lane != ops[j].lane) fail("one workspace on two streams");
        }
    }
};
// ssm_seq_process from seq_plan on: fork, the steps (seq_front, seq_back in the order map_first says), join
static void seq_front(Device& d, int stages, const SeqStep& st, int bi)
{
    if (stages & ORB) {
        d.launch(OP_ORB, st.lane, bi, st.chain);
        if (st.record_orb_done) { d.record(d.orb_done[st.chain], st.lane); for (int k = 0; k < st.nwait; k++) d.wait(st.lane, d.orb_done[st.wait_chain[k]]); }
    }
    if (stages & MATCH) d.launch(OP_MATCH, st.lane, bi);
}
static void seq_back(Device& d, int stages, const SeqStep& st, int bi)
{
    if (st.map_lane == LANE_NONE) return;
    if (stages & SEGNET) d.launch(OP_SEGNET, st.map_lane, bi);
    if (stages & MAP) d.launch(OP_MAP, st.map_lane, bi);
}
// -> the violations of the plan p for a call of `stages` with R reference frames (0: none), the first of them in *first
static int seq_violations(const SeqPlan& p, int stages, int R, string* first = nullptr)
{
    Device d;
    d.launch(OP_HIST, LANE_MAIN, -1);
    d.fork(p.forked);
    for (size_t bi = 0; bi < p.steps.size(); bi++) {
        const SeqStep& st = p.steps[bi];
        if (st.map_first) { seq_back(d, stages, st, (int)bi); seq_front(d, stages, st, (int)bi); }
        else              { seq_front(d, stages, st, (int)bi); seq_back(d, stages, st, (int)bi); }
        if (st.chain > 0 && !p.needs_alt_work) d.fail("chain 1 or 2 without needs_alt_work");
    }
    d.join(p.forked);
    d.check_end(p.needs_side_streams);
    // the matcher of a sub-batch is behind the history rows and behind ORB + expand of every sub-batch that holds one of the frames [f0 - R, f0 + nb)
    for (const Op& m : d.ops) {
        if (m.kind != OP_MATCH) continue;
        const SeqStep& st = p.steps[m.sub];
        if (!m.before.test(0)) d.fail("a matcher not behind the history rows");
        for (size_t i = 0; i < d.ops.size(); i++) {
            if (d.ops[i].kind != OP_ORB) continue;
            const SeqStep& o = p.steps[d.ops[i].sub];
            if (o.f0 < st.f0 + st.nb && o.f0 + o.nb > st.f0 - R && !m.before.test(i))
                d.fail("the matcher of sub-batch " + to_string(m.sub) + " is not behind ORB of sub-batch " + to_string(d.ops[i].sub));
        }
    }
    // the map's tail is behind every map launch
    for (size_t i = 0; i < d.ops.size(); i++) if (d.ops[i].kind == OP_MAP && !d.know[p.map_tail].test(i)) d.fail("a map launch the map's tail is not behind");
    if (first) *first = d.first;
    return d.violations;
}
static int stereo_violations(const StereoPlan& p, int n, int B, int stages, string* first)
{
    Device d;
    d.fork(p.forked);
    for (int f0 = 0; f0 < n; f0 += B) {
        if (stages & SSM_STEREO_QUAD) d.launch(OP_QUAD, LANE_MAIN, f0 / B);
        if (stages & SSM_STEREO_DEPTH) {
            if (p.work(f0 / B) < 0 || p.work(f0 / B) >= 3) d.fail("no such SGBM workspace");
            d.launch(OP_SGBM, p.lane(f0 / B), f0 / B, p.work(f0 / B));
        }
    }
    d.join(p.forked);
    d.check_end(p.two);
    *first = d.first;
    return d.violations;
}
static void test_model_grid()
{
    const int masks[4] = {DEF, ORB | MATCH, MAP, DEF | SEGNET};
    long shapes = 0;
    for (int n = 1; n <= 40; n++) for (int B = 1; B <= 8; B++) for (int stages : masks) for (int own = 0; own < 2; own++) for (int mode = 0; mode < 3; mode++) {
        const SeqPlan p = seq_plan(shape(B, n, stages, mode == 1, mode != 2, own));          // mode 1: serialised, 2: a width that is no multiple of 16
        for (int R = 1; R <= 12; R++, shapes++) {
            string first;
            const int v = seq_violations(p, stages, R, &first);
            check(v == 0, "model: n " + to_string(n) + " B " + to_string(B) + " R " + to_string(R) + " stages " + to_string(stages) + " map stream " + to_string(own) +
                          " mode " + to_string(mode) + ": " + first);
        }
    }
    for (int n = 0; n <= 40; n++) for (int B = 1; B <= 8; B++) for (int stages = 1; stages < 8; stages++) for (int streams = 1; streams <= 3; streams++) for (int ser = 0; ser < 2; ser++, shapes++) {
        string first;
        const int v = stereo_violations(stereo_plan(n, B, stages, ser != 0, streams), n, B, stages, &first);
        check(v == 0, "stereo model: n " + to_string(n) + " B " + to_string(B) + " stages " + to_string(stages) + " streams " + to_string(streams) + " serialize " + to_string(ser) + ": " + first);
    }
    printf("model: %ld shapes\n", shapes);
}

// ---------------------------------------------------------------- 3. a seeded negative
static void test_negative()
{
    // B = 2 < R = 5, three chains: sub-batch 2 (frames 4, 5) reads rows of sub-batches 0 and 1.  Chain 1 recorded its event BEFORE it waited for chain 0, so
    // without its own wait for chain 0 the matcher of sub-batch 2 is not behind ORB of sub-batch 0
    SeqPlan p = seq_plan(shape(2, 7));
    string first;
    check(seq_violations(p, DEF, 5, &first) == 0, "negative: the plan as it is: " + first);
    check(p.steps.size() == 4 && p.steps[2].nwait == 2 && p.steps[2].wait_chain[1] == 0, "negative: sub-batch 2 waits for chains 1, 0");
    p.steps[2].nwait = 1;
    check(seq_violations(p, DEF, 5, &first) > 0 && first == "the matcher of sub-batch 2 is not behind ORB of sub-batch 0", "negative: the deleted wait is reported (" + first + ")");
    check(seq_violations(p, DEF, 2, &first) == 0, "negative: with R = B = 2 that wait orders nothing the matcher reads: " + first);
}

int main()
{
    test_seq_table();
    test_stereo_table();
    test_model_grid();
    test_negative();
    printf("%ld checks, %d failures\n", checks, failures);
    puts(failures ? "FAILED" : "ALL PASSED");
    return failures ? 1 : 0;
}
