// test_orb_plan.cpp -- the ORB planner (csrc/ssm_orb_plan.cpp over csrc/ssm_orb_plan.h) as a stand-alone program: it links that one source, so it needs neither
// libssm_hip.so nor a GPU and runs as it is under the CPU sanitizers (make SAN=asan san).  The planner's index arithmetic decides what every ORB kernel may read
// and write; here it runs over the configurations of tests/test_pyramid_items.py and tests/test_fast_tiling.py -- orb_plan_build, then ssm_debug_fast_plan and
// ssm_debug_pyramid_plan (size query, then the full call) -- with the sizes of every table checked against the level it belongs to.
#include "../csrc/ssm_orb_plan.h"
#include <cstdio>
#include <cstring>
using namespace std;

static int failures = 0, accepted = 0, refused = 0, fused = 0, unfused = 0;
static const ssm_config* g_cfg = nullptr;
static void check(bool ok, const char* what)
{
    if (ok) return;
    printf("FAIL %s (%d x %d, %d levels, scale %g, thresholds %d / %d)\n", what, g_cfg->width, g_cfg->height, g_cfg->orb_levels, (double)g_cfg->orb_scale, g_cfg->orb_iniThFAST, g_cfg->orb_minThFAST);
    failures++;
}
static ssm_config config(int w, int h, int levels, float scale)
{
    ssm_config c; memset(&c, 0, sizeof(c));
    c.width = w; c.height = h; c.orb_levels = levels; c.orb_scale = scale; c.orb_features = 600; c.orb_iniThFAST = 20; c.orb_minThFAST = 7;
    return c;
}
static const int BANDS[8] = {-1, 0, 1, 7, 8, 32, 40, 64};

static void run(const ssm_config& cfg)
{
    g_cfg = &cfg;
    OrbPlan P; string err;
    // something in every field, so that a refusal has to clear it
    P.g.nlevels = 3; P.xofs[1].assign(5, 1); P.blur_tab.assign(7, 1); P.bands[0].bands = 8; P.band_tab[0].assign(4, 1); P.streaming[1] = true;
    const int r = orb_plan_build(cfg, P, err);
    if (r != SSM_OK) {
        refused++;
        bool empty = P.g.nlevels == 0 && P.blur_tab.empty() && !P.bands[0].bands && !P.bands[1].bands && P.band_tab[0].empty() && P.band_tab[1].empty();
        for (int l = 0; l < SSM_MAX_LEVELS; l++)
            empty = empty && P.xofs[l].empty() && P.yofs[l].empty() && P.xa[l].empty() && P.ya[l].empty() && P.xgrp[l].empty() && P.xgrp8[l].empty() && !P.streaming[l] && !P.wide_ok[l];
        check(r == SSM_E_INVAL && !err.empty(), "a refusal is SSM_E_INVAL with a message");
        check(empty, "a refusal leaves an empty plan");
        int n = -1;
        check(ssm_debug_fast_plan(&cfg, nullptr, 0, &n, nullptr) == r, "ssm_debug_fast_plan refuses it too");
        for (int b : BANDS) check(ssm_debug_pyramid_plan(&cfg, b, nullptr, 0, &n, nullptr, nullptr) == r, "ssm_debug_pyramid_plan refuses it too");
        return;
    }
    accepted++;
    const OrbGeom& g = P.g; const int L = g.nlevels;
    check(L == cfg.orb_levels && g.W == cfg.width && g.H == cfg.height && err.empty(), "geometry of the configuration");
    check(P.xofs[0].empty() && P.yofs[0].empty() && P.xgrp[0].empty() && P.xgrp8[0].empty() && !P.streaming[0] && !P.wide_ok[0], "level 0 has no tables");
    for (int l = 1; l < L; l++) {
        const LevelGeom& G = g.L[l];
        check(P.xofs[l].size() == (size_t)G.w && P.xa[l].size() == 2 * (size_t)G.w, "x tables: w entries");
        check(P.yofs[l].size() == (size_t)((G.h + 3) & ~3) && P.ya[l].size() == 2 * P.yofs[l].size(), "y tables: h rounded up to 4 entries");
        check(P.xgrp[l].size() == (size_t)(G.stride / 4) * 8, "4-pixel groups: stride / 4 x 8 words");
        check(P.xgrp8[l].size() == (size_t)(G.stride / 8) * 12, "8-pixel groups: stride / 8 x 12 words");
        check(!P.wide_ok[l] || P.streaming[l], "wide_ok implies streaming");
        for (int x = 0; x < G.w; x++) check(P.xofs[l][x] >= 0 && P.xofs[l][x] < g.L[l-1].w, "x offsets inside the source row");
        for (size_t y = 0; y < P.yofs[l].size(); y++) check(P.yofs[l][y] >= 0 && P.yofs[l][y] < g.L[l-1].h, "y offsets inside the source level");
    }
    check(P.blur_tab.size() == blur_mfma_table_bytes(g), "blur table bytes");
    for (int k = 0; k < 2; k++) {
        if (P.bands[k].bands) check(P.bands[k].lds <= PB_MAX_LDS && P.band_tab[k].size() == (size_t)P.bands[k].bands * L * 4 && !P.bands[k].d_tab, "chosen band plan: LDS and table size");
        else check(P.band_tab[k].empty(), "no band plan: no band table");
    }
    // the FAST plan: size query, full call, one entry too few
    {
        int n = -1, n2 = -1; int32_t limits[6];
        check(ssm_debug_fast_plan(&cfg, nullptr, 0, &n, limits) == SSM_OK && n == g.ftiles_total && n > 0 && limits[0] == FT_LDS_BYTES, "ssm_debug_fast_plan: size query");
        vector<int32_t> tiles((size_t)16 * n, -1);
        check(ssm_debug_fast_plan(&cfg, tiles.data(), n, &n2, nullptr) == SSM_OK && n2 == n, "ssm_debug_fast_plan: full call");
        bool ok = true;
        for (int t = 0; t < n; t++) {
            const int32_t* v = &tiles[16 * (size_t)t];
            ok = ok && v[0] >= 0 && v[0] < L && v[13] == g.L[v[0]].w && v[14] == g.L[v[0]].h && v[5] <= v[1] && v[1] < v[2] && v[2] <= v[6] && v[7] <= v[3] && v[3] < v[4] && v[4] <= v[8]
                    && v[11] >= 1 && v[11] <= 8 && v[12] >= 1 && v[12] <= 8;
        }
        check(ok, "ssm_debug_fast_plan: every tile's interior inside its scored rectangle, at most 8 x 8 cells");
        check(ssm_debug_fast_plan(&cfg, tiles.data(), n - 1, &n2, nullptr) == SSM_E_INVAL, "ssm_debug_fast_plan: too small a buffer");
    }
    // the pyramid plan at every band argument
    for (int b : BANDS) {
        int n = -1, n2 = -1; int32_t limits[16 + 3 * SSM_MAX_LEVELS];
        check(ssm_debug_pyramid_plan(&cfg, b, nullptr, 0, &n, nullptr, limits) == SSM_OK && n >= 0 && limits[6] == L, "ssm_debug_pyramid_plan: size query");
        if (!limits[0]) { unfused++; check(n == 0, "no fused plan: no items"); continue; }
        fused++;
        const int nb = limits[0];
        check((b > 0 ? nb == b : nb == P.bands[b == 0 ? 0 : 1].bands) && limits[1] <= PB_MAX_LDS && limits[2] > 0 && limits[2] <= limits[1], "fused plan: band count and LDS");
        vector<int32_t> items((size_t)12 * n, -1), tab((size_t)nb * L * 4, -1);
        check(ssm_debug_pyramid_plan(&cfg, b, items.data(), n, &n2, tab.data(), nullptr) == SSM_OK && n2 == n, "ssm_debug_pyramid_plan: full call");
        if (b <= 0) check(tab == P.band_tab[b == 0 ? 0 : 1], "the chosen plan's band table");
        bool ok = true;
        for (int i = 0; i < n; i++) ok = ok && items[12 * (size_t)i] >= 1 && items[12 * (size_t)i] < L && items[12 * (size_t)i + 1] >= 0 && items[12 * (size_t)i + 1] < nb;
        check(ok, "ssm_debug_pyramid_plan: every item names a level and a band of the plan");
        if (n > 0) check(ssm_debug_pyramid_plan(&cfg, b, items.data(), n - 1, &n2, nullptr, nullptr) == SSM_E_INVAL, "ssm_debug_pyramid_plan: too small a buffer");
    }
}

int main()
{
    static const int sizes[5][2] = {{640, 480}, {1241, 376}, {644, 484}, {642, 482}, {176, 88}};
    static const float scales[5] = {1.1f, 1.2f, 1.25f, 1.3f, 1.5f};
    for (auto& s : sizes) for (float sc : scales) for (int levels = 1; levels <= 8; levels++) run(config(s[0], s[1], levels, sc));
    // the thresholds and sizes build_geometry refuses
    const int before = refused;
    { ssm_config c = config(640, 480, 8, 1.2f); c.orb_iniThFAST = 0; run(c); }
    { ssm_config c = config(640, 480, 8, 1.2f); c.orb_iniThFAST = 255; run(c); }
    { ssm_config c = config(640, 480, 8, 1.2f); c.orb_minThFAST = 0; run(c); }
    { ssm_config c = config(640, 480, 8, 1.2f); c.orb_minThFAST = 255; run(c); }
    run(config(63, 480, 1, 1.2f));
    run(config(640, 4001, 1, 1.2f));
    { const ssm_config c = config(640, 480, 8, 1.2f); g_cfg = &c; check(refused == before + 6, "the six bad thresholds / sizes are refused"); }
    // the FAST quick test (ssm_debug_fast_quick) on seeded random groups against the definition: two adjacent compass points above c + t or below c - t
    {
        const ssm_config c = config(640, 480, 8, 1.2f); g_cfg = &c;
        const int N = 20000; vector<uint32_t> words((size_t)5 * N); vector<uint8_t> out(N);
        uint32_t seed = 12345u;
        for (uint32_t& w : words) { seed = seed * 1664525u + 1013904223u; w = seed ^ (seed >> 13); }
        for (size_t i = 0; i < words.size(); i += 3) words[i] = (words[i] & 0x1F1F1F1Fu) + 0x70707070u;      // some near-flat words: values within a threshold or two
        bool ok = true;
        for (int t : {c.orb_minThFAST, c.orb_iniThFAST}) for (int valid = 1; valid <= 4; valid++) {
            check(ssm_debug_fast_quick(words.data(), N, t, valid, out.data()) == SSM_OK, "ssm_debug_fast_quick");
            for (int i = 0; i < N; i++) {
                const uint32_t* w = &words[5 * (size_t)i];
                uint8_t row[12]; memcpy(row, &w[1], 4); memcpy(row + 4, &w[0], 4); memcpy(row + 8, &w[2], 4);      // pixels x - 4 .. x + 7
                int want = 0;
                for (int j = 0; j < valid; j++) {
                    const int ce = row[4 + j], p[4] = {(int)((w[3] >> (8 * j)) & 255), row[4 + j + 3], (int)((w[4] >> (8 * j)) & 255), row[4 + j - 3]};
                    bool pass = false;
                    for (int k = 0; k < 4; k++) pass = pass || (p[k] > ce + t && p[(k + 1) & 3] > ce + t) || (p[k] < ce - t && p[(k + 1) & 3] < ce - t);
                    want |= (pass ? 1 : 0) << j;
                }
                ok = ok && out[i] == want;
            }
        }
        check(ok, "ssm_debug_fast_quick equals the definition");
        check(ssm_debug_fast_quick(words.data(), 1, 7, 5, out.data()) == SSM_E_INVAL && ssm_debug_fast_quick(nullptr, 1, 7, 4, out.data()) == SSM_E_INVAL, "ssm_debug_fast_quick refuses bad arguments");
    }
    printf("orb plan: %d configurations accepted, %d refused; %d fused pyramid plans, %d band arguments without one\n", accepted, refused, fused, unfused);
    if (!accepted || !refused || !fused || !unfused) { printf("FAIL the sweep must see accepted and refused configurations, fused plans and geometries without one\n"); failures++; }
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
