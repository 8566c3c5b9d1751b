// test_match_keys.cpp -- the key arithmetic of the matrix-core matcher (csrc/match_keys.h) as a stand-alone program: no library, no device.
// Checked here: the exponent the launchers choose for every row length capT = 32 .. 32768 (2^(e+1) >= capT and the smallest such, every partial sum exact in
// f32, the start / mask value above every key), the switch to the VALU matcher above 32768, and the kernel's running pair in f32 on the host -- the per-tile
// shift, the two-values-per-update rule, the merge of the lane halves and the split at bit e + 1 -- against a sorted list of (distance, trainIdx).
#include "../csrc/match_keys.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <utility>
#include <vector>
using namespace std;

static int failures = 0;
static void check(bool ok, const string& name) { printf("%s %s\n", ok ? "PASS" : "FAIL", name.c_str()); if (!ok) failures++; }

static float med3(float a, float b, float c) { return max(min(a, b), min(max(a, b), c)); }

// one query against nt train descriptors at distances H[j], the way match_mfma_kernel tracks them: row i of tile T sits in lane half (i >> 2) & 1
static pair<uint32_t, uint32_t> kernel_top2(const vector<int>& H, int e)
{
    const int nt = (int)H.size(), ntile = (nt + 31) >> 5;
    float l0[2] = {SSM_MATCH_KEY_BIG, SSM_MATCH_KEY_BIG}, l1[2] = {SSM_MATCH_KEY_BIG, SSM_MATCH_KEY_BIG};
    for (int T = 0; T < ntile; T++)
        for (int h = 0; h < 2; h++) {
            float x[16];
            for (int i = 0; i < 16; i++) {
                const int row = (i & 3) + 8 * (i >> 2) + 4 * h, j = T * 32 + row;
                float acc = (float)(match_key_c0(e) + row);                            // the accumulator's start, then 256 products of +-2^e
                if (j < nt) acc += (float)((2 * H[j] - 256) * (1 << e)); else acc = SSM_MATCH_KEY_BIG;
                x[i] = acc;
            }
            l0[h] -= 32.0f; l1[h] -= 32.0f;
            for (int i = 0; i < 16; i += 2) {
                const float n1 = min(med3(x[i], x[i + 1], l0[h]), l1[h]);
                l0[h] = min(min(x[i], x[i + 1]), l0[h]); l1[h] = n1;
            }
        }
    const float m = max(l0[0], l0[1]);
    const float a0 = min(l0[0], l0[1]), a1 = min(min(m, l1[0]), l1[1]);
    const float back = (float)(32 * (ntile - 1));
    const uint32_t c0 = (uint32_t)(a0 + back), c1 = (uint32_t)(a1 + back), im = (2u << e) - 1u;
    return {((c0 >> (e + 1)) << 16) | (c0 & im), ((c1 >> (e + 1)) << 16) | (c1 & im)};
}
static pair<uint32_t, uint32_t> sorted_top2(const vector<int>& H)
{
    vector<uint32_t> k(H.size());
    for (size_t j = 0; j < H.size(); j++) k[j] = ((uint32_t)H[j] << 16) | (uint32_t)j;
    partial_sort(k.begin(), k.begin() + 2, k.end());
    return {k[0], k[1]};
}

int main()
{
    // the exponent for every row length the launchers can pass
    bool cover = true, smallest = true, exact = true, big = true, issue_form = true;
    for (int capT = 32; capT <= 32768; capT += 32) {
        const int e = match_key_exp(capT);
        cover = cover && e >= 4 && e <= 14 && (2 << e) >= capT && match_key_fits(capT);
        smallest = smallest && (e == 4 || (2 << (e - 1)) < capT);
        exact = exact && match_key_sum_bound(e) < (1 << 24) && match_key_max(e, capT) < (1 << 24) && match_key_max(e, capT) <= match_key_sum_bound(e) + capT;
        big = big && SSM_MATCH_KEY_BIG > (float)match_key_max(e, capT) && SSM_MATCH_KEY_BIG - 32.0f == SSM_MATCH_KEY_BIG && isfinite(SSM_MATCH_KEY_BIG);
        // the bounds in the form the change was asked for (a start of 2^(e+9) would need them; the start is 2^(e+8), see the header): they hold too
        issue_form = issue_form && 768 * (1 << e) + 31 < (1 << 24) && SSM_MATCH_KEY_BIG > (float)((1 << (e + 9)) + capT);
    }
    check(cover, "2^(e+1) >= capT for capT = 32 .. 32768");
    check(smallest, "e is the smallest such exponent");
    check(exact, "every partial sum and key is below 2^24");
    check(big, "the start / mask value is finite, above every key and unchanged by the shift");
    check(issue_form, "768 * 2^e + 31 < 2^24 and the start / mask value exceeds 2^(e+9) + capT");
    check(match_key_exp(1024) == 9 && match_key_exp(1056) == 10 && match_key_exp(1504) == 10 && match_key_exp(2112) == 11 && match_key_exp(4128) == 12 && match_key_exp(32) == 4,
          "e of rows of 32, 1024, 1056, 1504, 2112, 4128 descriptors");
    check(match_key_exp(32768) == 14 && match_key_exp(32800) == -1 && !match_key_fits(33024) && !match_key_fits(65536) && match_key_exp(0) == -1,
          "above 32768 there is no key: the route switches");

    // the running pair in f32 against the sorted list
    mt19937 rng(7);
    bool ok = true;
    int cases = 0;
    auto run = [&](const vector<int>& H) { const int e = match_key_exp(((int)H.size() + 31) & ~31); ok = ok && kernel_top2(H, e) == sorted_top2(H); cases++; };
    for (int nt : {2, 3, 31, 32, 33, 63, 64, 65, 95, 97, 1000, 1024, 1025, 1500, 2100, 4099, 32768})
        for (int hi : {0, 2, 256}) {                                                    // equal distances everywhere, few values, the whole range
            vector<int> H((size_t)nt);
            for (int rep = 0; rep < 3; rep++) { for (auto& v : H) v = hi ? (int)(rng() % (unsigned)(hi + 1)) : 0; run(H); }
        }
    { vector<int> H(1024, 200); H[0] = 0; H[1] = 1; run(H); }                            // shifted 31 times: the pair goes negative
    { vector<int> H(1000, 200); H[998] = 1; H[999] = 0; run(H); }
    { vector<int> H(33, 256); run(H); H[32] = 255; run(H); }                             // the largest key; one valid row in the last tile
    for (int b : {3, 7, 31}) { vector<int> H(70, 100); H[b] = 5; H[b + 1] = 5; run(H); }  // ties across the lane-half, register-group and tile borders
    check(ok, "running pair == sorted (distance, trainIdx) in " + to_string(cases) + " cases");
    printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
