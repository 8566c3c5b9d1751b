// match_keys.h -- the key arithmetic of the matrix-core matcher (kernels_match.hip), shared by the kernel, its launchers and host/test_match_keys.cpp.
// Plain C++ (constexpr, so the kernel may call them): no device code, no library.
//
// With the train block scale 2^e the matrix product of an expanded query / train pair is 2^(e+1) H - 2^(e+8) (H = their Hamming distance), so an accumulator
// started at 2^(e+8) + row holds key = 2^(e+1) H + row when its tile is done, and with 2^(e+1) >= capT the low e + 1 bits have room for a GLOBAL train index.
// Every partial sum is an integer of magnitude <= 2^(e+8) + 256 * 2^e + 31 = 512 * 2^e + 31 whatever the summation order, exact in f32 while that is below 2^24:
// e <= 14, capT <= 32768.
#pragma once

#define SSM_MATCH_KEY_MAX_CAPT 32768    // above it the callers take the VALU matcher
#define SSM_MATCH_KEY_BIG 1e30f         // start value of the running pair and mask of a padded train row: finite (kernels_match.hip is built with -fno-honor-nans),
                                        // above every key at every e, and unchanged by the per-tile shift (1e30f - 32 == 1e30f)

// the train scale's exponent e for rows of capT descriptors (a multiple of 32): the smallest with 2^(e+1) >= capT; -1 when no exact key exists (capT > 32768)
constexpr int match_key_exp(int capT)
{
    if (capT < 1 || capT > SSM_MATCH_KEY_MAX_CAPT) return -1;
    int e = 4;                                                  // one tile: 2^5 rows
    while ((2 << e) < capT) e++;
    return e;
}
constexpr bool match_key_fits(int capT) { return match_key_exp(capT) >= 0; }
// what the accumulator starts at (without the row), the largest key a descriptor can reach (H = 256, the last train index) and the largest partial sum
constexpr int match_key_c0(int e) { return 1 << (e + 8); }
constexpr int match_key_max(int e, int capT) { return (256 << (e + 1)) + capT - 1; }
constexpr int match_key_sum_bound(int e) { return 512 * (1 << e) + 31; }
