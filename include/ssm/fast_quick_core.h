// fast_quick_core.h -- the compass quick test of the FAST stage on four horizontally adjacent positions, compiled for host and device like uvd_core.h and
// pnp_core.h: fast_tile (csrc/kernels_orb.hip) and ssm_debug_fast_quick (csrc/ssm_orb_plan.cpp) call the same function (DESIGN.md s.4, row `fast`).
// A position with centre c passes at threshold t when two ADJACENT compass points of its ring (N, E, S, W at distance 3) are both above c + t or both
// below c - t: every 9-arc of the 16-pixel ring contains such a pair, so a position that fails cannot be a corner at t.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define FQ_HD __host__ __device__ inline
#else
#define FQ_HD inline
#endif

namespace ssm_fq {

// ---- the four instructions the test is written in.  Device: the gfx950 instruction; host: a portable stand-in with the same result
// v_alignbyte_b32: bytes n .. n + 3 of the 8-byte value hi:lo
FQ_HD uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, n);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (n & 3)));
#endif
}
// v_perm_b32: result byte i = byte sel[i] of the 8-byte value hi:lo for sel[i] = 0 .. 7, 0x00 for sel[i] = 0x0C (the selectors used here)
FQ_HD uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) { const uint32_t s = (sel >> (8 * i)) & 255u; if (s < 8) r |= (uint32_t)((v >> (8 * s)) & 255u) << (8 * i); }
    return r;
#endif
}
// packed signed 16-bit min / max / add / sub (v_pk_*_i16; wrap-around never happens here: every value stays within -256 .. 511)
#if defined(__HIP_DEVICE_COMPILE__)
typedef short pk16 __attribute__((ext_vector_type(2)));
FQ_HD pk16 as_pk(uint32_t v) { pk16 o; __builtin_memcpy(&o, &v, 4); return o; }
FQ_HD uint32_t as_u32(pk16 v) { uint32_t o; __builtin_memcpy(&o, &v, 4); return o; }
FQ_HD uint32_t pk_min(uint32_t a, uint32_t b) { return as_u32(__builtin_elementwise_min(as_pk(a), as_pk(b))); }
FQ_HD uint32_t pk_max(uint32_t a, uint32_t b) { return as_u32(__builtin_elementwise_max(as_pk(a), as_pk(b))); }
FQ_HD uint32_t pk_add(uint32_t a, uint32_t b) { return as_u32(as_pk(a) + as_pk(b)); }
FQ_HD uint32_t pk_sub(uint32_t a, uint32_t b) { return as_u32(as_pk(a) - as_pk(b)); }
FQ_HD uint32_t mulhi(uint32_t a, uint32_t b) { return __umulhi(a, b); }
#else
#define FQ_PK2(name, expr) \
    FQ_HD uint32_t name(uint32_t a, uint32_t b) \
    { \
        uint32_t r = 0; \
        for (int i = 0; i < 2; i++) { const int x = (int16_t)(a >> (16 * i)), y = (int16_t)(b >> (16 * i)); r |= (uint32_t)(uint16_t)(expr) << (16 * i); } \
        return r; \
    }
FQ_PK2(pk_min, x < y ? x : y)
FQ_PK2(pk_max, x > y ? x : y)
FQ_PK2(pk_add, x + y)
FQ_PK2(pk_sub, x - y)
#undef FQ_PK2
FQ_HD uint32_t mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
#endif

// the threshold as the test takes it: t in both halves
FQ_HD uint32_t pack_threshold(int t) { return (uint32_t)t * 0x00010001u; }
// which of a group's four positions may pass: the first `valid` ones (1 .. 4; the last group of a row may reach past the scored rectangle).
// One sign-byte mask bit per position, as quick4 takes it
FQ_HD uint32_t keep_mask(int valid) { return valid >= 4 ? 0x80808080u : valid <= 0 ? 0u : 0x80808080u >> (8 * (4 - valid)); }

// Four positions x .. x + 3 of one row.  C: their centre pixels (byte j = position j), P / Nx: the dwords left / right of C in the row, U / D: the
// dwords 3 rows up / down; th2 = pack_threshold(t); keep = keep_mask(valid).  Returns the pass bits in bits 0 .. 3 (bit j = position j); bits 4 .. 7
// are zero and bits 8 .. 31 are unspecified: callers keep the low byte.
//   * The ring values are compared RAW: min and max commute with subtracting the centre, so with BR = max over the adjacent pairs of min(x, y)
//     = min(max(S, N), max(E, W)) and DK = min over the pairs of max(x, y) = max(min(S, N), min(E, W)) a position passes iff BR > c + t or
//     DK < c - t, i.e. iff t - max(BR - c, c - DK) is negative: two subtractions of the centre instead of four, and the sign bit is the pass
//     bit as it stands, no negation and no complement.
//   * The four sign bytes are gathered by one perm, masked by `keep`, and one multiplication moves bits 7, 15, 23, 31 to bits 32 .. 35 (the partial
//     products land on distinct bits, so nothing carries; the stray ones are at bit 40 and above).
FQ_HD uint32_t quick4(uint32_t C, uint32_t P, uint32_t Nx, uint32_t U, uint32_t D, uint32_t th2, uint32_t keep)
{
    const uint32_t Lw = alignbyte(C, P, 1);                     // pixels x - 3 of the four positions
    const uint32_t Rw = alignbyte(Nx, C, 3);                    // pixels x + 3
    uint32_t e[2];
    for (int h = 0; h < 2; h++) {
        const uint32_t sel = h ? 0x0C030C02u : 0x0C010C00u;     // bytes (2h, 2h + 1) zero-extended to a pair of 16-bit values
        const uint32_t c = perm(0u, C, sel), s = perm(0u, D, sel), ea = perm(0u, Rw, sel), n = perm(0u, U, sel), w = perm(0u, Lw, sel);
        const uint32_t br = pk_min(pk_max(s, n), pk_max(ea, w)), dk = pk_max(pk_min(s, n), pk_min(ea, w));
        e[h] = pk_sub(th2, pk_max(pk_sub(br, c), pk_sub(c, dk)));            // bits 15 and 31: positions 2h and 2h + 1 pass
    }
    return mulhi(perm(e[1], e[0], 0x07050301u) & keep, 0x02040810u);
}

}  // namespace ssm_fq
