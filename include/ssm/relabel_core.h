// relabel_core.h -- the arithmetic of label fusion: the key-frames around a cloud (the VIEWS: depth image, label image, camera, pose) vote on the
// label of each of its points, and a point takes the label its views agree on.  Compiled for host and device like carve_core.h: csrc/kernels_relabel.hip and the
// host function of csrc/ssm_relabel_host.cpp call the same functions, so device == host bit for bit.  Every translation unit that includes this is built with
// -ffp-contract=off.  Whether a view measures the very surface a point lies on is carving's verdict SUPPORTED (carve_core.h verdict_at, s.16 steps 1-7); what is
// here is the vote of one view, the twelve packed counters and the decision.  The reference has no such step.
#pragma once
#include "carve_core.h"

namespace ssm_relabelc {

static const int MAX_VIEWS = 16;
static const int N_LABELS = 12;                 // the palette of render_core.h; a label above 11 is unknown
static const int MAX_OWN_WEIGHT = 15;           // 15 + 16 views = 31: a count fits its 5 bits
static const int MAX_MIN_VOTES = 31;

// one view as both paths read it: the images (device or host memory alike), what carve_core.h needs of camera, size and parameters, and the relative pose
// (carve_core.h rel_pose, evaluated once per call and view on the host)
struct View { const uint16_t* depth; const uint8_t* label; ssm_carvec::Setup S; double M[12]; };

CARVE_HD uint32_t count_of(uint64_t c, uint32_t l) { return (uint32_t)(c >> (5u * l)) & 31u; }
CARVE_HD uint64_t one_of(uint32_t l) { return (uint64_t)1 << (5u * l); }

// step 1: the point's own vote
CARVE_HD uint64_t own_vote(uint32_t L0, int own_weight) { return L0 < (uint32_t)N_LABELS ? (uint64_t)own_weight << (5u * L0) : (uint64_t)0; }

// step 2 for one view: -> the counters after it; *supported, *voted: 1 or 0
CARVE_HD uint64_t view_vote(uint64_t c, float x, float y, float z, const View& V, int edge_guard, int* supported, int* voted)
{
    int px = 0, py = 0;
    *supported = 0; *voted = 0;
    if (ssm_carvec::verdict_at(x, y, z, V.M, V.depth, V.S, &px, &py) != ssm_carvec::SUPPORTED) return c;
    *supported = 1;
    const uint32_t l = V.label[(size_t)py * (size_t)V.S.w + (size_t)px];
    if (l >= (uint32_t)N_LABELS) return c;
    if (edge_guard) {          // (a SUPPORTED point's window lies inside the image: s.16 step 4)
        bool same = true;
        for (int dy = -V.S.r; dy <= V.S.r; dy++) {
            const uint8_t* row = V.label + (size_t)(py + dy) * (size_t)V.S.w + (size_t)(px - V.S.r);
            for (int dx = 0; dx <= 2 * V.S.r; dx++) same = same && row[dx] == l;
        }
        if (!same) return c;
    }
    *voted = 1;
    return c + one_of(l);
}

// steps 3-5: the label after the vote (L0 itself where nothing changes, upper bytes and all)
CARVE_HD uint32_t decide(uint32_t L0, uint64_t c, int min_votes)
{
    uint32_t best = 0, lowest = 0;
    for (uint32_t l = (uint32_t)N_LABELS; l-- > 0;) { const uint32_t k = count_of(c, l); if (k >= best) { best = k; lowest = l; } }      // downwards with >=: the lowest id of the largest count
    if (best == 0) return L0;
    const uint32_t winner = (L0 < (uint32_t)N_LABELS && count_of(c, L0) == best) ? L0 : lowest;
    return (winner != L0 && best >= (uint32_t)min_votes) ? winner : L0;
}

}      // namespace ssm_relabelc
