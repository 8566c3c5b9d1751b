// ssm/vocab_train_core.h -- the arithmetic of vocabulary training: a hierarchical k-majority tree over 256-bit ORB descriptors, of the shape
// of DBoW2's TemplatedVocabulary<FORB>::create (k-means with bitwise-majority means, TF-IDF weights) but with a deterministic, integer-only contract of our
// own (DBoW2 seeds from its own random stream, so bit parity with it is no goal).  Shared by
//   * the host function of libssm_hip.so (ssm_vocab_train_host, csrc/ssm_vocab_train_host.cpp),
//   * the device trainer (csrc/kernels_vocab_train.hip),
// so that both build the same tree, byte for byte.
// THE CONTRACT (per node with members S, always taken in ascending input index)
//   * seeding: centre 0 = the first member; centre j = the member with the largest distance to its nearest centre so far, the LOWEST index on ties
//     (seed_key: the maximum of (distance << 32) | ~index); seeding stops when that distance is 0.
//   * assignment: the centre with the smallest Hamming distance, the LOWEST centre on ties (nearest: the rule of ssm_bow::descend).
//   * centre update: bit = 1 iff 2 * ones >= count over the cluster's members (majority_bit: an even split gives 1); an empty cluster keeps its centre.
//   * weight of a word: log((double)F / (double)Ni), Ni = the frames with at least one training descriptor in the word (idf_weight, host only).
#pragma once
#include "looper_core.h"
namespace ssm_vt {
enum { MAX_K = 20, MAX_L = 10, DESC_WORDS = ssm_bow::DESC_WORDS, DESC_BITS = 256 };
static const long long MAX_N = 1ll << 26;
// farthest-point seeding: the largest key wins = the largest distance, then the lowest index
SSM_HD unsigned long long seed_key(int dist, uint32_t index) { return ((unsigned long long)(uint32_t)dist << 32) | (unsigned long long)(uint32_t)~index; }
SSM_HD int seed_key_dist(unsigned long long key) { return (int)(key >> 32); }
SSM_HD uint32_t seed_key_index(unsigned long long key) { return ~(uint32_t)key; }
SSM_HD int majority_bit(int ones, int count) { return 2 * ones >= count ? 1 : 0; }
// the nearest of nc centres (rows of DESC_WORDS words), the lowest on ties; *dist_out = its distance
SSM_HD int nearest(const uint32_t* centres, int nc, const uint32_t* q, int* dist_out)
{
    int best = 0, bd = ssm_bow::hamming(q, centres);
    for (int j = 1; j < nc; j++) { const int d = ssm_bow::hamming(q, centres + (size_t)j * DESC_WORDS); if (d < bd) { bd = d; best = j; } }
    if (dist_out) *dist_out = bd;
    return best;
}
inline double idf_weight(int frames, int frames_with_word) { return log((double)frames / (double)frames_with_word); }
}  // namespace ssm_vt
