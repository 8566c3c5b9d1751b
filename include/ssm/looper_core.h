// ssm/looper_core.h -- the arithmetic of rgbd_tutor::Looper (reference include/looper.h, src/looper.cpp) as plain functions on plain arrays: what
// DBoW2::TemplatedVocabulary<FORB>::transform and ::score compute for an L1_NORM / TF_IDF vocabulary (DBoW2 is not in the reference tree; DESIGN.md s.10
// restates it), shared by
//   * the host functions of libssm_hip.so (ssm_vocab_transform_host, ssm_bow_score_host) and the host path of rgbd_tutor::Looper,
//   * the device looper (csrc/kernels_bow.hip),
// so that a bag-of-words vector or a score computed on the host and on the GPU are the same bits (both sides are built -ffp-contract=off).
// THE NUMERIC CONTRACT
//   * word of a descriptor: from the root, among a node's children the one with the smallest 256-bit Hamming distance, the EARLIEST child on ties; until a
//     node has no children.  Integers only.
//   * value of a word in a frame: the word's weight added `count` times to 0.0, one addition per feature that fell into the word (word_value).  All
//     features of a word carry the same weight, so the feature order does not matter.  Words of weight <= 0 do not enter the vector.
//   * L1 norm of a vector: entry i (ascending word id) belongs to lane i mod 64; a lane adds its entries in ascending order, starting from 0.0; the 64 lane
//     sums are added as the xor butterfly of a wavefront (lane l + lane l^1, then ^2, ^4, ^8, ^16, ^32: tree_sum64).  DBoW2 adds the entries one after the
//     other: a rounding-level difference.  Every value is then DIVIDED by the norm (when it is > 0).
//   * score(v, w) = 0.0 - 0.5 * S, S = sum over the entries of w (the SECOND vector: the stored frame) whose word id is also in v of
//     (|v_i - w_i| - |v_i|) - |w_i|; entry j of w belongs to lane j mod 64, a lane adds its common entries in ascending order starting from 0.0 (an entry that is not
//     common adds nothing), the lanes are added by tree_sum64.  An empty vector gives +0.0.
#pragma once
#include <math.h>
#include <stdint.h>
#ifndef SSM_HD
#  if defined(__HIPCC__)
#    define SSM_HD __host__ __device__ inline
#  else
#    define SSM_HD inline
#  endif
#endif
namespace ssm_bow {
enum { LANES = 64, DESC_BYTES = 32, DESC_WORDS = 8 };
// the vocabulary tree, nodes numbered breadth-first (node 0 = the root; the children of a node are consecutive and keep the file's order)
struct Tree {
    const int32_t* first_child;   // per node
    const int32_t* n_child;       // per node; 0 = a word
    const uint32_t* desc;         // per node, DESC_WORDS words (32-byte aligned rows)
    const int32_t* word;          // per node: word id, -1 for inner nodes
    const double* weight;         // per WORD id
    int n_nodes, n_words, max_depth;
};
SSM_HD int popc32(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(x);
#else
    return __builtin_popcount(x);
#endif
}
SSM_HD int hamming(const uint32_t* a, const uint32_t* b) { int d = 0; for (int k = 0; k < DESC_WORDS; k++) d += popc32(a[k] ^ b[k]); return d; }
// the word (leaf NODE index) of one descriptor, one thread walking the tree
SSM_HD int descend(const Tree& t, const uint32_t* q)
{
    int node = 0;
    for (int lvl = 0; lvl < t.max_depth; lvl++) {
        const int nc = t.n_child[node]; if (nc == 0) break;
        const int first = t.first_child[node];
        int best = first, bd = hamming(q, t.desc + (size_t)first * DESC_WORDS);
        for (int c = 1; c < nc; c++) { const int d = hamming(q, t.desc + (size_t)(first + c) * DESC_WORDS); if (d < bd) { bd = d; best = first + c; } }
        node = best;
    }
    return node;
}
SSM_HD double word_value(double weight, int count) { double v = 0.0; for (int k = 0; k < count; k++) v = v + weight; return v; }
SSM_HD double score_term(double v, double w) { return (fabs(v - w) - fabs(v)) - fabs(w); }
SSM_HD double score_from_sum(double s) { return 0.0 - 0.5 * s; }

// ---- host side: the lane tree walked by one thread
inline double tree_sum64(double* lane)          // destroys lane[0 .. 64)
{
    for (int s = 1; s < LANES; s <<= 1) for (int l = 0; l < LANES; l += 2 * s) lane[l] = lane[l] + lane[l + s];
    return lane[0];
}
inline double l1_norm(const double* vals, int m)
{
    double lane[LANES]; for (int l = 0; l < LANES; l++) lane[l] = 0.0;
    for (int i = 0; i < m; i++) lane[i % LANES] = lane[i % LANES] + fabs(vals[i]);
    return tree_sum64(lane);
}
// both vectors in ascending word id
inline double score(const int32_t* ids1, const double* v1, int n1, const int32_t* ids2, const double* v2, int n2)
{
    if (n1 <= 0 || n2 <= 0) return 0.0;
    double lane[LANES]; for (int l = 0; l < LANES; l++) lane[l] = 0.0;
    int i = 0;
    for (int j = 0; j < n2; j++) {
        while (i < n1 && ids1[i] < ids2[j]) i++;
        if (i < n1 && ids1[i] == ids2[j]) lane[j % LANES] = lane[j % LANES] + score_term(v1[i], v2[j]);
    }
    return score_from_sum(tree_sum64(lane));
}
// words: the word id of every feature with a weight > 0, SORTED ascending (nw of them) -> the normalised vector; returns its length (<= nw).  ids / vals hold nw entries
inline int bow_from_sorted_words(const int32_t* words, int nw, const double* weight, int32_t* ids, double* vals)
{
    int m = 0;
    for (int i = 0; i < nw;) { int j = i; while (j < nw && words[j] == words[i]) j++; ids[m] = words[i]; vals[m] = word_value(weight[words[i]], j - i); m++; i = j; }
    const double norm = l1_norm(vals, m);
    if (norm > 0.0) for (int i = 0; i < m; i++) vals[i] = vals[i] / norm;
    return m;
}
}  // namespace ssm_bow
