// ssm_internal.h -- shared between the translation units of libssm_hip.so (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "../../include/ssm_hip.h"
#include "ssm_orb_plan.h"      // the ORB geometry, the fused pyramid's plan types and the planner: HIP-free
#include "cloud_table.h"       // CloudSeg and the device look-ups of carving, rendering and alignment

#define SSM_VOX_EMPTY ((int64_t)-1)
// Layout of one buffer that several regions share.  take<T>(count) starts a region of count T at the next multiple of `align` and returns its byte offset;
// off is then the bytes used so far (end(): rounded up).  The offsets are computed first, the total goes to whoever provides the buffer, and base + offset
// gives the pointers: the size asked for and the pointers used come from the same statements.
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
struct Carve {
    size_t off = 0; template <class T> size_t take(size_t count, size_t align = 256) { const size_t at = (off + align - 1) & ~(align - 1); off = at + count * sizeof(T); return at; }
    size_t end() { return take<uint8_t>(0); }
};

// candidate: lo = x | y<<12 | score<<24 (x,y relative to minBorder), hi = rank (cell-major raster order)
typedef uint2 cand_t;

// What the launchers size grids and dynamic LDS from, asked once per context (ssm_abi.hip ctx_init); the defaults are the fall-backs when a query fails.
struct DeviceInfo { int id = 0, cus = 256, max_lds = 160 * 1024; };
// Dynamic LDS above the 64 KB default needs the attribute on the current device's copy of the function: set once per (device, function) to `limit`, the largest
// size any launch of it will ask for -- not per launch: the call can serialise against kernels in flight.  The set of pairs already done is process-global on
// purpose: the attribute belongs to the device and the function, not to a context.  bytes <= 48 KB: nothing to do.
hipError_t allow_dynamic_lds(const void* fn, size_t bytes, int limit);

// ---- launchers (each enqueues on `s`; returns hipGetLastError()) ----
hipError_t k_gray(const uint8_t* img, int channels, int n, const OrbGeom& g, uint8_t* pyr, hipStream_t s);
hipError_t k_copy_gray_strided(const uint8_t* img, int stride, const OrbGeom& g, uint8_t* pyr, hipStream_t s);
hipError_t k_pyramid(int n, const OrbGeom& g, uint8_t* pyr, const int32_t* const* xofs, const int16_t* const* xa,
                     const int32_t* const* yofs, const int16_t* const* ya, const void* const* xgroups, hipStream_t s);
hipError_t k_pyramid_bands(const uint8_t* img, int channels, int n, const OrbGeom& g, uint8_t* pyr, const PyrBandPlan& p,
                           const int32_t* const* yofs, const int16_t* const* ya, const void* const* xgroups, const void* const* xgroups8, hipStream_t s);
hipError_t k_blur(int n, const OrbGeom& g, const uint8_t* pyr, uint8_t* blur, hipStream_t s);
// the same blur on the matrix cores; tab = blur_mfma_tables() on the device
hipError_t k_blur_mfma(int n, const OrbGeom& g, const uint8_t* pyr, uint8_t* blur, const void* tab, hipStream_t s);
hipError_t k_fast(int n, const OrbGeom& g, const uint8_t* pyr, cand_t* cand, int32_t* ncand, int32_t* cellmax /* k_fast_cellmax_ints(frames) ints */, hipStream_t s);
size_t k_fast_ncand_pad(int nframes, const OrbGeom& g);         // ints reserved for the per-level candidate counters in front of the cell maxima (one allocation, one fill)
size_t k_fast_cellmax_ints(int nframes, const OrbGeom& g);      // per-cell maxima of nframes frames + the retry work list of k_fast behind them
hipError_t k_octree(int n, const OrbGeom& g, const cand_t* cand, const int32_t* ncand, const int32_t* cellmax, uint16_t* node_of,
                    uint32_t* sel, int32_t* nsel, int32_t* status, hipStream_t s);
int k_octree_nodes(const OrbGeom& g);       // the LDS node capacity (256 / 512 / 1024) of the instance k_octree launches for this geometry
hipError_t k_describe(int n, const OrbGeom& g, const uint8_t* pyr, const uint8_t* blur, const uint32_t* sel,
                      const int32_t* nsel, const float* pattern_f /* the 256 x 4 BRIEF table as floats */, const uint16_t* depth, ssm_camera cam, void* kpaux /* n * sel_total * 32 B */,
                      ssm_keypoint* kps, uint8_t* desc, float* pos3d, int32_t* nkp, hipStream_t s,
                      const void* planted_aux = nullptr /* ssm_debug_orb_describe: n * sel_total (m10, m01, 0.f, 0.f) records that replace orient_kernel's before angle_kernel reads them */);

// matcher.  pair p: query = desc + qoff[p]*32 (nq[p] rows), train = desc + toff[p]*32 (nt[p] rows)
struct MatchPair { int32_t qoff, nq, toff, nt, out_slot; };
hipError_t k_match_pairs(const uint8_t* desc, const MatchPair* pairs, int npairs, double ratio, int cap,
                         ssm_dmatch* out, int32_t* nout, int32_t* knn_idx, int32_t* knn_dist, hipStream_t s);
// as k_match_pairs but pair descriptors derived on the device from nkp[] (sequence mode)
hipError_t k_match_seq(const uint8_t* desc, const int32_t* nkp, int f0, int n, int R, int hist, double ratio, int cap,
                       ssm_dmatch* out, int32_t* nout, int32_t* pend /* n * R ints of scratch */, hipStream_t s);

// the matcher on the matrix cores: descriptors expanded to FP4 rows (capT = cap rounded up to 32 descriptors, SSM_MATCH_DESC_BYTES each, tile-fragment
// order), then v_mfma_scale_f32_32x32x64_f8f6f4 distance tiles -> knn keys -> ratio test + ordered compaction.  Same results as k_match_seq.
// e = match_key_exp(capT) (match_keys.h): the train scale's exponent; rows with no exact key (e < 0, capT > 32768) go to the VALU matcher instead.
#define SSM_MATCH_DESC_BYTES 128
hipError_t k_match_expand(const uint8_t* desc, const int32_t* nkp, int row0, int nrows, int cap, int capT, uint8_t* eq, uint8_t* et, hipStream_t s);
hipError_t k_match_seq_mfma(const uint8_t* eq, const uint8_t* et, const int32_t* nkp, int f0, int n, int R, int hist, double ratio, int cap, int capT,
                            int e, void* knn /* n * R * capT * 8 B */, ssm_dmatch* out, int32_t* nout, hipStream_t s);

// mapper front half
hipError_t k_moving_mask(const uint8_t* sem, int n, int w, int h, uint8_t* mask, hipStream_t s);
hipError_t k_backproject(const uint16_t* depth, const uint8_t* rgb, const uint8_t* sem, const uint8_t* mask,
                         const double* pose, int n, int w, int h, ssm_camera cam, double max_distance,
                         int32_t* chunk_cnt, int64_t* chunk_off, int32_t* npoints, int64_t* total,
                         ssm_point* out, hipStream_t s);
int backproject_chunks(int w, int h);

// voxel table
hipError_t k_voxel_clear(ssm_voxel* tab, int cap_log2, int32_t* counters, hipStream_t s);
hipError_t k_voxel_insert(const ssm_point* pts, const int64_t* n_dev, int64_t n_max, float leaf, ssm_voxel* tab,
                          int cap_log2, int32_t* counters, hipStream_t s);
// the fused map stage (kernels_map.hip map_stream2_kernel): n frames of w x h (w % 16 == 0, w <= 4096).  skip: the context's skip list (k_map_fuse_skip_cap() ints,
// counted in counters[6]); hw: a block that starts with more than hw records in the overflow list logs itself there and adds nothing; tag: the launch's slot in the
// host's ring of launch descriptors.  nredo > 0: run the blocks redo_ids[0 .. nredo) (device; entries as logged) of the launch with these arguments again.
// md, exact: k_map_div of cam, which the caller computes once per camera
struct MapDiv { double rscale, rfx, rfy; };      // the reciprocals of cam.scale, fx, fy (kernels_map.hip markstein_div)
bool k_map_div(const ssm_camera& cam, MapDiv& md);      // false: these divisors need the division itself (a 65,536-step host check)
hipError_t k_map_fuse(const uint16_t* depth, const uint8_t* rgb, const uint8_t* sem, const double* pose, int n, int w, int h,
                      ssm_camera cam, const MapDiv& md, bool exact, double max_distance, float leaf,
                      ssm_voxel* tab, int cap_log2, int32_t* counters, int32_t* npoints, hipStream_t s, int32_t* skip, int hw, int tag, const int32_t* redo_ids, int nredo);
int k_map_fuse_blocks_per_frame(int w, int h);
int k_map_fuse_block_records(void);        // overflow records one block can append at most
int k_map_fuse_resident_blocks(void);      // blocks of the kernel the device can hold at a time
int k_map_fuse_skip_cap(void);
hipError_t k_voxel_merge(const ssm_voxel* src, int n, ssm_voxel* tab, int cap_log2, int32_t* counters, hipStream_t s);
hipError_t k_voxel_rehash(const ssm_voxel* src, int src_cap_log2, ssm_voxel* tab, int cap_log2, int32_t* counters, hipStream_t s);
hipError_t k_voxel_compact(const ssm_voxel* tab, int cap_log2, ssm_voxel* out, int32_t* n_out, hipStream_t s);
hipError_t k_voxel_gather_points(const ssm_voxel* compact, const uint32_t* order, int n, ssm_point* out, hipStream_t s);
hipError_t k_voxel_gather_table(const ssm_voxel* compact, const uint32_t* order, int n, ssm_voxel* out, hipStream_t s);
hipError_t k_voxel_bounds(const ssm_point* pts, int n, float* minmax6, hipStream_t s);
// dst[i] = T src[i] (T: HOST pointer to a column-major 4 x 4, or nullptr = copy); pcl::transformPointCloud's arithmetic
hipError_t k_cloud_transform(const ssm_point* src, int n, const double* T, ssm_point* dst, hipStream_t s);
// sort n (key,index) pairs by key; tmp storage managed by caller via size query (tmp==nullptr)
hipError_t voxel_sort_pairs(void* tmp, size_t* tmp_bytes, const ssm_voxel* compact, int n, uint64_t* keys_a, uint64_t* keys_b,
                            uint32_t* idx_a, uint32_t* idx_b, hipStream_t s);

// synthetic stream
hipError_t k_synth(uint64_t seed, int first, int n, int w, int h, uint8_t* bgr, uint16_t* depth, uint8_t* sem,
                   uint8_t* lab, double* pose, hipStream_t s);

// SegNet (kernels_segnet.hip)
hipError_t k_segnet_prep(const uint8_t* bgr, int n, int sw, int sh, int dw, int dh, const int32_t* xofs, const int16_t* xa,
                         const int32_t* yofs, const int16_t* ya, void* out_f16, hipStream_t s);
// the tile counters of the conv kernels (self-resetting, see conv3x3_dma2_kernel): CONV_QUEUE_INTS zeroed ints per stream, owned by the caller (Lane::conv_tiles)
#define CONV_QUEUE_INTS 1024          // a counter pair per (XCD group, cout tile): 8 x 32 x 2 at most
hipError_t k_segnet_begin(int* tiles, hipStream_t s);
// wt_wino != nullptr: the layer's weights transformed for the Winograd F(2, 3) kernel ([cout tile 64][cin chunk 32][tap = 4 dy + k][c8 4][cout 64][8] fp16): that kernel runs
hipError_t k_segnet_conv(const void* in, const void* wt, const float* scale, const float* shift, void* out, int n, int H, int W,
                         int CinPad, int Cout, int relu, const DeviceInfo& dev, int* tiles, hipStream_t s, const void* wt_wino = nullptr);
// nb frames per launch: left / right [nb][h][w], disp_out [nb][h][w]
size_t k_sgbm_workspace_bytes(int w, int h, const ssm_sgbm_params& p, int nb, int form_cfg);      // sized for the configured formulation (0 = the default), never less than one frame in the largest
bool sgbm_cost_geometry(int D, int SW, int* TX_out, size_t* lds_out);      // false: SADWindowSize too wide for the streaming cost kernel
// fail_flag: device int the sweep kernel ORs 1 into when a strip hand-off times out (never on a healthy device; the host turns it into SSM_E_HIP)
// fan: the lane's side streams for forms 0 / 1 (ssm_ctx.h SgFan), created here when such a form first runs
struct SgFan;
hipError_t k_sgbm(const uint8_t* left, const uint8_t* right, int w, int h, int nb, const ssm_sgbm_params& p, void* workspace, size_t ws_bytes, int16_t* disp_out, int raw_only,
                  const DeviceInfo& dev, SgFan& fan, hipStream_t s, int* fail_flag = nullptr, int form_cfg = 0, int concurrent = 1);
// medianBlur 3 (op bit 0: src -> dst) and / or filterSpeckles (bit 1: in place on dst) on nb stacked w x h maps, launched as k_sgbm's last steps; parent / count nb*w*h ints
hipError_t k_sgbm_post(const int16_t* src, int16_t* dst, int w, int h, int nb, int op, int newVal, int maxSpeckleSize, int maxDiff, int* parent, int* count, hipStream_t s);
hipError_t k_sgbm_depth(const int16_t* disp, int w, int h, int nb, double baseline, double cu, double cv, double f, double roix, double roiy, double roiz, double scale,
                        int* min_scratch /* nb ints */, uint16_t* depth, hipStream_t s);
hipError_t k_vo_estimate(const ssm_pmatch* m, int n, const ssm_vo_params& P, const int32_t* samples, int iters,
                         double* tr_all, int32_t* count, double* tr_out, int32_t* inliers, int32_t* result, hipStream_t s);
hipError_t k_vo_estimate_batch(const ssm_pmatch* m_all, int stride, const int32_t* n_all, int nb, const ssm_vo_params& P, const uint32_t* rand_stream, int iters,
                               int32_t* consumed, int32_t* rand_off, double* tr_all, int32_t* count, double* tr_out, int32_t* inliers, int32_t* result, hipStream_t s);
hipError_t k_segnet_conv_argmax(const void* in, const void* wt, const float* scale, const float* shift, uint8_t* labels, int n, int H, int W,
                                int CinPad, int Cout, const DeviceInfo& dev, int* tiles, hipStream_t s);
hipError_t k_segnet_conv_pool(const void* in, const void* wt, const float* scale, const float* shift, void* out, uint8_t* code, int n, int H, int W,
                              int CinPad, int Cout, const DeviceInfo& dev, int* tiles, hipStream_t s);
int k_segnet_conv_unpool_available();
hipError_t k_segnet_conv_unpool(const void* pooled, const uint8_t* ucode, const void* wt, const float* scale, const float* shift, void* out, int n, int H, int W,
                                int CinPad, int Cout, const DeviceInfo& dev, int* tiles, hipStream_t s);
hipError_t k_segnet_pool(const void* in, int n, int H, int W, int C, void* out, uint8_t* code, hipStream_t s);
hipError_t k_segnet_unpool(const void* in, const uint8_t* code, int n, int PH, int PW, int C, void* out, int H, int W, hipStream_t s);
hipError_t k_segnet_argmax(const void* logits, int n, int npix, int Cstore, int ncls, uint8_t* labels, hipStream_t s);
hipError_t k_segnet_color(const uint8_t* ids, int n, int sw, int sh, int dw, int dh, const int32_t* xofs, const int16_t* xa,
                          const int32_t* yofs, const int16_t* ya, int pavement_to_road, int nearest, uint8_t* sem_bgr, uint8_t* ids_out, hipStream_t s);

// quad matcher (kernels_quad.hip).  Images of the stereo path live in SLOTS: 2 sides x B1 slots, a slot = the 4-level LK pyramid of one image
// (level l at element offset off[l], packed rows) in `pyr` and its Scharr derivatives (x, y int16 pairs) at the same element offsets in `der`.
// Slot 0 = the carried previous frame, slot 1 + f = frame f of the sub-batch.
struct QuadBatch { const uint8_t* pyr; const int16_t* der; size_t slot_elems; int B1; int w[4], h[4], off[4]; };
hipError_t k_quad_pyramids(const QuadBatch& q, int nb, hipStream_t s);
struct GfttWork { float* eig; int* cand_at; uint32_t* cand_bits; /* one bit per pixel: cand_at != 0; k_quad_gftt_bits_words(w, h) words per frame */ unsigned long long *keys, *kept; uint32_t* deps; uint8_t *depn, *state; int *maxord, *count, *nkept; int cap; };
size_t k_quad_gftt_deps_per_candidate();
size_t k_quad_gftt_bits_words(int w, int h);
hipError_t k_quad_gftt(const QuadBatch& q, int nb, int max_corners, double quality, double min_distance, const GfttWork& g, float* pts, int stride, int* ncorner, hipStream_t s);
hipError_t k_quad_lk(const QuadBatch& q, const float* prev_pts, int n, float* next_pts, uint8_t* status, float* err, int max_count, float eps2, float min_eig_thr, hipStream_t s);
hipError_t k_quad_track(const QuadBatch& q, int nb, float* pts, int stride, const int* ncorner, const int* has_prev, void* out, int* nout, hipStream_t s);
hipError_t k_quad_window_match(const float* kp1, const uint8_t* d1, int n1, const float* kp2, const uint8_t* d2, int n2, int sw, int sh, float thr,
                               ssm_dmatch* out, hipStream_t s);

// looper (kernels_bow.hip): words of nframes x cap descriptors (frame f has nkp[f] of them, or n_fixed when nkp is null), the vector of each frame into a staging
// area (cap entries per frame), the append to the CSR database, the score rows of nq query entries and their candidates in (query, entry) order
namespace ssm_bow { struct Tree; }
hipError_t k_bow_words(const ssm_bow::Tree& t, const uint8_t* desc, const int32_t* nkp, int n_fixed, int nframes, int cap, int32_t* words, int variant /* 0: 16 lanes per descriptor, 1: one */, hipStream_t s);
size_t k_bow_frame_lds(int P);
hipError_t k_bow_frame(const int32_t* words, const double* weight, const int32_t* nkp, int n_fixed, int nframes, int cap, int P /* power of two >= cap, <= 4096 */, int32_t* st_ids, double* st_vals, int32_t* st_m, hipStream_t s);
hipError_t k_bow_append(const int32_t* st_ids, const double* st_vals, const int32_t* st_m, int nframes, int cap, int32_t* offsets, int e0, int32_t* db_ids, double* db_vals, long long db_cap, int32_t* hdr, hipStream_t s);
size_t k_bow_score_lds(int qcap);
hipError_t k_bow_score(const int32_t* offsets, const int32_t* db_ids, const double* db_vals, const int32_t* frame_ids, int first, int nq, int against, int row, int qcap,
                       double min_score, int min_interval, double* scores, int32_t* counts, hipStream_t s);
hipError_t k_bow_emit(const int32_t* frame_ids, const double* scores, const int32_t* counts, int first, int nq, int against, int row, double min_score, int min_interval,
                      int32_t* pairs, double* out_scores, int cap, int32_t* hdr /* [1] = the candidate count */, hipStream_t s);

// vocabulary training (kernels_vocab_train.hip; the arithmetic is include/ssm/vocab_train_core.h): ONE LEVEL of the tree under construction.  A POSITION p holds
// the input index perm[p] and the level's node nodeof[p]; a node's members are the positions start[v] .. start[v + 1], in ascending input index.  A CHUNK is
// VT_CHUNK consecutive positions = one block.  Every kernel is one thread per position (or per bit of a chunk); no loop runs longer than k or VT_CHUNK.
#define VT_CHUNK 256
struct VtLevel {
    const uint32_t* desc;          // N x 8, input order
    int N, k, nn;                  // positions, centres per node at most, nodes of this level
    int32_t* perm; int32_t* nodeof; const int32_t* start /* nn + 1 */;
    int32_t* m; int32_t* a;        // per position: distance to the nearest seed so far; cluster
    uint32_t* centres;             // nn x k x 8
    int32_t* ncent;                // nn: centres seeded
    uint32_t* gcnt;                // per straddling node (one that crosses a chunk boundary; slot = the chunk it starts in): k x 257 (ones per bit, then the count); all 0 between passes
    int32_t* changed_at;           // nn: the last pass that changed an assignment of the node
    int32_t* flag;                 // [0]: an assignment changed in this pass
};
// seeding round r (0 .. k - 1): centre r of every node that has not stopped (keys_in: the argmax of round r - 1; null for r = 0) -> m, a, centres, ncent, and the
// argmax for centre r + 1 into keys_out (preset to 0; null for the last round)
hipError_t k_vt_seed(const VtLevel& L, int r, const unsigned long long* keys_in, unsigned long long* keys_out, hipStream_t s);
// centre update: per chunk the ones of every (node, cluster, bit); nodes inside the chunk get their new centres at once, straddling nodes add into gcnt and
// k_vt_finish (strad: their ids, ns of them) makes their centres and zeroes gcnt again
hipError_t k_vt_count(const VtLevel& L, hipStream_t s);
hipError_t k_vt_finish(const VtLevel& L, const int32_t* strad, int ns, hipStream_t s);
hipError_t k_vt_assign(const VtLevel& L, int pass, hipStream_t s);
// stable partition of every node by cluster: hist (chunks x k) = members of cluster j in the chunk; with its exclusive prefix over the chunks (prefix), rank[p] =
// the positions before p that hold cluster a[p] and noderank (nn x k) the same for every cluster at each node's first position; then the move to
// dest[v k + a] + (rank - noderank[v k + a]) with the child node child[v k + a]
hipError_t k_vt_hist(const VtLevel& L, int32_t* hist, hipStream_t s);
hipError_t k_vt_rank(const VtLevel& L, const int32_t* prefix, int32_t* rank, int32_t* noderank, hipStream_t s);
hipError_t k_vt_scatter(const VtLevel& L, const int32_t* rank, const int32_t* noderank, const int32_t* dest, const int32_t* child, int32_t* perm_out, int32_t* nodeof_out, hipStream_t s);
hipError_t k_vt_leaves(const VtLevel& L, const int32_t* leaf_id /* nn */, int32_t* leaf_of_feature /* N, input order */, hipStream_t s);

// UVDisparity (kernels_uvd.hip; the arithmetic is include/ssm/uvd_core.h): n packed frames of w x h.  v_dis: n x h x 256 u8 rows of the V-disparity image,
// maxmin: n x (max, min) of the raw disparities, preset to (INT_MIN, INT_MAX).  K: n FrameK.  u_raw / u_adj / uni: n x 256 x w (u_rows rows of each frame used).
// coords: n x cap (u, v) of the matches, probes: n x cap (roi << 16 | the disparity's 16 bits).  counts: n, preset to 0
namespace ssm_uvdc { struct FrameK; struct Calib; struct Roi; }
hipError_t k_uvd_vdisp(const int16_t* disp, int n, int w, int h, uint8_t* v_dis, int32_t* maxmin, hipStream_t s);
hipError_t k_uvd_classify(const uint8_t* left, const int16_t* disp, int n, int w, int h, const ssm_uvdc::FrameK* K, const ssm_uvdc::Calib& c, const ssm_uvdc::Roi& r,
                          const double* rate, uint8_t* ground, uint8_t* roi, uint8_t* u_raw, uint8_t* u_adj, hipStream_t s);
hipError_t k_uvd_probe(const uint8_t* roi, const int16_t* disp, int n, int w, int h, const int32_t* coords, const int32_t* nmatch, int cap, int32_t* probes, hipStream_t s);
hipError_t k_uvd_segment(const int16_t* disp, const uint8_t* roi, const uint8_t* uni, int n, int w, int h, const ssm_uvdc::FrameK* K, uint8_t* moving, int32_t* counts, hipStream_t s);

// semantic-motion fusion (kernels_motion_fuse.hip; the arithmetic is include/ssm/motion_fuse_core.h): n packed frames of w x h, motion null = all zero.  One launch
// sequence, no wait.  always / cand / filled / mask: n x w x h; labels: n x k_mf_label_stride(w, h) ints (a frame's labels are its first w h); area / overlap:
// n x w x h ints, the figures at each blob's root pixel and 0 elsewhere; info: n x (blobs, large, confirmed, added)
size_t k_mf_label_stride(int w, int h);
int k_mf_tile_w();
int k_mf_tile_h();
hipError_t k_motion_fuse(const uint8_t* sem, const uint8_t* motion, int n, int w, int h, int32_t area_thres, double overlay_thres, uint8_t* always, uint8_t* cand,
                         uint8_t* filled, int32_t* labels, int32_t* area, int32_t* overlap, uint8_t* mask, int32_t* info, hipStream_t s);

// statistical outlier removal (kernels_sor.hip; the arithmetic is include/ssm/sor_core.h).  SorHead: the call's counters in device memory -- the finite points' box as
// ordered ints, their number, the queries a level left unsettled, `bad` (a mean distance off the statistics grid), the queries of the current level, the three sums.
// SorBufs: the workspaces, n entries each (block_cnt / block_off: one per k_sor_block() points, plus one); tmp: k_sor_tmp_bytes(n) for rocPRIM.
// k_sor_begin: head, mean_dist = 0, settled = non-finite.  k_sor_level: one level of the ladder over the n_query points still unsettled (the host knows that number
// from the previous level's read of head->remaining; level 0: nf).  k_sor_stats: the sums.  k_sor_compact: keep[] and the kept points, in input order, to `out`
// (not pts); head->... is not touched: block_off[blocks] is the number kept.  Everything is queued on s, nothing waits.
struct SorHead { int32_t mn[3], mx[3], n_finite, remaining, bad; uint32_t nq; unsigned long long s1, s2_lo, s2_hi; };
struct SorBufs {
    SorHead* head; float* mean_dist; uint8_t *settled, *keep, *flags; uint64_t *keys_a, *keys_b; uint32_t *idx_a, *idx_b, *query, *block_cnt, *block_off; float4* sorted;
    void* tmp; size_t tmp_bytes;
};
int k_sor_block();
size_t k_sor_tmp_bytes(int n);
hipError_t k_sor_begin(const ssm_point* pts, int n, const SorBufs& B, hipStream_t s);
hipError_t k_sor_level(const ssm_point* pts, int n, int nf, const float lo[3], double c, int top, int k, float r2, int n_query, const SorBufs& B, hipStream_t s);
hipError_t k_sor_stats(const ssm_point* pts, int n, const SorBufs& B, hipStream_t s);
hipError_t k_sor_compact(const ssm_point* pts, int n, double threshold, int too_few, const SorBufs& B, ssm_point* out, hipStream_t s);

// free-space carving (kernels_carve.hip; the arithmetic is include/ssm/carve_core.h): one view against m clouds whose points are numbered through, `total` in all
// (2^30 at most).  CarveBufs: seg (m) and blk, the cloud table (cloud_table.h) with blocks of k_carve_block() points, info (m ssm_carve_info, as 8 ints), base
// (m + 1: where a cloud's kept points start in the scratch copy), verdict / run_new / keep / tmp_run (total bytes each), block_cnt / block_off (blocks + 1),
// tmp_pts (total), tmp: k_carve_tmp_bytes(total) for rocPRIM.  k_carve queues everything on s and waits for nothing; afterwards the clouds hold their kept
// points and counters at the front, info[k] is complete, and verdict / run_new are every point's verdict and counter before the compaction.
namespace ssm_carvec { struct Setup; }
struct CarveBufs {
    const CloudSeg* seg; const int32_t* blk; int32_t* info; uint32_t* base; uint8_t *verdict, *run_new, *keep, *tmp_run; uint32_t *block_cnt, *block_off; ssm_point* tmp_pts;
    void* tmp; size_t tmp_bytes;
};
int k_carve_block();
size_t k_carve_tmp_bytes(int total);
hipError_t k_carve(const uint16_t* depth, const ssm_carvec::Setup& S, int min_votes, int m, int total, const CarveBufs& B, hipStream_t s);

// map rendering (kernels_render.hip; the arithmetic is include/ssm/render_core.h): m clouds whose points are numbered through, `total` in all (below 2^32), into a
// w x h z-buffer of 64-bit keys.  seg, blk: the cloud table (cloud_table.h) with blocks of k_render_block() points.  info: 4 ints (ssm_render_info).  k_render
// queues the clear, the splat and the resolve on s and waits for nothing; k_render_compare the comparison (counts: 9 x int64 as ssm_render_compare_info, cleared
// by the call).
namespace ssm_renderc { struct Setup; }
struct RenderImgs { unsigned long long* keys; uint16_t* depth; uint8_t* bgr; uint8_t* label; int32_t* index; };
int k_render_block();
hipError_t k_render(const ssm_renderc::Setup& S, const CloudSeg* seg, const int32_t* blk, int m, int64_t total, const RenderImgs& T, int32_t* info, hipStream_t s);
hipError_t k_render_compare(const uint16_t* rdepth, const uint8_t* rlabel, const uint16_t* depth, const uint8_t* sem, int64_t np, int64_t tol_abs, int64_t ppm,
                            uint8_t* cls, unsigned long long* counts, hipStream_t s);

// ground grid (kernels_grid.hip; the arithmetic is include/ssm/grid_core.h): m clouds whose points are numbered through, `total` in all (below 2^31), into
// S.nx x S.ny cells.  seg, blk: the cloud table (cloud_table.h) with blocks of k_grid_block() points.  info: 10 x int64 as ssm_grid_info.  k_grid queues the
// clear, pass A, the ground kernel, pass B and the resolve on s and waits for nothing.  form: how passes A and B accumulate -- one atomic per point and address
// (GRID_FORM_POINTS, the baseline), or one per run of adjacent lanes with the same destination (GRID_FORM_RUNS); the same bits.
namespace ssm_gridc { struct Setup; }
enum { GRID_FORM_POINTS = 0, GRID_FORM_RUNS = 1, GRID_FORM_DEFAULT = GRID_FORM_RUNS };
struct GridBufs { ssm_grid_cell* cells; uint8_t *cls, *ground_label, *obstacle_label; int32_t *ground_q, *top_q; uint32_t *n, *n_high; };
int k_grid_block();
hipError_t k_grid(const ssm_gridc::Setup& S, const CloudSeg* seg, const int32_t* blk, int64_t total, const GridBufs& T, unsigned long long* info, int form, hipStream_t s);

// object extraction (kernels_objects.hip; the arithmetic is include/ssm/objects_core.h).  Stage 1 on nx x ny cells: k_objects_label queues the tile forests, the rim
// unions, the flatten pass and the scan of the roots; labels[i]: the root of cell i's component (-1: no member), rank[i]: the roots below cell i, rank[nc] their
// number, which the host reads before k_objects_records (comp: that many records), which queues the figures, the keep decision, the scan of the kept (kid[C]: their
// number), the compaction into objs and the paint of object_id.  info: 8 x int64 as ssm_objects_info (k_objects_label sets it).  Stage 2: k_objects_points over the
// cloud table with blocks of k_objects_block() points; form as ssm_debug_objects_form.  Everything is queued on s, nothing waits.
namespace ssm_objc { struct Setup; }
enum { OBJECTS_FORM_POINTS = 0, OBJECTS_FORM_RUNS = 1, OBJECTS_FORM_DEFAULT = OBJECTS_FORM_RUNS };
struct ObjectsCells { const uint8_t *cls, *obstacle_label; const int32_t *ground_q, *top_q; const uint32_t* n_high; int nx, ny; };
struct ObjectsBufs { int32_t *labels, *isroot, *rank, *object_id; uint16_t* loc; void* tmp; size_t tmp_bytes; };
int k_objects_tile_w();
int k_objects_tile_h();
int k_objects_block();
size_t k_objects_tmp_bytes(int64_t nc);
hipError_t k_objects_label(const ObjectsCells& G, const ssm_objc::Setup& S, const ObjectsBufs& B, unsigned long long* info, hipStream_t s);
hipError_t k_objects_records(const ObjectsCells& G, const ssm_objc::Setup& S, const ObjectsBufs& B, int32_t C, ssm_object* comp, int32_t* keep, int32_t* kid, ssm_object* objs,
                             unsigned long long* info, hipStream_t s);
hipError_t k_objects_points(const ssm_gridc::Setup& G, const CloudSeg* seg, const int32_t* blk, int64_t total, const ssm_grid_cell* cells, const int32_t* object_id,
                            ssm_object* objs, int32_t K, int32_t* point_ids, unsigned long long* info, int form, hipStream_t s);

// clearance map (kernels_clearance.hip; the arithmetic is include/ssm/clearance_core.h): k_clearance queues the whole stage on the class image cls of nx x ny cells --
// the column pass (mask: k_clearance_mask_words(nx, ny) words; row: every cell's nearest blocked row of its column), the row pass in the given form (dist2, nearest),
// the seed's snap, the labelling of the traversable cells (labels) and the finish (reach, the counts).  info: 9 x uint64, the eight counts of ssm_clearance_info and
// the seed's key (k_clearance sets them).  Everything is queued on s, nothing waits.
namespace ssm_clrc { struct Setup; }
enum { CLEARANCE_FORM_LDS = 0, CLEARANCE_FORM_SCAN = 1, CLEARANCE_FORM_DEFAULT = CLEARANCE_FORM_LDS };
struct ClearanceBufs { uint32_t* mask; int32_t* row; uint32_t* dist2; int32_t *nearest, *labels; uint8_t* reach; };
int k_clearance_chunk();
size_t k_clearance_mask_words(int nx, int ny);
hipError_t k_clearance(const uint8_t* cls, int nx, int ny, const ssm_clrc::Setup& S, const ClearanceBufs& B, unsigned long long* info, int form, hipStream_t s);

// route field (kernels_route.hip; the arithmetic is include/ssm/route_core.h) on nx x ny cells.  k_route_begin: every cell's byte (in), its dist2 copied (d2), cost
// COST_NONE but 0 at the source (source < 0: none), the tile flags cleared, the active list the *n_first tiles of form 1's first round (the source's and its neighbours), info (9 x uint64: routed, unrouted,
// near_cells, ..., [8] the far key) and ctl (2 x int32, the ring of active counts) zeroed.  k_route_sweeps: form 0, one batch of k_route_batch() sweeps; *changed is
// cleared first and non-zero afterwards when a cost fell.  k_route_round: form 1, the n_active tiles of list relaxed to their fixed points, then the tiles their
// rims woke compacted into list and counted in ctl[round & 1].  k_route_finish: parent, the counts and the far key.  k_route_path: the goal's snap and the walk --
// pinfo: 8 x uint64, the seven counts of ssm_route_path_info and the goal's key; rev: the walk's cells, goal first; path: the same, source first (both max_path
// entries).  Everything is queued on s, nothing waits.
#include "../../include/ssm/route_core.h"
enum { ROUTE_FORM_SWEEPS = 0, ROUTE_FORM_TILES = 1, ROUTE_FORM_DEFAULT = ROUTE_FORM_TILES };
struct RouteBufs { uint8_t* in; uint32_t *d2, *cost; int32_t *parent, *flag, *list; };
int k_route_tile();
int k_route_batch();
int64_t k_route_tiles(int nx, int ny);
hipError_t k_route_begin(const uint8_t* reach, const uint32_t* dist2, int nx, int ny, int32_t source, const ssm_rtc::Setup& S, const RouteBufs& B, unsigned long long* info, int32_t* ctl,
                         int* n_first, hipStream_t s);
hipError_t k_route_sweeps(int nx, int ny, const ssm_rtc::Setup& S, const RouteBufs& B, int32_t* changed, hipStream_t s);
hipError_t k_route_round(int nx, int ny, const ssm_rtc::Setup& S, const RouteBufs& B, int n_active, int round, int32_t* ctl, hipStream_t s);
hipError_t k_route_finish(int nx, int ny, int32_t source, const ssm_rtc::Setup& S, const RouteBufs& B, unsigned long long* info, hipStream_t s);
hipError_t k_route_path(int nx, int ny, const ssm_rtc::Setup& S, const RouteBufs& B, int goal_cx, int goal_cy, int goal_snap, int max_path, int32_t* rev, int32_t* path,
                        unsigned long long* pinfo, hipStream_t s);

// label fusion (kernels_relabel.hip; the arithmetic is include/ssm/relabel_core.h): A.v views vote on the labels of the n points at pts, which change in place
// (the 4 label bytes of a changed point).  votes, new_label: every point's record, n entries; info: 6 x uint64 (n_supported, n_voted, n_changed, n_filled,
// pairs_supported, pairs_voted), cleared by the launcher.  form: RELABEL_FORM_IMAGES reads a view's depth and label images (View::depth, View::label),
// RELABEL_FORM_PACKED one uint32 per pixel, depth | label << 16 (View::depth points at it), 1.4 - 1.5 times faster; RELABEL_FORM_PAIRS the packed image with the windows of two views in flight before either is
// judged: the default, another 10 - 15 % (profiles/r22_relabel.md); the same bits.  k_relabel_labels makes a view's label image from its
// semantic BGR image and, with packed not null, the packed image from that and the depth image.  Both queue on s and wait for nothing.
#include "../../include/ssm/relabel_core.h"
enum { RELABEL_FORM_IMAGES = 0, RELABEL_FORM_PACKED = 1, RELABEL_FORM_PAIRS = 2, RELABEL_FORM_DEFAULT = RELABEL_FORM_PAIRS };
struct RelabelArgs { ssm_relabelc::View view[ssm_relabelc::MAX_VIEWS]; int32_t v, edge_guard, own_weight, min_votes; };
hipError_t k_relabel_labels(const uint8_t* bgr, const uint16_t* depth, int64_t np, uint8_t* label, uint32_t* packed, hipStream_t s);
hipError_t k_relabel(const RelabelArgs& A, int form, ssm_point* pts, int n, uint64_t* votes, uint32_t* new_label, unsigned long long* info, hipStream_t s);

// dense alignment (kernels_align.hip; the arithmetic is include/ssm/align_core.h).  seg, blk: the cloud table (cloud_table.h) of the points USED (every stride-th
// of a cloud), with chunks of k_align_block() points as its blocks.  k_align_normals fills a view's normal map (16 bytes per pixel); k_align_accumulate adds one
// iteration's NSUM 64-bit sums under the increment E (12 doubles, host memory) to sums, which the caller has zeroed.  Both queue on s and wait for nothing.
namespace ssm_alignc { struct Setup; }
int k_align_block();
hipError_t k_align_normals(const uint16_t* depth, const ssm_alignc::Setup& S, void* normals, hipStream_t s);
hipError_t k_align_accumulate(const ssm_alignc::Setup& S, const double* E, const CloudSeg* seg, const int32_t* blk, int64_t total, const uint16_t* depth,
                              const void* normals, unsigned long long* sums, hipStream_t s);

// pose-graph optimiser (kernels_pgo.hip; the arithmetic is include/ssm/pgo_core.h): n views in device memory, one 1024-thread block each.  op 0: optimize(iterations);
// op 1: linearise + assemble; op 2: factor and solve the view's envelope with `lambda`
namespace ssm_pgc { struct View; }
hipError_t k_pgo(const ssm_pgc::View* views, int n, int iterations, int op, double lambda, hipStream_t s);

// for the translation units that only use the public ABI (ssm_track.hip): the configuration a context was created with
void ssm_internal_get_config(const ssm_ctx* c, ssm_config* out);
int ssm_internal_get_device(const ssm_ctx* c);      // the HIP device the context lives on: raw HIP calls of another translation unit select it first
