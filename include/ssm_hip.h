/* ssm_hip.h -- C ABI of libssm_hip.so, the MI355X (gfx950) implementation of the per-frame semantic-mapping
 * front end of MuMuJun97/semantic_slam_mapping.  Plain pointers and sizes only; no C++/torch types.
 *
 * The reference has no FFI: its hot path sits behind plain C++ classes linked into librgbd_tutor_lib.so
 * (/root/reference/src/CMakeLists.txt:1-5).  Each entry point below names the reference interface it replaces;
 * the C++ classes of the same names (include/ssm/ *.h in this repo) are thin callers of these functions, and
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions: every function returns SSM_OK (0) or a negative ssm_status; nothing throws across the ABI; the caller
 * owns every host buffer and passes capacities; the context owns device memory and one HIP stream; calls on one
 * context are serialised by an internal mutex (the reference calls detectFeatures on the main thread and
 * generatePointCloud on the viewer thread, SURVEY.md s.8b "threading": give each thread its own context or share one).
 * Host-pointer functions are synchronous.  *_dev functions take DEVICE pointers, enqueue on the context stream and
 * return without waiting (ssm_sync waits).
 */
#ifndef SSM_HIP_H
#define SSM_HIP_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    SSM_OK = 0,
    SSM_E_INVAL = -1,        /* bad argument / unsupported configuration */
    SSM_E_NOMEM = -2,        /* device or host allocation failed */
    SSM_E_HIP = -3,          /* HIP runtime error (ssm_last_error has the text) */
    SSM_E_CAPACITY = -4,     /* caller buffer or internal table too small */
    SSM_E_TOO_FEW_TRAIN = -5,/* matcher needs >= 2 train descriptors (src/orb.cpp:25 indexes [1] unguarded) */
    SSM_E_VOXEL_RANGE = -6,  /* PCL VoxelGrid index-overflow guard would trip: output == input in the reference */
    SSM_E_NODEVICE = -7,
    SSM_E_COMM = -8          /* RCCL error (ssm_last_error has ncclGetErrorString) */
} ssm_status;

/* layout-identical to cv::KeyPoint (OpenCV 2.4), 28 bytes */
typedef struct { float x, y, size, angle, response; int32_t octave, class_id; } ssm_keypoint;
/* layout-identical to cv::DMatch, 16 bytes */
typedef struct { int32_t queryIdx, trainIdx, imgIdx; float distance; } ssm_dmatch;
/* layout-identical to pcl::PointXYZRGBL (a superset of Mapper::PointT = pcl::PointXYZRGBA, include/mapper.h:18), 32 bytes */
typedef struct { float x, y, z, w; uint8_t b, g, r, a; uint32_t label; uint32_t pad[2]; } ssm_point;
/* rgbd_tutor::CAMERA_INTRINSIC_PARAMETERS (include/utils.h:8-16) */
typedef struct { double cx, cy, fx, fy, scale; } ssm_camera;
/* one voxel of the map table: exact integer sums (DESIGN.md "voxel contract"), 112 bytes */
typedef struct {
    int64_t  key;            /* ((k+2^20)<<42)|((j+2^20)<<21)|(i+2^20), ijk = floor(p * (1.0f/leaf)) */
    int64_t  sx, sy, sz;     /* sums of llrint(coord * 2^24) */
    uint64_t sr, sg, sb, n;  /* colour sums, point count */
    uint32_t hist[12];       /* label votes */
} ssm_voxel;

/* keys of /root/reference/parameters.txt that the path reads (include/orb.h:21-28, include/mapper.h:24-29,
 * include/track.h:69-70, src/parameter_reader.cpp:6-18) plus sizing knobs of this implementation */
typedef struct {
    int    width, height;            /* frame geometry the context is sized for */
    int    orb_features;             /* parameters.txt:66 */
    float  orb_scale;                /* :68 */
    int    orb_levels;               /* :69 */
    int    orb_iniThFAST;            /* :70 */
    int    orb_minThFAST;            /* :71 */
    double knn_match_ratio;          /* :72 */
    int    tracker_ref_frames;       /* :81 */
    double mapper_resolution;        /* :97 */
    double mapper_max_distance;      /* :98 */
    ssm_camera camera;               /* :37-40,63 */
    int    max_batch;                /* frames per batched launch (device workspace is sized for this) */
    int    voxel_capacity_log2;      /* slots the context's voxel map STARTS with = 2^this (8..28).  The map grows by itself like the reference's globalMap
                                        (src/mapper.cpp:121-158): it is re-hashed into a larger table whenever it is a quarter full */
    const int8_t* brief_pattern;     /* NULL = built-in 256x4 table; else 1024 int8 (x0,y0,x1,y1)*256.  Every point must have x^2 + y^2 <= SSM_BRIEF_MAX_R2 (342): turned by
                                        the keypoint's angle it then rounds to at most 18 (sqrt(342) = 18.493), the reach of the patch the BRIEF kernel stages;
                                        ssm_create refuses any other table with SSM_E_INVAL (before it looks for a device) */
    int    voxel_max_capacity_log2;  /* the map never grows beyond 2^this slots (default and maximum 28: 30 GB); a map that needs more fails with SSM_E_CAPACITY */
    /* the stereo path (configs[3]).  0 = the default of each */
    int    sgbm_form;                /* SGBM formulation: 2 (default) = two volumes, top-down sweep with strip hand-offs; 1 = four path volumes, no cross-block waits
                                        (also what a sweep that times out is repeated with); 3 = the round-3 five-volume form.  All give the same disparities */
    int    sgbm_streams;             /* 1 | 2 | 3 streams (and workspaces) that alternate sub-batches of the batched stereo path; default 2 */
    int    stereo_batch;             /* frame pairs per launch of ssm_stereo_seq_process; default: max_batch, at most 128 */
} ssm_config;

#define SSM_BRIEF_MAX_R2 342             /* largest x^2 + y^2 of a brief_pattern point */

typedef struct ssm_ctx ssm_ctx;

void        ssm_config_default(ssm_config* cfg);        /* parameters.txt values, 640x480 TUM fr1 camera at scale 1000 */
int         ssm_create(int device, const ssm_config* cfg, ssm_ctx** out);
void        ssm_destroy(ssm_ctx* ctx);
const char* ssm_last_error(const ssm_ctx* ctx);          /* valid until the next call on ctx; ctx==NULL: last create error */
const char* ssm_version(void);
int         ssm_orb_capacity(const ssm_ctx* ctx);        /* max keypoints per frame: orb_features + 3*orb_levels */
int         ssm_sync(ssm_ctx* ctx);
void*       ssm_stream(ssm_ctx* ctx);                    /* hipStream_t of the context */

/* ---- OrbFeature::detectFeatures (include/orb.h:32-53): gray conversion, ORB, 3-D position per keypoint.
 * img: 8-bit, channels 1 (gray) or 3 (BGR interleaved), row stride in bytes.  depth: u16 row-major w x h or NULL.
 * kps/desc/pos3d hold cap entries (desc 32 B each, pos3d 3 floats each, may be NULL). */
int ssm_orb_extract(ssm_ctx* ctx, const uint8_t* img, int w, int h, int stride, int channels, const uint16_t* depth,
                    ssm_keypoint* kps, uint8_t* desc, float* pos3d, int cap, int* n_out);

/* ---- cv::BFMatcher(NORM_HAMMING)::knnMatch(q,t,knn,2) as called at src/orb.cpp:21.  idx/dist: nq x 2.  Like ssm_match it completes the context's pending
 * asynchronous calls (below) before it returns. */
int ssm_hamming_knn2(ssm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* idx, int32_t* dist);
/* ---- OrbFeature::match (src/orb.cpp:16-29): knn + ratio test, ascending queryIdx */
int ssm_match(ssm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, double ratio,
              ssm_dmatch* out, int cap, int* n_out);
/* ---- asynchronous forms of the two calls a tracker frame makes (Tracker::trackRefFrame, src/track.cpp:140-163: detectFeatures, then one match per
 * reference frame).  The call stages its inputs in the context's pinned ring, enqueues the copies and kernels on the context stream and returns; the
 * results (and *n_out) are written into the caller's buffers by ssm_wait, which completes every pending call in the order it was made and returns the first
 * error.  Input buffers may be reused at once (they have been copied); OUTPUT buffers and n_out must stay valid until ssm_wait.  ssm_orb_extract / ssm_match
 * are these + ssm_wait; any other entry point of the context may be called in between (same stream: it runs behind the pending work). */
int ssm_orb_extract_async(ssm_ctx* ctx, const uint8_t* img, int w, int h, int stride, int channels, const uint16_t* depth,
                          ssm_keypoint* kps, uint8_t* desc, float* pos3d, int cap, int* n_out);
int ssm_match_async(ssm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, double ratio, ssm_dmatch* out, int cap, int* n_out);
int ssm_wait(ssm_ctx* ctx);
/* the loop `for (pFrame : refFrames) orb.match(pFrame, currentFrame)` of Tracker::trackRefFrame (src/track.cpp:150-152) as one call: refs[i] (nrefs[i] x 32
 * bytes) are the query sets, cur (ncur x 32) the train set of every pair; outs[i] (caps[i] entries) / n_outs[i] receive what ssm_match(refs[i], cur) gives.
 * One upload, one matrix-core launch for all pairs, one download.  ncur < 2: SSM_E_TOO_FEW_TRAIN; nrefs[i] == 0: n_outs[i] = 0. */
int ssm_match_refs(ssm_ctx* ctx, const uint8_t* const* refs, const int* nrefs, int nref, const uint8_t* cur, int ncur, double ratio,
                   ssm_dmatch* const* outs, const int* caps, int* n_outs);
int ssm_match_refs_async(ssm_ctx* ctx, const uint8_t* const* refs, const int* nrefs, int nref, const uint8_t* cur, int ncur, double ratio,
                         ssm_dmatch* const* outs, const int* caps, int* n_outs);          /* completed by ssm_wait */

/* ---- Mapper::semantic_motion_fuse (src/mapper.cpp:189-216): sem = BGR class-colour image, mask = w*h bytes */
int ssm_moving_mask(ssm_ctx* ctx, const uint8_t* sem_bgr, int w, int h, int stride, uint8_t* mask);
/* ---- Mapper::generatePointCloud (src/mapper.cpp:12-94) incl. RGBDFrame::project2dTo3d (include/rgbdframe.h:63-75)
 * and pcl::transformPointCloud by T (16 doubles, column-major = Eigen::Isometry3d::matrix(); NULL = camera frame).
 * packed images (stride = w*channels).  out holds cap points (w*h always suffices). */
int ssm_backproject(ssm_ctx* ctx, const uint16_t* depth, const uint8_t* rgb_bgr, const uint8_t* sem_bgr, int w, int h,
                    const ssm_camera* cam, const double* T, double max_distance, ssm_point* out, int cap, int* n_out);

/* ---- pcl::VoxelGrid::filter as used in Mapper::viewer (src/mapper.cpp:106-107,154-155) */
int ssm_voxel_filter(ssm_ctx* ctx, const ssm_point* pts, int n, float leaf, ssm_point* out, int cap, int* n_out);
/* ---- the device-resident form of the two calls above, for Mapper::viewer (src/mapper.cpp:96-171): a key-frame's gated camera-frame cloud is made ONCE
 * (mapper.cpp:17-20 caches frame->pointcloud) and STAYS in device memory as an ssm_cloud; a map update transforms the chosen clouds by their current
 * poses, adds them to the previous filtered map and runs the VoxelGrid pass, all on the device -- the viewer's `*map += *generatePointCloud(kf)` loop and
 * its `voxel.filter(*tmp)` without the key-frame clouds or the whole global map crossing PCIe on every update; only the published map is downloaded.
 * Results are the bytes ssm_backproject + host transform + ssm_voxel_filter give (exact integer sums: independent of the order points are added in). */
typedef struct ssm_cloud ssm_cloud;
int  ssm_backproject_dev(ssm_ctx* ctx, const uint16_t* depth, const uint8_t* rgb_bgr, const uint8_t* sem_bgr, int w, int h,
                         const ssm_camera* cam, double max_distance, ssm_cloud** cloud_out);      /* host images in; camera-frame cloud left on the device */
int  ssm_cloud_size(const ssm_cloud* cloud);
int  ssm_cloud_fetch(ssm_ctx* ctx, const ssm_cloud* cloud, const double* T, ssm_point* out, int cap, int* n_out);   /* transformed copy to the host (T = NULL: as stored) */
void ssm_cloud_free(ssm_ctx* ctx, ssm_cloud* cloud);
/* gives the device memory of the viewer's map path back: every slab whose clouds have all been freed, the concatenation buffer and the map buffer of
 * ssm_viewer_map_update (the next update allocates again).  Mapper::viewer calls it when it falls back to its host path after a device error (out of memory on a long
 * sequence), so that the host path's own device work has room.  test_fail_next: != 0 makes the NEXT ssm_viewer_map_update of the context fail with SSM_E_NOMEM (tests). */
int  ssm_viewer_map_release(ssm_ctx* ctx, int test_fail_next);
/* map <- VoxelGrid(leaf)( (rebuild ? nothing : the previous map's centroids) + sum over i of poses[i] * clouds[i] ); poses: n x 16 doubles, column-major, HOST.
 * A cloud extent PCL's VoxelGrid refuses (dx dy dz > INT_MAX) leaves the unfiltered concatenation as the map, like mapper.h's `*out = *in`. */
int  ssm_viewer_map_update(ssm_ctx* ctx, int rebuild, ssm_cloud* const* clouds, const double* poses, int n, float leaf, int* n_map_out);
int  ssm_viewer_map_fetch(ssm_ctx* ctx, ssm_point* out, int cap, int* n_out);                       /* the map after the last update (sorted by voxel index) */
/* the persistent map of the context: table of exact sums keyed by voxel.  It grows like the reference's globalMap (src/mapper.cpp:121-158) and never drops a
 * contribution below 2^voxel_max_capacity_log2 slots, whatever the stream does: ssm_seq_process sizes the table from the stream's own voxel rate; when a launch brings
 * far more than that (the camera leaves a near wall at a fine leaf), what the table refuses waits in an overflow list, and blocks of the map kernel that start
 * while that list is nearly full add nothing, log themselves and are run again after the table has grown -- which is why the DEVICE INPUTS of an
 * ssm_seq_process call whose map stage ran must stay unchanged until the next ssm_sync / ssm_map_size / ssm_map_export* / ssm_voxel_allgather of the context.
 * Only a map that needs more than the configured maximum loses contributions: the entry point that notices returns SSM_E_CAPACITY once, and from then on
 * ssm_map_size / ssm_map_export* / ssm_voxel_allgather keep returning SSM_E_CAPACITY for this map -- it is incomplete -- until ssm_map_clear.  Skipped points
 * (non-finite, or outside the 21-bit voxel index range) are reported once as SSM_E_VOXEL_RANGE and leave the map usable (pcl::VoxelGrid skips such points too). */
int ssm_map_clear(ssm_ctx* ctx);
int ssm_map_insert(ssm_ctx* ctx, const ssm_point* pts, int n);                 /* globalMap += cloud */
int ssm_map_size(ssm_ctx* ctx, int* n_voxels);
/* how the map got where it is: stats[0] = log2 of the table's slots now, [1] = times it was re-hashed into a larger table, [2] = blocks of the map kernel that were
 * run again after skipping themselves, [3] = records its overflow list holds (a context that has run the map stage of ssm_seq_process keeps the large list) */
int ssm_map_stats(ssm_ctx* ctx, int64_t stats[4]);
int ssm_map_export(ssm_ctx* ctx, ssm_point* out, int cap, int* n_out);         /* centroids sorted by voxel index */
int ssm_map_export_table(ssm_ctx* ctx, ssm_voxel* out, int cap, int* n_out);   /* key-sorted table, for merging */
int ssm_map_merge_table(ssm_ctx* ctx, const ssm_voxel* tab, int n);            /* add another rank's table */
/* same two with DEVICE buffers (the RCCL all-gather of per-GPU tables works on device memory); export is synchronous
 * (it needs the voxel count on the host), merge is enqueued on the context stream.  ssm_map_size and ssm_map_export_table_dev wait for the MAP: after
 * an ssm_seq_process whose map stage ran on a side stream they wait for that stream only, and the call's ORB -> match chain may still be running when
 * they return (its outputs are ordered on the context stream as always; ssm_sync waits for everything).  A loop of ssm_map_clear / ssm_seq_process /
 * ssm_map_export_table_dev per sequence therefore keeps the GPU busy across its iterations. */
int ssm_map_export_table_dev(ssm_ctx* ctx, ssm_voxel* out_dev, int cap, int* n_out);
int ssm_map_merge_table_dev(ssm_ctx* ctx, const ssm_voxel* tab_dev, int n);

/* ---- multi-GPU (BASELINE.json configs[4]).  The reference is one process (experiment/exp_mapping.cpp:18-59), so these have no
 * counterpart there.  One process per GPU; frames shard by contiguous block (each rank first runs its tracker_ref_frames halo frames with
 * stages = SSM_STAGE_ORB, then its block with continue_sequence = 1, so that the match tables equal the single-GPU ones, src/track.cpp:150-152);
 * every rank fuses its frames into its own context map; ssm_voxel_allgather merges the maps with ONE RCCL all-gather over xGMI.
 * Bootstrap without any framework: rank 0 calls ssm_comm_get_unique_id and ships the SSM_COMM_ID_BYTES bytes to the other ranks (file, pipe,
 * MPI, torch.distributed ...); every rank calls ssm_comm_init_rank (= ncclCommInitRank on the context's device). */
#define SSM_COMM_ID_BYTES 128
int ssm_comm_get_unique_id(void* id /* SSM_COMM_ID_BYTES */);
int ssm_comm_init_rank(ssm_ctx* ctx, int nranks, int rank, const void* id);
int ssm_comm_finalize(ssm_ctx* ctx);
int ssm_comm_rank(const ssm_ctx* ctx);
int ssm_comm_size(const ssm_ctx* ctx);
/* COLLECTIVE: every rank of the communicator must call it, and every rank gets the same return code -- the voxel counts travel together with each
 * rank's table-full flag, and an allocation failure of the receive buffer is agreed on by a second 4-byte all-gather, so no rank can leave between two
 * collectives while its peers wait in the next one (on any failure no rank has merged anything).
 * rccl_comm: a ncclComm_t the caller created for this context's device, or NULL = the context's own communicator.  Afterwards the context
 * map of EVERY rank holds the union of all ranks' maps (exact integer sums: bit-identical on every rank and to the single-GPU map).
 * On the context stream: all-gather of the voxel counts, one in-place all-gather of the tables padded to the longest, re-insertion of the
 * nranks - 1 remote tables.  Waits on the host once (for the counts); the merge kernels are enqueued, not waited for. */
int ssm_voxel_allgather(ssm_ctx* ctx, void* rccl_comm);

/* ---- device-resident batched path (the benchmarked one): n frames of a sequence, packed, all DEVICE pointers.
 * Runs detectFeatures for every frame, match(ref, cur) against the <= tracker_ref_frames preceding frames (the
 * refFrames deque of Tracker::trackRefFrame, src/track.cpp:150-152, when every frame tracks), the moving mask,
 * generatePointCloud with pose[f], and fuses every cloud into the context map. */
typedef struct {
    const uint8_t*  bgr;      /* n x h x w x 3 */
    const uint16_t* depth;    /* n x h x w     */
    const uint8_t*  sem_bgr;  /* n x h x w x 3 */
    const double*   pose;     /* n x 16, column-major T_f_w */
    int n;
    int continue_sequence;    /* 1: the last tracker_ref_frames frames of the previous call are the first refs */
    int stages;               /* bit mask of SSM_STAGE_*, 0 = all */
} ssm_frames_dev;
enum { SSM_STAGE_ORB = 1, SSM_STAGE_MATCH = 2, SSM_STAGE_MAP = 4,
       SSM_STAGE_SEGNET = 8 /* BASELINE configs[2]: labels come from the on-GPU SegNet instead of sem_bgr (sem_bgr may be NULL) */ };
typedef struct {              /* DEVICE pointers owned by the context, valid until the next ssm_seq_process/destroy */
    const ssm_keypoint* kps;  /* n x cap */
    const uint8_t*  desc;     /* n x cap x 32 */
    const float*    pos3d;    /* n x cap x 3 */
    const int32_t*  nkp;      /* n */
    const ssm_dmatch* matches;/* n x R x cap ; slot r of frame f = match(frame f-R+r ... ), see nmatch */
    const int32_t*  nmatch;   /* n x R ; -1 where the ref frame does not exist */
    const int32_t*  npoints;  /* n : points emitted by generatePointCloud */
    int cap, R;
} ssm_seq_out_dev;
int ssm_seq_process(ssm_ctx* ctx, const ssm_frames_dev* in, ssm_seq_out_dev* out);

/* ---- Tracker::updateFrame in bulk (src/track.cpp:8-36,140-212): the consumer of ssm_seq_process's match tables that closes the pose loop.
 * ssm_seq_process computes features and match tables for whole sub-sequences ahead of the pose chain; ssm_tracker_run then walks the frames of that
 * call in order and does, per frame, what Tracker::updateFrame does in RGB-D mode: initFirstFrame / trackRefFrame / lostRecover -- the refFrames deque
 * (<= tracker_ref_frames successfully tracked frames), for every reference frame the matches (reference -> current), the 3-D points of the matched
 * reference features moved to the world by the inverse reference pose (track.cpp:150-163), PnPSolver::solvePnP (src/pnp.cpp:5-118) from
 * speed * lastPose, the < 15 correspondences / < 15 inliers tests, cntLost / max_lost_frame -> LOST -> lostRecover.  A reference frame that is one of
 * the tracker_ref_frames frames in front of the current one uses the precomputed table slot; after a tracking failure the deque holds older frames,
 * and those pairs are matched on demand (OrbFeature::match through the same matcher kernels), so the result is the per-frame Tracker's, bit for bit
 * (one numeric contract: include/ssm/pnp_core.h).  The solved poses go back into a stages = SSM_STAGE_MAP pass of ssm_seq_process.
 * The tracker object keeps the state between calls (speed, lastPose, cntLost, the deque with the features of its frames). */
typedef struct ssm_tracker ssm_tracker;
typedef struct {
    int32_t max_lost_frame;   /* tracker_max_lost_frame (include/track.h:69; 10) */
    int32_t ref_frames;       /* tracker_ref_frames (:70; 5) -- must equal the context's */
    int32_t pnp_min_inliers;  /* pnp_min_inliers (include/pnp.h; 10): only PnPSolver's unused return value depends on it */
    int32_t use_device;       /* 1: solve the pose chain of regular frames on the GPU (kernels_pnp.hip: a cluster of eight blocks per chain, one block for an own_stream tracker; SSM_PNP_BLOCKS overrides); 0: on the host.  Same bits. */
    double  first_pose[16];   /* T_f_w the first frame arrives with (initFirstFrame leaves it alone), column-major */
    int32_t own_stream;       /* 1: the device chain of this tracker runs on a stream of its own (behind what the context's stream holds at the time of the
                                 call), so that trackers of independent sequences, driven from different host threads, solve side by side -- a chain is one
                                 block = one CU of 256.  0: on the context's stream */
    int32_t blocks;           /* blocks per device chain: 1, 2, 4 or 8; 0 = default (8; 1 for an own_stream tracker).  Same bits in every form */
} ssm_tracker_params;
typedef struct { int32_t state; /* Tracker::getState() after the frame: 1 OK, 2 LOST */ int32_t tracked; /* 1: the frame joined refFrames */
                 int32_t n_matches; /* correspondences handed to solvePnP (-1: none gathered) */ int32_t n_inliers; } ssm_track_info;
void ssm_tracker_params_default(ssm_tracker_params* p);
int  ssm_tracker_create(ssm_ctx* ctx, const ssm_tracker_params* p, ssm_tracker** out);
void ssm_tracker_destroy(ssm_tracker* t);
int  ssm_tracker_reset(ssm_tracker* t);                       /* back to NOT_READY */
/* seq: the output of the most recent ssm_seq_process on the tracker's context (stages ORB | MATCH at least), n its frame count.  The frames are taken
 * as the continuation of the frames of the previous ssm_tracker_run.  pose_out: n x 16 doubles (HOST, column-major): RGBDFrame::T_f_w of every frame as
 * updateFrame leaves it (a frame that fails to track keeps the prediction speed * refFrames.back()); info_out: n entries (HOST, may be NULL). */
int  ssm_tracker_run(ssm_tracker* t, const ssm_seq_out_dev* seq, int n, double* pose_out, ssm_track_info* info_out);
const char* ssm_tracker_last_error(const ssm_tracker* t);
/* frames solved by the device chain / by the host path so far (use_device = 1: the host path takes the first frame, lostRecover, and the frames whose
 * refFrames deque reaches behind the match-table window after a tracking failure) */
int  ssm_tracker_stats(const ssm_tracker* t, int64_t* device_frames, int64_t* host_frames);
/* what the device chain has computed so far, for a roofline of PnPSolver::solvePnP (src/pnp.cpp:5-118: g2o's optimize(10) x 4 rounds): work[0] = Levenberg iterations
 * (one pass over the edges each: chi2 + normal equations), work[1] = chi2 passes (one per trial + one per optimize), work[2] / work[3] = level-0 edges those evaluated */
int  ssm_tracker_work(const ssm_tracker* t, int64_t work[4]);

/* ---- QuadFeatureMatch (include/quadmatcher.hpp:51-136, src/quadmatcher.cpp): the stereo quad matcher of the KITTI path
 * (Tracker::estimateVO, src/track.cpp:45-55).  Images are 8-bit gray, any size (buffers are re-sized on demand). */
/* layout-identical to struct pmatch (include/quadmatcher.hpp:33-49), 52 bytes */
typedef struct { float u1p, v1p; int32_t i1p; float u2p, v2p; int32_t i2p; float u1c, v1c; int32_t i1c; float u2c, v2c; int32_t i2c; int16_t dis_c, dis_p; } ssm_pmatch;
/* init(DET_GFTT, ..) + detectFeature() + circularMatching() in tracking mode (mode_track = true): GFTT (quality 0.04,
 * minDistance 8, max_corners: cv default 1000) on the current-left image, four pyramidal LK passes lc->rc, rc->rp,
 * rp->lp, lc->lp (11x11 window, 3 pyramid levels, <= 200 iterations, eps 0.01, min-eigen threshold 1e-6),
 * filteringTracks.  out: quadmatches in feature order. */
int ssm_quad_track(ssm_ctx* ctx, const uint8_t* lc, const uint8_t* rc, const uint8_t* lp, const uint8_t* rp, int w, int h, int stride,
                   int max_corners, ssm_pmatch* out, int cap, int* n_out);
/* the two OpenCV calls on their own: cv::goodFeaturesToTrack (blockSize 3, no Harris) and cv::calcOpticalFlowPyrLK
 * (win 11x11, maxLevel 3, OPTFLOW_LK_GET_MIN_EIGENVALS).  pts arrays hold (x, y) float pairs. */
int ssm_gftt(ssm_ctx* ctx, const uint8_t* img, int w, int h, int stride, int max_corners, double quality, double min_distance,
             float* pts, int cap, int* n_out);
int ssm_lk_track(ssm_ctx* ctx, const uint8_t* prev, const uint8_t* next, int w, int h, int stride, const float* prev_pts, int n,
                 float* next_pts, uint8_t* status, float* err, int max_count, double epsilon, double min_eig_threshold);
/* QuadFeatureMatch::matching on binary descriptors (:41-83, caldistance :525-544): windowed brute-force nearest
 * neighbour, one DMatch per query (trainIdx -1 when unmatched), kp = (x, y) float pairs, descriptors 32 B */
int ssm_window_match(ssm_ctx* ctx, const float* kp1, const uint8_t* d1, int n1, const float* kp2, const uint8_t* d2, int n2,
                     int search_width, int search_height, float distance_threshold, ssm_dmatch* out);

/* ---- depth from stereo: calDisparity_SGBM (src/stereo.cpp:11-30, cv::StereoSGBM) and FrameReader's disparity -> depth
 * conversion with the 3-D ROI gate (src/rgbdframe.cpp:81-116) -------------------------------------------------------------
 * params mirror the public fields of cv::StereoSGBM (fullDP = false).  ssm_sgbm_params_default fills what stereo.cpp sets:
 * 80 disparities, SAD window 11, P1 = 4*11*11, P2 = 32*11*11, uniqueness 10, speckle window 100 / range 32, disp12MaxDiff 1,
 * preFilterCap 63.  left / right: rectified 8-bit images.  disp: int16 per pixel, fixed point with 4 fractional bits,
 * (minDisparity - 1) * 16 where no disparity was accepted (what cv::StereoSGBM::operator() writes).  stage 1 stops after
 * computeDisparitySGBM (no medianBlur / filterSpeckles), for tests.  numberOfDisparities: a multiple of 16, <= 128.  minDisparity >= 2: OpenCV 2.4 reads its half-sample
 * interval buffers outside the range it filled there (calcPixelCostBT); this library uses the intervals of the pixels actually compared -- the
 * reference sets minDisparity = 0. */
typedef struct { int32_t minDisparity, numberOfDisparities, SADWindowSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio,
                 speckleWindowSize, speckleRange; } ssm_sgbm_params;
void ssm_sgbm_params_default(ssm_sgbm_params* p);
int ssm_sgbm(ssm_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int stride, const ssm_sgbm_params* params, int stage, int16_t* disp);
/* the whole depth step of FrameReader::next() in KITTI mode: SGBM, then depth = ushort(f * baseline / d * 16 * scale) inside
 * the ROI (|x| < roix, |y| < roiy, 0 < z < roiz), 0 elsewhere and where d is 0 or the image's minimum disparity value.
 * disp (may be NULL) receives the disparity image too. */
int ssm_stereo_depth(ssm_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int stride, const ssm_sgbm_params* params,
                     double baseline, double cu, double cv, double f, double roix, double roiy, double roiz, double scale,
                     uint16_t* depth, int16_t* disp);

/* ---- stereo visual odometry on the quad matches: VisualOdometryStereo::estimateMotion (src/vo_stereo.cpp:47-152) --------
 * params mirror VisualOdometryStereo::parameters (include/vo_stereo.hpp: calib.f/cu/cv, base, inlier_threshold,
 * reweighting).  samples: iters x 3 match indices, what VisualOdometry::getRandomSample (src/vo.cpp:74-93) draws per RANSAC
 * iteration -- the host class owns the rand() stream (include/ssm/vo_stereo.hpp).  tr = (rx, ry, rz, tx, ty, tz) of
 * the best hypothesis after refinement; inliers (cap entries) / n_inliers = its consensus set in index order; *success = 0
 * where the reference returns an empty vector (fewer than 6 matches or inliers, refinement not converged).
 * Contracts (sin/cos, LU, summation order): oracle/vo.c. */
typedef struct { double f, cu, cv, base, inlier_threshold; int32_t reweighting, pad; } ssm_vo_params;
int ssm_vo_estimate(ssm_ctx* ctx, const ssm_pmatch* matches, int n, const ssm_vo_params* params, const int32_t* samples, int iters,
                    double tr[6], int32_t* inliers, int cap, int* n_inliers, int* success);

/* ---- PnPSolver::solvePnP (reference src/pnp.cpp:5-118) for ONE correspondence list, on the device -----------------------------------
 * The per-frame caller's entry point (Tracker::trackRefFrame, src/track.cpp:166-175; PnPSolver::solvePnPLazy, src/pnp.cpp:120-226): img = n x 2
 * pixels in frame 2, obj = n x 3 points in frame 1's camera frame ((0,0,0) = no depth: skipped as pnp.cpp:34 does), cam = (fx, fy, cx, cy),
 * T = column-major 4 x 4, initial value in, estimate out.  inliers (n bytes, may be NULL) = the flag vector as pnp.cpp keeps it (SURVEY.md
 * Appendix A quirk 14), *n_inliers = the number of set flags, *success (may be NULL) = the reference's return value (n > min_inliers: the
 * vector's LENGTH is what pnp.cpp:115 tests).  One 1024-thread block of kernels_pnp.hip; the result is the same bits as ssm_pnp::solve of
 * include/ssm/pnp_core.h on the host (lane-ordered sums, polynomial sin / cos) and as oracle/pnp.c.  n <= 65535. */
int ssm_pnp_solve(ssm_ctx* ctx, const float* img, const float* obj, int n, const double cam[4], int min_inliers, double T[16],
                  uint8_t* inliers, int* n_inliers, int* success);
int ssm_debug_pnp_solve_blocks(ssm_ctx* ctx);                            /* 8 or 1: the blocks the context's next ssm_pnp_solve starts with (1 after a cluster timed out once) */
int ssm_pnp_lds_edge_capacity(void);                                  /* the largest n whose edge list the device solve keeps in LDS (above it: in global memory, same bits): the tests build their sizes around it */

/* ---- Looper (reference include/looper.h, src/looper.cpp): the DBoW2 bag-of-words loop detector ------------------------------------------------------
 * Looper::add is vocab.transform(descriptors, frame->bowVec, ..), Looper::getPossibleLoops is vocab.score(frame, pf) against every stored key-frame with
 * `score > min_sim_score && abs(pf->id - frame->id) > min_interval`.  DBoW2 is not in the reference tree; DESIGN.md s.10 restates the contract of
 * TemplatedVocabulary<FORB> as ORB-SLAM2 ships it, and include/ssm/looper_core.h holds the arithmetic (host and device give the same bits).
 * A VOCABULARY is a host object and needs no GPU.  The text format is DBoW2's saveToTextFile (looper_vocab_file, parameters.txt:91): line 1 `k L scoring
 * weighting`, then one node per non-blank line `parent isLeaf b0 .. b31 weight`; node ids count from 1 in line order, id 0 is the root; word ids count from
 * 0 in order of the isLeaf > 0 lines.  0 <= k <= 20, 1 <= L <= 10.  ONLY scoring == 0 (L1_NORM) with weighting == 0 (TF_IDF) -- what ORBvoc.txt uses -- is
 * supported: anything else, a parent that is not an earlier node, a leaf with children, a non-leaf or a root without children and a malformed line are
 * SSM_E_INVAL, with the reason in ssm_last_error(NULL).  The FeatureVector (levelsup = 4) that Looper::add computes and drops is not built. */
typedef struct ssm_vocab ssm_vocab;
int  ssm_vocab_load_text(const char* path, ssm_vocab** out);
/* the same from arrays: node i (id i + 1) has parent[i] (an id), is_leaf[i], desc + 32 i, weight[i] */
int  ssm_vocab_create(int k, int L, int scoring, int weighting, const int32_t* parent, const uint8_t* is_leaf,
                      const uint8_t* desc, const double* weight, int n_nodes, ssm_vocab** out);
void ssm_vocab_destroy(ssm_vocab* v);
int  ssm_vocab_info(const ssm_vocab* v, int32_t info[6]);             /* k, L, nodes incl. the root, words, scoring, weighting */
/* vocab.transform on the host: word_of_feature (n entries, may be NULL) = the word id of every descriptor; (ids, vals) = the normalised vector in ascending
 * word id, *n_out entries (more than cap: SSM_E_CAPACITY, *n_out = the count needed) */
int  ssm_vocab_transform_host(const ssm_vocab* v, const uint8_t* desc, int n, int32_t* word_of_feature,
                              int32_t* ids, double* vals, int cap, int* n_out);
/* vocab.score(v1, v2): v1 = the query frame, v2 = the stored frame (the sum runs over v2's entries: looper_core.h) */
int  ssm_bow_score_host(const int32_t* ids1, const double* v1, int n1, const int32_t* ids2, const double* v2, int n2, double* score);
/* the arrays ssm_vocab_create / the text file take, in the order the vocabulary was given (node i has id i + 1): parent, is_leaf: cap entries, desc: cap x
 * 32, weight: cap (0.0 for inner nodes); any of them may be NULL.  cap < nodes - 1: SSM_E_CAPACITY.  ssm_vocab_create on them gives an equal vocabulary */
int  ssm_vocab_export(const ssm_vocab* v, int32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight, int cap);
/* DBoW2's text format, as ssm_vocab_load_text reads it; weights with 17 significant digits: load(save(v)) exports the same bits */
int  ssm_vocab_save_text(const ssm_vocab* v, const char* path);
/* VOCABULARY TRAINING (include/ssm/vocab_train_core.h): a hierarchical k-majority tree over the descriptors of F frames -- desc: N x 32, frame
 * 0's first; n_per_frame[F]: counts (zeros allowed) that sum to N, 1 <= N <= 2^26.  Farthest-point seeding, nearest-centre assignment (lowest centre on ties),
 * bitwise-majority centres (a tie gives 1), at most max_iters passes per node, breadth-first ids, weight = log(F / frames that hold the word).  Integers only,
 * so the host function and the device path give the same vocabulary, word_of_feature (N entries, may be NULL: the word every training descriptor was trained
 * into, which is also where ssm_vocab_transform_host puts it) and report, byte for byte.  Bad parameters: SSM_E_INVAL. */
typedef struct { int32_t k, L, max_iters; } ssm_vocab_train_params;                    /* 2 .. 20, 1 .. 10, >= 1 */
typedef struct {
    int32_t nodes, words;            /* nodes incl. the root */
    int32_t levels;                  /* the deepest level that holds a node */
    int32_t capped_nodes;            /* nodes whose max_iters-th pass still changed an assignment */
    int32_t passes[10];              /* per level l (the nodes of level l being split): the assignment passes after seeding, the maximum over its nodes */
} ssm_vocab_train_report;
void ssm_vocab_train_params_default(ssm_vocab_train_params* p);                        /* 10, 5, 32 */
int  ssm_vocab_train_host(const uint8_t* desc, const int32_t* n_per_frame, int n_frames, const ssm_vocab_train_params* params,
                          int32_t* word_of_feature, ssm_vocab_train_report* report, ssm_vocab** out);
int  ssm_vocab_train(ssm_ctx* ctx, const uint8_t* desc, const int32_t* n_per_frame, int n_frames, const ssm_vocab_train_params* params,
                     int32_t* word_of_feature, ssm_vocab_train_report* report, ssm_vocab** out);
/* ONE pass of step 4 (centre update, then assignment) on a state the caller makes up: descriptor i belongs to node node_of[i] (non-decreasing, < n_nodes)
 * and cluster cluster_of[i] (< k); centres: n_nodes x k x 32, in and out (an empty cluster keeps its row); assign_out[i]: the new cluster.  ctx NULL: the
 * host function.  Tests reach emptied clusters and constructed ties this way */
int  ssm_debug_vocab_kmajority(ssm_ctx* ctx, const uint8_t* desc, int n, const int32_t* node_of, const int32_t* cluster_of, int n_nodes, int k,
                               uint8_t* centres, int32_t* assign_out);
/* wall time of the last ssm_vocab_train on this context per level (upload / the final word pass are in total_ms only): scripts/vocab_train_bench.py */
int  ssm_debug_vocab_train_times(ssm_ctx* ctx, double level_ms[10], double* total_ms);
/* A LOOPER belongs to a context: the vocabulary tree (re-numbered breadth-first, 32-byte descriptor rows) and the database of the added frames' vectors
 * (CSR: offsets, word ids, f64 values, frame ids; grows by doubling) live in the context's device memory.  ssm_looper_create uploads and waits: v may be
 * destroyed afterwards.  Entries are numbered in the order they were added.  A frame holds at most ssm_orb_capacity descriptors (at most 4096). */
typedef struct ssm_looper ssm_looper;
int  ssm_looper_create(ssm_ctx* ctx, const ssm_vocab* v, ssm_looper** out);
void ssm_looper_destroy(ssm_looper* l);
int  ssm_looper_clear(ssm_looper* l);                                 /* forget every entry (the memory stays) */
int  ssm_looper_size(const ssm_looper* l);                            /* entries */
int  ssm_looper_add(ssm_looper* l, const uint8_t* desc, int n, int frame_id);          /* Looper::add of one frame, host descriptors; synchronous */
/* Looper::add of n_frames frames whose descriptors are on the device: desc_dev (n_frames x cap x 32) / nkp_dev (n_frames) = ssm_seq_out_dev.desc / .nkp as
 * they are (cap = ssm_orb_capacity); frame_ids: HOST, copied before the call returns.  Enqueued on the context stream, not waited for */
int  ssm_looper_add_dev(ssm_looper* l, const uint8_t* desc_dev, const int32_t* nkp_dev, int n_frames, int cap, const int32_t* frame_ids);
int  ssm_looper_bow(ssm_looper* l, int entry, int32_t* ids, double* vals, int cap, int* n_out);     /* an entry's vector */
/* scores[e] = score(entry, e) for e in [0, against), or for e in [0, entry] when against = -1 */
int  ssm_looper_scores(ssm_looper* l, int entry, int against, double* scores);
/* Looper::getPossibleLoops for the query entries [first, first + n): entry q is compared with the entries [0, against), or with 0 .. q when against = -1
 * (the reference's order: add(frame) directly before getPossibleLoops(frame)).  pairs: cap x 2 (query entry, candidate entry), sorted by (query, candidate);
 * scores: cap.  More than cap candidates: SSM_E_CAPACITY, *n_out = the count needed.  Waits once, for the download */
int  ssm_looper_query(ssm_looper* l, int first, int n, int against, double min_sim_score, int min_interval,
                      int32_t* pairs, double* scores, int cap, int* n_out);

/* ---- UVDisparity::Process (include/uvdisparity.hpp, src/uvdisparity.cpp:842-903) with triangulate10D, correct3DPoints and setImageROI
 * (src/stereo.cpp:41-192): the moving-object mask, the ROI mask, the ground (obstacle) mask and the pitch of a stereo frame from its left image, its
 * SGBM disparity (x16 fixed point) and the quad matches with their VO inlier flags.  DESIGN.md s.11 is the contract; include/ssm/uvd_core.h the per-pixel
 * arithmetic, shared by the kernels and the host function, so device == host bit for bit.  Disparities 0 < d / 16 <= 255 are supported. */
typedef struct {
    double f, cu, cv, base;                  /* CalibPars */
    double roi_x, roi_y, roi_z;              /* ROI3D (parameters.txt camera.roix / roiy / roiz: include/track.h:80-86) */
    int32_t min_intense, min_disparity_raw, min_area;       /* USegmentPars() = 32, 64, 40 */
    int32_t inlier_tolerance;                /* SetInlierTolerance(3), include/track.h:100 */
} ssm_uvd_params;
enum { SSM_UVD_TOO_LARGE = 1 /* a disparity above 255 x 16 */, SSM_UVD_NO_LINE = 2 /* v_cols <= 26 or fewer than 2 line points */, SSM_UVD_SKIPPED = 4 /* nmatch < 0 */ };
typedef struct {
    int32_t status;                          /* SSM_UVD_* bits; any bit: the three masks are zero and the Kalman filters did not move */
    int32_t v_cols, u_rows;                  /* ceil(max / 16), and that + 1 */
    int32_t otsu_threshold, n_line_points;
    float   slope;                           /* b / a of the ground line in the V-disparity image */
    double  v_c;                             /* its intercept */
    float   pitch_measured, pitch_filtered;  /* (float)atan((cv - v_c) / f) = Process' pitch1 = pitch2; Kalman filter 1's state after this frame */
    int32_t n_seeds, n_masks_found, n_masks_merged, n_masks_kept;     /* flood fills started; of area > min_area; after mergeMasks; after verifyByInliers */
    int32_t n_moving;                        /* pixels of the moving mask that are 255 */
    float   line[4];                         /* fitLine's (cos t, sin t, mean x, mean y) */
    int32_t pad;
} ssm_uvd_info;
typedef struct ssm_uvd ssm_uvd;
void ssm_uvd_params_default(ssm_uvd_params* p);          /* include/track.h:84-101 + USegmentPars(); the calibration is KITTI 00's (parameters.txt) */
/* the object owns the workspaces and the two Kalman filters.  ctx may be NULL: an object for ssm_uvd_process_host only, which needs no GPU */
int  ssm_uvd_create(ssm_ctx* ctx, const ssm_uvd_params* params, ssm_uvd** out);
void ssm_uvd_destroy(ssm_uvd* u);
int  ssm_uvd_reset(ssm_uvd* u);                           /* the Kalman filters start again from x = 0, P = 1 */
/* one pair, HOST pointers; left (bytes) and disp (int16) have rows of `stride` elements, the masks (w x h bytes, packed; each may be NULL) are written.
 * matches / inlier_flags (n_matches; 1 = VO inlier, 0 = outlier) are in/out the way filterInOut edits vo.quadmatches_inlier / _outlier: a match that
 * is erased gets bit 1 (value 2) of its flag set, one that stays gets its dis_c recorded.  n_matches < 0 skips the frame like nmatch[i] < 0 below.  Synchronous */
int  ssm_uvd_process(ssm_uvd* u, const uint8_t* left, const int16_t* disp, int w, int h, int stride, ssm_pmatch* matches, uint8_t* inlier_flags,
                     int n_matches, uint8_t* moving, uint8_t* roi, uint8_t* ground, ssm_uvd_info* info);
/* n frames in frame order; left_dev / disp_dev (n x h x w, packed) and the masks (n x h x w bytes; each may be NULL) are DEVICE pointers, e.g.
 * ssm_stereo_out_dev.disp of a chunk.  matches (n x cap), nmatch (n) and inlier_flags (n x cap) are HOST arrays, edited as above; nmatch[i] < 0 skips
 * frame i (viso.Process failed: the reference does not run the block, src/track.cpp:62-79): zero masks, SSM_UVD_SKIPPED, the Kalman state does not move.
 * info: n entries.  Three device phases around two host steps, one wait each; returns when the masks are complete.  The context's lock is released during
 * the host steps (other threads of the context run meanwhile); one ssm_uvd object serves one thread at a time */
int  ssm_uvd_process_dev(ssm_uvd* u, const uint8_t* left_dev, const int16_t* disp_dev, int n, int w, int h, ssm_pmatch* matches, const int32_t* nmatch,
                         uint8_t* inlier_flags, int cap, uint8_t* moving_dev, uint8_t* roi_dev, uint8_t* ground_dev, ssm_uvd_info* info);
/* ssm_uvd_process on the CPU: the same functions of uvd_core.h, the same bits.  Needs no GPU */
int  ssm_uvd_process_host(ssm_uvd* u, const uint8_t* left, const int16_t* disp, int w, int h, int stride, ssm_pmatch* matches, uint8_t* inlier_flags,
                          int n_matches, uint8_t* moving, uint8_t* roi, uint8_t* ground, ssm_uvd_info* info);
/* intermediate images of frame `frame` of the last call, for the tests (each may be NULL): v_dis h x 256 (columns from v_cols on are zero), u_dis
 * u_rows x w after adjustUdisIntense, bin h x 256 (the Otsu image, v_cols columns used), union_mask u_rows x w */
int  ssm_debug_uvd_images(ssm_uvd* u, int frame, uint8_t* v_dis, uint8_t* u_dis, uint8_t* bin, uint8_t* union_mask);
/* one recorded stage of that frame, packed: 1 blurred, 2 eroded, 3 binary (h x v_cols bytes), 4 the point list (int32 x, y pairs), 5 the U-disparity
 * image before the adjustment (u_rows x w), 7 the area of every flood fill (int32), 8 / 9 / 10 the masks found / merged / kept (each u_rows x w bytes).
 * *bytes: the stage's size (out NULL: only that; more than cap: SSM_E_CAPACITY) */
/* on != 0: later calls keep a copy of every mask found / merged / kept per frame (stages 8 - 10; SSM_E_INVAL without it).  Off by default: the masks then move
 * through findAllMasks, mergeMasks and verifyByInliers without being copied */
int  ssm_debug_uvd_record(ssm_uvd* u, int on);
int  ssm_debug_uvd_stage(ssm_uvd* u, int frame, int stage, void* out, size_t cap, size_t* bytes);
/* host wall time of the last ssm_uvd_process / ssm_uvd_process_dev in milliseconds: host step 1 (lines, Kalman), host step 2 (filter, fills, merge, verify),
 * the whole call with its three waits.  For scripts/uvd_bench.py */
int  ssm_debug_uvd_times(ssm_uvd* u, double ms[3]);

/* ---- the semantic-motion fusion (reference src/mapper.cpp:217-271 with the Car class of src/mapper.cpp~:146-229): the maybe-moving classes of the semantic
 * image, dilated, taken as outer blobs with their holes filled; a blob joins the moving mask when it is large and enough of it lies under the motion mask
 * (UVDisparity's).  DESIGN.md s.14 is the contract; include/ssm/motion_fuse_core.h the arithmetic shared by the device path and the host function.
 * sem: BGR class colours; motion: w x h bytes, packed, only 255 counts; NULL = no motion, and the mask is then ssm_moving_mask's byte for byte. */
typedef struct { int32_t area_thres; int32_t pad; double overlay_thres; } ssm_motion_fuse_params;
typedef struct { int32_t blobs, large, confirmed, added; } ssm_motion_fuse_info;       /* blobs; those with area > area_thres; those confirmed; mask pixels the always-moving classes did not set */
void ssm_motion_fuse_params_default(ssm_motion_fuse_params* p);          /* parameters.txt: motion_area_thres 1000, motion_overlay_portion_thres 0.143 */
void ssm_motion_fuse_tile(int32_t wh[2]);                                /* the device labelling's tile (width, height): the tests build their sizes around it */
/* host images of any size (stride: bytes per row of sem); info may be NULL */
int  ssm_motion_fuse(ssm_ctx* ctx, const uint8_t* sem, const uint8_t* motion, int w, int h, int stride, const ssm_motion_fuse_params* params, uint8_t* mask,
                     ssm_motion_fuse_info* info);
/* n packed frames in device memory, one launch sequence and one wait; mask_dev: n x w x h; info: n entries on the host (may be NULL) */
int  ssm_motion_fuse_dev(ssm_ctx* ctx, const uint8_t* sem_dev, const uint8_t* motion_dev, int n, int w, int h, const ssm_motion_fuse_params* params,
                         uint8_t* mask_dev, ssm_motion_fuse_info* info);
/* the same on the CPU, the same bits; needs no GPU.  labels (w x h int32: the smallest row-major index of the pixel's blob, -1 outside every blob), area and
 * overlap (w x h int32: the blob's figures at its root pixel, 0 elsewhere) and cand (w x h bytes) may each be NULL */
int  ssm_motion_fuse_host(const uint8_t* sem, const uint8_t* motion, int w, int h, int stride, const ssm_motion_fuse_params* params, uint8_t* mask,
                          ssm_motion_fuse_info* info, int32_t* labels, int32_t* area, int32_t* overlap, uint8_t* cand);
/* what ssm_motion_fuse_host hands out, of frame `frame` of the context's last device call (each may be NULL) */
int  ssm_debug_motion_fuse(ssm_ctx* ctx, int frame, int32_t* labels, int32_t* area, int32_t* overlap, uint8_t* cand);
/* ssm_backproject / ssm_backproject_dev with the fusion in the place of the class mask: points under the fused mask are dropped.  motion NULL: the bytes of
 * the plain calls.  params NULL: the defaults */
int  ssm_backproject_fused(ssm_ctx* ctx, const uint16_t* depth, const uint8_t* rgb_bgr, const uint8_t* sem_bgr, const uint8_t* motion, int w, int h,
                           const ssm_camera* cam, const double* T, double max_distance, const ssm_motion_fuse_params* params, ssm_point* out, int cap, int* n_out);
int  ssm_backproject_fused_dev(ssm_ctx* ctx, const uint16_t* depth, const uint8_t* rgb_bgr, const uint8_t* sem_bgr, const uint8_t* motion, int w, int h,
                               const ssm_camera* cam, double max_distance, const ssm_motion_fuse_params* params, ssm_cloud** cloud_out);

/* ---- statistical outlier removal of a key-frame cloud (pcl::StatisticalOutlierRemoval as reference src/mapper.cpp:137-146 sets it up: meanK 30, stddev
 * multiplier 1.0; commented out there): a point's value is the mean distance to its mean_k nearest neighbours, and a point stays when that is at most
 * mean + stddev_mul * stddev over the cloud.  DESIGN.md s.15 is the contract; include/ssm/sor_core.h the arithmetic shared by the device path and the host
 * function.  The neighbours are exact (a ladder of uniform grids, cell = its first cell size, 0: automatic -- a tuning parameter that changes no output);
 * mean and stddev come from exact integer sums on a 2^-20 m grid.  Non-finite points are dropped; with fewer than mean_k + 1 finite points nothing else is
 * (too_few).  The output keeps the input order and a kept point's 32 bytes.  1 <= mean_k <= 64. */
typedef struct { int32_t mean_k; float cell; double stddev_mul; } ssm_sor_params;
typedef struct { int32_t n_in, n_finite, n_kept, too_few, levels, pad; uint64_t sum_q, sum_q2_lo, sum_q2_hi; double mean, stddev, threshold; } ssm_sor_info;
void ssm_sor_params_default(ssm_sor_params* p);                          /* 30, 0 (automatic), 1.0 */
int  ssm_sor_chunk(void);                                                /* candidates per LDS chunk of the device search: the tests build a case around it */
/* host arrays in and out; *n_out is the number kept (SSM_E_CAPACITY when cap is smaller: nothing written); info may be NULL.  SSM_E_INVAL: mean_k outside
 * 1..64, a negative or non-finite cell, a non-finite stddev_mul, or a mean distance of 4096 m or more (off the statistics grid) */
int  ssm_sor_filter(ssm_ctx* ctx, const ssm_point* pts, int n, const ssm_sor_params* params, ssm_point* out, int cap, int* n_out, ssm_sor_info* info);
/* the same on the CPU, the same bits; needs no GPU.  mean_dist (n floats: the point's value, 0 where it has none) and keep (n bytes) may each be NULL */
int  ssm_sor_filter_host(const ssm_point* pts, int n, const ssm_sor_params* params, ssm_point* out, int cap, int* n_out, ssm_sor_info* info,
                         float* mean_dist, uint8_t* keep);
/* the two arrays of the context's last device call (ssm_sor_filter or ssm_cloud_sor) over n points; each may be NULL */
int  ssm_debug_sor_record(ssm_ctx* ctx, float* mean_dist, uint8_t* keep, int n);
/* the ladder of the context's last device call: queries[l] = the points still unsettled when level l began (at most cap entries are written), *n_levels = info.levels.
 * For scripts/sor_bench.py */
int  ssm_debug_sor_levels(ssm_ctx* ctx, int32_t* queries, int cap, int* n_levels);
/* the device-resident form: the cloud is filtered where it lives and shrinks in place (its memory is a piece of a slab that later clouds follow, so there
 * is nothing to hand back); ssm_cloud_size is n_kept afterwards */
int  ssm_cloud_sor(ssm_ctx* ctx, ssm_cloud* cloud, const ssm_sor_params* params, ssm_sor_info* info);

/* ---- free-space carving: a LATER key-frame's depth image (the view) judges the points of earlier key-frames' camera-frame clouds, and a point the view has
 * seen through `min_votes` times in a row leaves its cloud.  The reference has no such step; DESIGN.md s.16 is the contract, include/ssm/carve_core.h the
 * arithmetic shared by the device path and the host function.  A point is carried into the view's frame by T_rel = inverse(T_view) . T_cloud (4x4, column-major
 * doubles as elsewhere in this header), projected to the nearest pixel and compared, in integer depth units, with the (2 radius + 1)^2 window around it:
 * verdict 0 UNKNOWN (non-finite, nearer than z_min, window not inside the image or holding a zero depth), 1 OCCLUDED, 2 SUPPORTED (within tol of the centre
 * depth), 3 SEEN_THROUGH (nearer than the window's minimum by more than tol); tol = tol_abs + depth * tol_rel_ppm / 10^6.  Every point has a run counter
 * (uint8, zero when the cloud is made): SEEN_THROUGH adds one (up to 255), SUPPORTED clears it, the others leave it; afterwards a point whose counter is at
 * least min_votes is removed.  The rest keep their order, their 32 bytes and their counters.
 * SSM_E_INVAL: min_votes outside 1..255, radius outside 0..3, tol_abs outside 0..10^6 or non-finite, tol_rel_ppm outside 0..10^6, z_min negative or
 * non-finite, a camera whose fx, fy, cx, cy are not finite or whose scale is outside (0, 10^6], a non-finite pose. */
typedef struct { int32_t min_votes, radius; double tol_abs; int32_t tol_rel_ppm, pad; double z_min; } ssm_carve_params;
typedef struct { int32_t n_in, n_kept, unknown, occluded, supported, seen_through, removed, pad; } ssm_carve_info;
typedef struct ssm_carve_view ssm_carve_view;
void ssm_carve_params_default(ssm_carve_params* p);                      /* 2, 1, 0.05 m, 20000 ppm, 0.1 m */
/* a view: the depth image goes to device memory and stays there until ssm_carve_view_free */
int  ssm_carve_view_create(ssm_ctx* ctx, const uint16_t* depth_host, int w, int h, const ssm_camera* cam, ssm_carve_view** view_out);
void ssm_carve_view_free(ssm_ctx* ctx, ssm_carve_view* view);
/* the pipeline's form: one view against m device-resident clouds (T_clouds: m poses of 16 doubles) in one launch sequence and one wait.  The clouds shrink in
 * place (ssm_cloud_size is the kept count afterwards) and their counters live with them; a cloud of size 0 is legal, the same cloud twice is not.  infos: m
 * entries, may be NULL.  A cloud that has counters is refused by ssm_cloud_sor (SSM_E_INVAL): filter first, carve afterwards. */
int  ssm_carve(ssm_ctx* ctx, const ssm_carve_view* view, const double* T_view, ssm_cloud* const* clouds, const double* T_clouds, int m,
               const ssm_carve_params* params, ssm_carve_info* infos);
/* host arrays through the device: run_inout holds the n counters before and the *n_out kept counters after (NULL: all zero, none returned); *n_out is the number
 * kept (SSM_E_CAPACITY when cap is smaller: nothing written, run_inout untouched); info may be NULL */
int  ssm_carve_points(ssm_ctx* ctx, const uint16_t* depth, int w, int h, const ssm_camera* cam, const double* T_view, const ssm_point* pts, int n,
                      const double* T_cloud, uint8_t* run_inout, const ssm_carve_params* params, ssm_point* out, int cap, int* n_out, ssm_carve_info* info);
/* the same on the CPU, the same bits; needs no GPU.  verdict and run (n bytes each: every point's verdict and its counter BEFORE the compaction) may be NULL */
int  ssm_carve_host(const uint16_t* depth, int w, int h, const ssm_camera* cam, const double* T_view, const ssm_point* pts, int n, const double* T_cloud,
                    uint8_t* run_inout, const ssm_carve_params* params, ssm_point* out, int cap, int* n_out, ssm_carve_info* info, uint8_t* verdict, uint8_t* run);
/* the same two arrays for cloud k of the context's last device call (ssm_carve: k < m; ssm_carve_points: k = 0) over its n points; each may be NULL */
int  ssm_debug_carve_record(ssm_ctx* ctx, int k, uint8_t* verdict, uint8_t* run, int n);
/* the counters of a device-resident cloud (all zero before its first ssm_carve): cap >= ssm_cloud_size entries */
int  ssm_cloud_run_fetch(ssm_ctx* ctx, const ssm_cloud* cloud, uint8_t* run, int cap);

/* ---- map rendering: the points of m posed clouds are splatted, z-buffered, into a pinhole view (w x h, a camera, T_view), and the rendering is compared per
 * pixel with a key-frame's own depth and semantic image.  The reference has no such step; DESIGN.md s.17 is the contract, include/ssm/render_core.h the
 * arithmetic shared by the device path and the host functions.  A point is carried into the view's frame by T_rel = inverse(T_view) . T_cloud, projected to the
 * nearest pixel, its depth quantised to depth units (1..65535, else invisible); it covers the (2 s + 1)^2 pixels around its centre that lie inside the image,
 * s = min(max_radius, floor(0.5 fx point_size / z)) (point_size 0: one pixel).  Every pixel keeps the smallest key (depth << 32 | index of the point in the
 * concatenation of the clouds): the nearest point, at equal depth the lowest index, whatever the order of processing.  Per pixel: depth (0 = empty), the winner's
 * b g r (0), the low byte of its label (255) and its index (-1).
 * The comparison classifies each pixel: 0 unrendered, 1 the frame has no depth, 2 the map in front of the measured surface, 3 behind it, 4 agree (within
 * tol = llrint(tol_abs scale) + d tol_rel_ppm / 10^6, carving's tolerance); the agreeing pixels by label: equal and known, both known and different, else unknown.
 * SSM_E_INVAL: max_radius outside 0..8; point_size, z_min, z_max or tol_abs negative or non-finite (z_max: 1e9 is "no limit"); tolerance and camera limits as
 * carving's; a non-finite pose; w or h < 1 or w h > 2^26; m < 0; 2^32 points or more in all. */
typedef struct { double point_size; int32_t max_radius; int32_t pad; double z_min, z_max; double tol_abs; int32_t tol_rel_ppm; int32_t pad2; } ssm_render_params;
typedef struct { int32_t n_in, n_visible, n_covered, pad; } ssm_render_info;      /* points given, points with a non-empty footprint, non-empty pixels */
typedef struct { int64_t unrendered, no_depth, in_front, behind, agree, label_agree, label_disagree, label_unknown, n_pixels; } ssm_render_compare_info;
typedef struct ssm_render_target ssm_render_target;
void ssm_render_params_default(ssm_render_params* p);                    /* 0 m, 3 px, 0.1 m, 1e9 m, 0.05 m, 20000 ppm */
/* the device z-buffer and the four output images of a w x h view, reused across calls */
int  ssm_render_target_create(ssm_ctx* ctx, int w, int h, ssm_render_target** target_out);
void ssm_render_target_free(ssm_ctx* ctx, ssm_render_target* target);
/* host arrays through the device: pts[k] holds n[k] points of cloud k, T_clouds m poses of 16 doubles.  info may be NULL */
int  ssm_render_points(ssm_ctx* ctx, ssm_render_target* target, const ssm_camera* cam, const double* T_view, const ssm_point* const* pts, const int32_t* n,
                       const double* T_clouds, int m, const ssm_render_params* params, ssm_render_info* info);
/* device-resident clouds: nothing is uploaded but the poses.  A cloud of size 0 is legal */
int  ssm_render_clouds(ssm_ctx* ctx, ssm_render_target* target, const ssm_camera* cam, const double* T_view, ssm_cloud* const* clouds, const double* T_clouds, int m,
                       const ssm_render_params* params, ssm_render_info* info);
/* the map the last ssm_viewer_map_update left on the device, at the identity pose; SSM_E_INVAL when there is none (no update yet, an empty map, or released) */
int  ssm_render_viewer_map(ssm_ctx* ctx, ssm_render_target* target, const ssm_camera* cam, const double* T_view, const ssm_render_params* params, ssm_render_info* info);
/* the images of the target's last rendering: depth w h uint16, bgr w h 3 bytes, label w h bytes, index w h int32; each may be NULL */
int  ssm_render_fetch(ssm_ctx* ctx, const ssm_render_target* target, uint16_t* depth, uint8_t* bgr, uint8_t* label, int32_t* index);
/* the target's last rendering against a frame (host images of the target's size; cam_scale: depth units per metre of both): uploads the frame and compares on the
 * device.  class_img (w h bytes) may be NULL */
int  ssm_render_compare(ssm_ctx* ctx, ssm_render_target* target, const uint16_t* depth_host, const uint8_t* sem_bgr_host, double cam_scale,
                        const ssm_render_params* params, ssm_render_compare_info* info, uint8_t* class_img);
/* the same on the CPU, the same bits; need no GPU.  Every output pointer may be NULL; keys: the raw z-buffer, w h entries (all ones = empty) */
int  ssm_render_host(int w, int h, const ssm_camera* cam, const double* T_view, const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m,
                     const ssm_render_params* params, uint16_t* depth, uint8_t* bgr, uint8_t* label, int32_t* index, uint64_t* keys, ssm_render_info* info);
int  ssm_render_compare_host(const uint16_t* rendered_depth, const uint8_t* rendered_label, int w, int h, const uint16_t* depth, const uint8_t* sem_bgr, double cam_scale,
                             const ssm_render_params* params, ssm_render_compare_info* info, uint8_t* class_img);
/* label image -> BGR through the 12-class palette (255 and any other value: black); n pixels, out 3 n bytes */
void ssm_render_label_colours(const uint8_t* label, int64_t n, uint8_t* bgr_out);
/* the raw z-buffer after the target's last rendering (w h entries), for the tests */
int  ssm_debug_render_keys(ssm_ctx* ctx, const ssm_render_target* target, uint64_t* keys);

/* ---- ground grid: the points of m posed clouds are dropped into a horizontal grid of nx x ny square cells (a bird's-eye semantic elevation map).  The reference
 * has no such step; DESIGN.md s.19 is the contract, include/ssm/grid_core.h the arithmetic shared by the device path and the host function (device == host byte
 * for byte, every raw accumulator included; integer accumulators only, so the order of points and clouds does not matter).  G: row-major 3 x 4, world -> grid
 * frame (grid x, y span the plane, grid z is height).  A point is used when it is finite, its height lies in [h_min, h_max] and its cell is inside.  Pass A: per
 * cell n, hmin, hmax (heights in units of 2^-10 m).  Ground: base = the smallest hmin of the non-empty cells of the (2 ground_radius + 1)^2 window.  Pass B: a
 * point at most step above base is LOW (n_low, sum_low, hist_low[label]), otherwise HIGH (n_high, hist_high[label]); a label above 11 enters no bin.  Resolve:
 * class 0 unobserved (heights INT32_MIN, labels 255), 4 obstacle (n_high >= min_obstacle_points), else by the ground label 1 drivable (Road 4, Road_marking 3),
 * 2 walkable (Pavement 5), 3 other ground; ground_q = floor(sum_low / n_low) (base when n_low == 0), top_q = hmax; the labels are the fullest bins, the lowest id
 * on a tie, 255 when empty (obstacle_label: 255 unless the cell is an obstacle).
 * SSM_E_INVAL: a non-finite entry of G or parameter; cell <= 0; nx or ny < 1, nx ny > 2^24 or above the target's cells; h_max < h_min, |h_min| or |h_max| above
 * 2^20; step < 0; ground_radius outside 0..4; min_obstacle_points < 1; a non-finite pose; m < 0, a negative count, the same cloud twice; 2^31 points or more. */
typedef struct { double G[12]; double x0, y0, cell; int32_t nx, ny; double h_min, h_max, step; int32_t ground_radius, min_obstacle_points; } ssm_grid_params;
typedef struct { int64_t n_in, n_finite, out_of_band, outside, n_used, unobserved, drivable, walkable, other_ground, obstacle; } ssm_grid_info;   /* points, then cells by class */
/* a cell's raw accumulators (128 bytes).  A cell no point fell into: hmin and base INT32_MAX, hmax INT32_MIN, everything else 0 */
typedef struct { uint32_t n; int32_t hmin, hmax, base; uint32_t n_low, n_high; int64_t sum_low; uint32_t hist_low[12], hist_high[12]; } ssm_grid_cell;
typedef struct ssm_grid_target ssm_grid_target;
/* G for a y-down, z-forward world (g.x = x, g.y = z, g.z = -y), 0.2 m cells, 512 x 512 of them centred in x and starting 10 m behind the origin, heights -3 .. +3 m,
 * step 0.3 m, ground_radius 1, min_obstacle_points 3 */
void ssm_grid_params_default(ssm_grid_params* p);
/* G (translation 0) for a world whose up and forward directions are given; SSM_E_INVAL: a non-finite entry, an up of length 0, a forward along up */
int  ssm_grid_frame_from_up(const double up[3], const double forward[3], double G[12]);
/* device accumulators and outputs for grids of up to nx ny cells, reused across builds (every build clears them) */
int  ssm_grid_target_create(ssm_ctx* ctx, int nx, int ny, ssm_grid_target** target_out);
void ssm_grid_target_free(ssm_ctx* ctx, ssm_grid_target* target);
/* m device-resident clouds at the poses T_clouds (m x 16 doubles, column-major); nothing is uploaded but the poses.  params NULL: the defaults; info may be NULL */
int  ssm_grid_clouds(ssm_ctx* ctx, ssm_grid_target* target, ssm_cloud* const* clouds, const double* T_clouds, int m, const ssm_grid_params* params, ssm_grid_info* info);
/* the same from host arrays, through the device */
int  ssm_grid_points(ssm_ctx* ctx, ssm_grid_target* target, const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m, const ssm_grid_params* params,
                     ssm_grid_info* info);
/* the map the last ssm_viewer_map_update left on the device, at the identity pose; SSM_E_INVAL when there is none */
int  ssm_grid_viewer_map(ssm_ctx* ctx, ssm_grid_target* target, const ssm_grid_params* params, ssm_grid_info* info);
/* the arrays of the target's last build, nx ny entries each, cell (cx, cy) at cy nx + cx; each may be NULL */
int  ssm_grid_fetch(ssm_ctx* ctx, const ssm_grid_target* target, uint8_t* cls, uint8_t* ground_label, uint8_t* obstacle_label, int32_t* ground_q, int32_t* top_q,
                    uint32_t* n, uint32_t* n_high);
/* the same on the CPU, no GPU, the same bits; cells (may be NULL): the raw accumulators */
int  ssm_grid_host(const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m, const ssm_grid_params* params, uint8_t* cls, uint8_t* ground_label,
                   uint8_t* obstacle_label, int32_t* ground_q, int32_t* top_q, uint32_t* n_out, uint32_t* n_high, ssm_grid_cell* cells, ssm_grid_info* info);
/* the raw cells after the target's last build (nx ny entries), for the tests */
int  ssm_debug_grid_cells(ssm_ctx* ctx, const ssm_grid_target* target, ssm_grid_cell* cells);
/* how the context's later builds accumulate, for the tests and the measurement: 0 one atomic per point and address, 1 one per run of adjacent lanes with the same
 * destination, -1 the default (1); the same bits either way */
int  ssm_debug_grid_form(ssm_ctx* ctx, int form);
/* the cell arrays as images whose row r is cell row ny - 1 - r (forward is up).  bgr (3 bytes per cell, may be NULL): an obstacle takes the palette colour of its
 * label, white when unknown; ground that of its label, (64, 64, 64) when unknown; unobserved is black.  height (16 bits per cell, may be NULL):
 * clamp(ground_q - llrint(1024 h_min), 0, 65534) + 1, 0 for unobserved */
void ssm_grid_colours(const uint8_t* cls, const uint8_t* ground_label, const uint8_t* obstacle_label, const int32_t* ground_q, int nx, int ny, double h_min,
                      uint8_t* bgr_out, uint16_t* height_out);

/* ---- object extraction: labelled obstacle instances from a built ground grid.  The reference has no such step; DESIGN.md s.21 is the contract,
 * include/ssm/objects_core.h the arithmetic shared by the device path and the host functions (device == host byte for byte; integers only).
 * Stage 1, cells: a cell is a MEMBER when its class is obstacle (4), its obstacle_label is below 12 and bit obstacle_label of label_mask is set.  Two members are
 * joined when they are adjacent under `connectivity` (4 or 8) and have the same obstacle_label; a COMPONENT is a class of the closure, its root its smallest cell
 * index cy nx + cx.  A component is KEPT when cells >= min_cells, cell_points (the sum of its cells' n_high) >= min_points and top_q - ground_q (the largest top_q
 * and the smallest ground_q of its cells) >= llrint(1024 min_height); the info counts the first rule that fails, in that order.  The kept components are the
 * objects 0 .. K - 1 in ascending root order; object_id (int32 per cell) is the object of a kept component's cells and -1 everywhere else.
 * Stage 2, points: a point of the grid's clouds is a point of object k when the grid used it, it is HIGH in its cell and its cell's object_id is k.  Per object
 * the count, those whose own label is the object's (n_label), the box and the sums of the quantised grid coordinates (units of 2^-10 m).  Before stage 2 the
 * minima are INT32_MAX, the maxima INT32_MIN, counts and sums 0.
 * SSM_E_INVAL: a null argument; a target of another context; a grid target never built or an object target smaller than the grid; connectivity other than 4 or 8;
 * negative min_cells or min_points; a negative or non-finite min_height; a grid whose extent leaves +-2^20 m; stage 2 before stage 1, after the grid target was
 * built again, or with a total point count other than that build's; the same cloud twice; 2^31 points or more. */
typedef struct { uint32_t label_mask; int32_t connectivity, min_cells, min_points; double min_height; } ssm_objects_params;
typedef struct { int64_t member_cells, components, kept, rejected_cells, rejected_points, rejected_height, n_in, object_points; } ssm_objects_info;   /* the last two: stage 2 */
typedef struct {
    int32_t root, label; uint32_t cells, n_points; uint64_t cell_points; int32_t cx_min, cx_max, cy_min, cy_max; int32_t ground_q, top_q;
    int32_t x_min_q, x_max_q, y_min_q, y_max_q, z_min_q, z_max_q; uint32_t n_label, pad; int64_t sum_x, sum_y, sum_z;
} ssm_object;                                                               /* 104 bytes */
typedef struct ssm_objects_target ssm_objects_target;
/* label_mask: Vehicle, Pedestrian, Bike (bits 9, 10, 11); connectivity 8; min_cells 2; min_points 20; min_height 0.3 m */
void ssm_objects_params_default(ssm_objects_params* p);
/* device labels, records and the object_id image for grids of up to nx ny cells, reused across calls */
int  ssm_objects_target_create(ssm_ctx* ctx, int nx, int ny, ssm_objects_target** target_out);
void ssm_objects_target_free(ssm_ctx* ctx, ssm_objects_target* target);
/* stage 1 on the grid target's last build; nothing is uploaded.  params NULL: the defaults; info may be NULL */
int  ssm_objects_grid(ssm_ctx* ctx, const ssm_grid_target* grid, const ssm_objects_params* params, ssm_objects_target* target, ssm_objects_info* info);
/* stage 2 on the device clouds the grid was built from, at the same poses, under the grid build's parameters */
int  ssm_objects_clouds(ssm_ctx* ctx, const ssm_grid_target* grid, ssm_objects_target* target, ssm_cloud* const* clouds, const double* T_clouds, int m, ssm_objects_info* info);
/* the same from host arrays, through the device; ids_out (may be NULL): one int32 per point of the concatenation, its object or -1 */
int  ssm_objects_points(ssm_ctx* ctx, const ssm_grid_target* grid, ssm_objects_target* target, const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m,
                        int32_t* ids_out, ssm_objects_info* info);
/* the same on the map the last ssm_viewer_map_update left on the device, at the identity pose */
int  ssm_objects_viewer_map(ssm_ctx* ctx, const ssm_grid_target* grid, ssm_objects_target* target, ssm_objects_info* info);
/* the K records of the target's last stage 1 (with the point figures of its last stage 2) and the object_id image (nx ny entries); either may be NULL.  cap < K:
 * SSM_E_CAPACITY, *n_out = K and nothing else written */
int  ssm_objects_fetch(ssm_ctx* ctx, const ssm_objects_target* target, ssm_object* out, int cap, int* n_out, int32_t* object_id);
/* stage 1 on the CPU, no GPU, the same bits, from the arrays ssm_grid_fetch / ssm_grid_host give */
int  ssm_objects_cells_host(const uint8_t* cls, const uint8_t* obstacle_label, const int32_t* ground_q, const int32_t* top_q, const uint32_t* n_high, int nx, int ny,
                            const ssm_objects_params* params, ssm_object* out, int cap, int* n_out, int32_t* object_id, ssm_objects_info* info);
/* ssm_grid_host, then both stages, on the CPU: the same bits as the device chain.  object_id (nx ny entries) and ids_out (one per point) may be NULL */
int  ssm_objects_host(const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m, const ssm_grid_params* grid_params, const ssm_objects_params* params,
                      ssm_object* out, int cap, int* n_out, int32_t* object_id, int32_t* ids_out, ssm_objects_info* info);
/* for the tests: hand-made cell arrays (nx ny entries each) uploaded and stage 1 run on them, so that the labelling can be tested at any shape without clouds
 * (stage 2 is refused after it).  SSM_E_INVAL also when the n_high sum to 2^31 or more: no built grid does */
int  ssm_debug_objects_cells(ssm_ctx* ctx, ssm_objects_target* target, const uint8_t* cls, const uint8_t* obstacle_label, const int32_t* ground_q, const int32_t* top_q,
                             const uint32_t* n_high, int nx, int ny, const ssm_objects_params* params, ssm_objects_info* info);
/* how the context's later stage-2 calls accumulate: 0 one atomic per point and figure, 1 one per run of adjacent lanes with the same object, -1 the default; the
 * same bits either way */
int  ssm_debug_objects_form(ssm_ctx* ctx, int form);
/* the per-point object ids of the context's last stage-2 call (n: that call's point count) */
int  ssm_debug_objects_point_ids(ssm_ctx* ctx, int32_t* out, int64_t n);
/* the labelling's tile, for the tests */
int  ssm_debug_objects_tile_w(void);
int  ssm_debug_objects_tile_h(void);

/* ---- clearance map: obstacle distance and reachable free space of a built ground grid.  The reference has no such step; DESIGN.md s.22 is the contract,
 * include/ssm/clearance_core.h the arithmetic shared by the device path and the host function (device == host byte for byte; integers only).
 * Input: the class image cls of a grid (nx x ny, cell (cx, cy) at cy nx + cx; nx, ny <= 32768).  A cell is BLOCKED when bit cls of blocked_mask is set.
 * dist2 (uint32) and nearest (int32) are the minimum over ALL blocked cells b of the key (d2(c, b) << 24) | index(b): dist2 the exact squared Euclidean distance
 * in cells (0 on a blocked cell), nearest the index of the blocked cell that attains it, the lowest index among equals; no blocked cell at all: UINT32_MAX and -1.
 * A cell is TRAVERSABLE when bit cls of free_mask is set and dist2 > r2 = floor((radius / cell)^2) (saturated at 2^31).  The SEED is the traversable cell with the
 * smallest key (d2 to (seed_cx, seed_cy) << 24) | index among those with d2 <= seed_snap^2, or none.  reach (uint8): 2 in the seed's connected component of
 * traversable cells (under `connectivity`), 1 on every other traversable cell, 0 elsewhere; without a seed every traversable cell is 1.
 * SSM_E_INVAL: a null argument; mask bits above class 4; masks that overlap; connectivity other than 4 or 8; a negative or non-finite radius; a cell size that
 * is not positive and finite; seed_snap outside 0 .. 1024; a seed outside the grid other than (-1, -1); a side above 32768 or more than 2^24 cells; a target
 * smaller than the grid or of another context; a grid target never built. */
typedef struct {
    uint32_t blocked_mask, free_mask;        /* bits over the cell classes 0 .. 4 */
    int32_t connectivity, seed_cx, seed_cy, seed_snap;
    double radius;                           /* metres */
    double cell;                             /* metres per cell of a hand-made class image (ssm_clearance_cells_host, ssm_debug_clearance_cells); ssm_clearance_grid takes the grid's */
} ssm_clearance_params;
typedef struct { int64_t blocked, free_cells, traversable, components, reachable, seed_cell, max_d2_reachable, r2; } ssm_clearance_info;
typedef struct ssm_clearance_target ssm_clearance_target;
/* blocked_mask: OBSTACLE (bit 4); free_mask: DRIVABLE (bit 1); radius 1.0 m; connectivity 4; no seed (-1, -1); seed_snap 10; cell 1.0 */
void ssm_clearance_params_default(ssm_clearance_params* p);
/* device arrays for grids of up to nx ny cells, reused across calls */
int  ssm_clearance_target_create(ssm_ctx* ctx, int nx, int ny, ssm_clearance_target** target_out);
void ssm_clearance_target_free(ssm_ctx* ctx, ssm_clearance_target* target);
/* the stage on the grid target's last build; nothing is uploaded, one download (the info).  params NULL: the defaults; info may be NULL */
int  ssm_clearance_grid(ssm_ctx* ctx, const ssm_grid_target* grid, const ssm_clearance_params* params, ssm_clearance_target* target, ssm_clearance_info* info);
/* the images of the target's last call (nx ny entries each); each pointer may be NULL */
int  ssm_clearance_fetch(ssm_ctx* ctx, const ssm_clearance_target* target, uint32_t* dist2, int32_t* nearest, uint8_t* reach);
/* the stage on the CPU, no GPU, the same bits: a column pass, then the lower envelope of every row's parabolas, then a flood fill.  Each output may be NULL */
int  ssm_clearance_cells_host(const uint8_t* cls, int nx, int ny, const ssm_clearance_params* params, uint32_t* dist2, int32_t* nearest, uint8_t* reach, ssm_clearance_info* info);
/* for the tests: a hand-made class image uploaded and the stage run on it */
int  ssm_debug_clearance_cells(ssm_ctx* ctx, ssm_clearance_target* target, const uint8_t* cls, int nx, int ny, const ssm_clearance_params* params, ssm_clearance_info* info);
/* the row pass of the context's later calls: 0 the whole row staged through LDS in chunks, 1 an outward scan that stops at the best distance, -1 the default; the
 * same bits either way */
int  ssm_debug_clearance_form(ssm_ctx* ctx, int form);
/* the staging width of row-pass form 0, for the tests */
int  ssm_debug_clearance_chunk(void);

/* ---- route field: the cheapest paths over a clearance map.  The reference has no such step; DESIGN.md s.23 is the contract, include/ssm/route_core.h the
 * arithmetic shared by the device path and the host functions (device == host byte for byte; integers only).
 * Input: the last result of a clearance target -- reach, dist2 and the seed cell.  Only cells with reach == 2 take part; the SOURCE is the seed cell.  A cell
 * weighs 1 + near_weight when dist2 <= comfort2 = floor((comfort / cell)^2) (saturated at 2^31), else 1.  The axial moves have step 5, with moves == 8 the diagonal
 * ones step 7, and a diagonal move exists only when both cells that share an edge with its two ends take part as well (no corner is cut).  An edge costs
 * step (w(a) + w(b)).  cost (uint32): the minimum over all paths from the source of the sum of the edges, 0 at the source, UINT32_MAX where no path leads.
 * parent (int32): for a routed cell other than the source the neighbour p with the smallest key ((cost(p) + edge(p, c)) << 24) | index(p), -1 at the source and
 * on unrouted cells.  Without a seed the call succeeds and routes nothing.
 * A path query snaps the goal to the routed cell with the smallest key (d2 << 24) | index within goal_snap cells (the clearance seed's rule) and writes the cells
 * from the source to that cell.  No such cell: len 0, goal_cell -1, cost -1, min_d2 -1.  A path longer than the target's max_path: SSM_E_CAPACITY, the path info
 * filled (len: the length needed), no cell written.
 * SSM_E_INVAL: a null argument; moves other than 4 or 8; near_weight outside 0 .. 8; a negative or non-finite comfort; a cell size that is not positive and
 * finite; goal_snap outside 0 .. 1024; a goal outside the grid; a side above 32768 or more than 2^24 cells; a source that is neither -1 nor a cell with
 * reach == 2; a target smaller than the grid or of another context; max_path < 1; a clearance target never run; a path query before a field. */
typedef struct {
    int32_t moves, near_weight;
    double comfort;                          /* metres */
    double cell;                             /* metres per cell of hand-made inputs (the host functions, ssm_debug_route_cells); ssm_route_field takes the clearance call's */
} ssm_route_params;
/* near_cells: routed cells with dist2 <= comfort2 (whatever near_weight); far_cell: the routed cell of largest cost, the lowest index among equals */
typedef struct { int64_t routed, unrouted, near_cells, max_cost, far_cell, source_cell, comfort2, moves; } ssm_route_info;
/* near_steps: cells of the path with dist2 <= comfort2; min_d2: the smallest dist2 on the path */
typedef struct { int64_t len, goal_cell, cost, n_axial, n_diag, near_steps, min_d2; } ssm_route_path_info;
typedef struct ssm_route_target ssm_route_target;
/* moves 8; near_weight 2; comfort 2.0 m; cell 1.0 */
void ssm_route_params_default(ssm_route_params* p);
/* device arrays for grids of up to nx ny cells and paths of up to max_path cells, reused across calls */
int  ssm_route_target_create(ssm_ctx* ctx, int nx, int ny, int max_path, ssm_route_target** target_out);
void ssm_route_target_free(ssm_ctx* ctx, ssm_route_target* target);
/* the field over the clearance target's last result; nothing is uploaded.  The route target keeps what a path query needs: the clearance target may be run again
 * or freed afterwards.  params NULL: the defaults; info may be NULL */
int  ssm_route_field(ssm_ctx* ctx, const ssm_clearance_target* clearance, const ssm_route_params* params, ssm_route_target* target, ssm_route_info* info);
/* a path of the target's field: cells_out has room for the target's max_path indices (cy nx + cx), source first */
int  ssm_route_path(ssm_ctx* ctx, ssm_route_target* target, int goal_cx, int goal_cy, int goal_snap, int32_t* cells_out, ssm_route_path_info* path_info);
/* the images of the target's field (nx ny entries each); each pointer may be NULL */
int  ssm_route_fetch(ssm_ctx* ctx, const ssm_route_target* target, uint32_t* cost, int32_t* parent);
/* the field on the CPU, no GPU, the same bits: Dijkstra with a circular bucket queue.  source_cell: an index or -1; each output may be NULL */
int  ssm_route_cells_host(const uint8_t* reach, const uint32_t* dist2, int nx, int ny, int source_cell, const ssm_route_params* params, uint32_t* cost, int32_t* parent,
                          ssm_route_info* info);
/* a path on the CPU from the arrays of a field (cost, parent) and the clearance map's dist2; cells_out (room for max_path indices) may be NULL: only the info */
int  ssm_route_path_host(const uint32_t* cost, const int32_t* parent, const uint32_t* dist2, int nx, int ny, const ssm_route_params* params, int goal_cx, int goal_cy, int goal_snap,
                         int max_path, int32_t* cells_out, ssm_route_path_info* path_info);
/* for the tests: hand-made reach and dist2 images uploaded and the stage run on them */
int  ssm_debug_route_cells(ssm_ctx* ctx, ssm_route_target* target, const uint8_t* reach, const uint32_t* dist2, int nx, int ny, int source_cell, const ssm_route_params* params,
                           ssm_route_info* info);
/* how the context's later fields relax: 0 sweeps of one thread per cell in batches, 1 tiles relaxed to their own fixed point from an active list, -1 the default;
 * the same bits either way */
int  ssm_debug_route_form(ssm_ctx* ctx, int form);
/* how many times the context's last field asked the device whether it was done (form 0: batches of sweeps, form 1: rounds of active tiles); a measurement, not
 * part of the contract */
int  ssm_debug_route_rounds(ssm_ctx* ctx);
/* the tile of form 1 and the sweeps per batch of form 0, for the tests */
int  ssm_debug_route_tile(void);
int  ssm_debug_route_batch(void);

/* ---- label fusion: the key-frames around a cloud (the views: depth image, label image, camera, world pose) vote on the label of each of its points, and a point
 * takes the label its views agree on.  The reference has no such step; DESIGN.md s.20 is the contract, include/ssm/relabel_core.h the arithmetic shared by the
 * device path and the host function (device == host bit for bit).  A view votes for a point with the label at the point's pixel when carving's verdict (s.16) is
 * SUPPORTED, that label is one of the palette's twelve and -- with edge_guard -- the whole (2 radius + 1)^2 window carries it.  The point's own label (unknown
 * above 11) counts own_weight.  The largest count wins, the own label on a tie, else the lowest id; the label changes when the winner differs and has at least
 * min_votes.  Only the 4 label bytes of a point are ever written.  At most 16 views per call.
 * SSM_E_INVAL: v outside 0..16, a null view or the same view twice, a view or cloud of another context, a non-finite pose or camera, a scale outside (0, 1e6],
 * radius outside 0..3, edge_guard outside 0..1, own_weight outside 0..15, min_votes outside 1..31, the tolerances and z_min outside carving's ranges */
typedef struct { int32_t radius, edge_guard, own_weight, min_votes; double tol_abs; int32_t tol_rel_ppm, pad; double z_min; } ssm_relabel_params;
/* n_supported, n_voted: points with at least one SUPPORTED / voting view; n_filled: the changed points whose label was unknown; pairs: (point, view) pairs */
typedef struct { int32_t n_in, n_supported, n_voted, n_changed, n_filled, pad; int64_t pairs_supported, pairs_voted; } ssm_relabel_info;
/* a view of the host function: label is the w x h image of ssm_relabel_labels_host */
typedef struct { const uint16_t* depth; const uint8_t* label; int32_t w, h; ssm_camera cam; } ssm_relabel_host_view;
typedef struct ssm_relabel_view ssm_relabel_view;
void ssm_relabel_params_default(ssm_relabel_params* p);                  /* 1, 1, 1, 2, 0.05 m, 20000 ppm, 0.1 m */
/* a view: the depth image is uploaded, the label image made on the device from the semantic BGR image (3 bytes per pixel, rows packed); both stay there until
 * ssm_relabel_view_free */
int  ssm_relabel_view_create(ssm_ctx* ctx, const uint16_t* depth_host, const uint8_t* sem_bgr_host, int w, int h, const ssm_camera* cam, ssm_relabel_view** view_out);
void ssm_relabel_view_free(ssm_ctx* ctx, ssm_relabel_view* view);
/* v views (T_views: v x 16 doubles, column-major world poses) on one device-resident cloud, relabelled in place; info may be NULL */
int  ssm_relabel(ssm_ctx* ctx, const ssm_relabel_view* const* views, const double* T_views, int v, ssm_cloud* cloud, const double* T_cloud,
                 const ssm_relabel_params* params, ssm_relabel_info* info);
/* the same on n host points through the device: label_out gets every point's label afterwards (n entries) */
int  ssm_relabel_points(ssm_ctx* ctx, const ssm_relabel_view* const* views, const double* T_views, int v, const ssm_point* pts, int n, const double* T_cloud,
                        const ssm_relabel_params* params, uint32_t* label_out, ssm_relabel_info* info);
/* the same on the CPU, no GPU.  votes_out (may be NULL): every point's twelve counts, 5 bits each, class l at bits 5 l .. 5 l + 4 */
int  ssm_relabel_host(const ssm_relabel_host_view* views, const double* T_views, int v, const ssm_point* pts, int n, const double* T_cloud,
                      const ssm_relabel_params* params, uint32_t* label_out, uint64_t* votes_out, ssm_relabel_info* info);
/* the label image of n semantic BGR pixels: the palette's class, 255 for any other colour */
int  ssm_relabel_labels_host(const uint8_t* sem_bgr, int64_t n, uint8_t* label_out);
/* the packed counts and the labels of the context's last device call over its n points; each may be NULL */
int  ssm_debug_relabel_record(ssm_ctx* ctx, uint64_t* votes, uint32_t* new_label, int n);
/* a view's label image (w h bytes) */
int  ssm_debug_relabel_view(ssm_ctx* ctx, const ssm_relabel_view* view, uint8_t* label_out);
/* how the context's later views are stored and read, for the tests and the measurement: 0 a depth and a label image, 1 one packed word per pixel (depth |
 * label << 16) that the vote gathers alone, 2 the same with the windows of two views in flight, -1 the default; the same bits either way.  A view votes only under the form it was made under */
int  ssm_debug_relabel_form(ssm_ctx* ctx, int form);

/* ---- dense alignment: projective point-to-plane ICP of the points of m posed clouds against a key-frame's depth image (the view).  The reference has no such
 * step; DESIGN.md s.18 is the contract, include/ssm/align_core.h the arithmetic shared by the device path and the host function.  The view gets a normal per
 * pixel (invalid at depth 0, at the border and across a depth edge: a neighbour farther than carving's tolerance).  Per iteration every point is carried into the
 * view's frame by E . inverse(T_view) . T_cloud (E: the increment, the identity at first), projected to the nearest pixel, and contributes its point-to-plane
 * residual r = n . (q - V) when the pixel is valid and |r| <= dist_max, Huber-weighted.  The sums are exact 64-bit integer sums of fixed-point terms, so the
 * result does not depend on the order of the points or clouds.  The 6 x 6 solve (damped: lambda = damping inliers) runs on the host.
 * status: 0 max_iterations reached, 1 converged (|omega| < eps_rot and |upsilon| < eps_trans), 2 fewer than min_inliers inliers, 3 a non-positive pivot,
 * 4 the accumulated increment left max_shift / max_angle.  With 2, 3 and 4 T_view_out = T_view and E = the identity; else T_view_out = T_view . inverse(E).
 * SSM_E_INVAL: max_iterations outside 1..64, stride outside 1..2^20, a negative or non-finite parameter, z_max < z_min, max_angle above pi, tolerance and camera
 * limits as carving's, w or h < 3 or w h > 2^26, a non-finite pose, m < 0, a negative count, the same cloud twice, or a point count whose sums could reach 2^62
 * (align_core.h term_bound_units, from z_max, dist_max and the camera's field of view). */
enum { SSM_ALIGN_MAX_ITER = 0, SSM_ALIGN_CONVERGED = 1, SSM_ALIGN_TOO_FEW = 2, SSM_ALIGN_DEGENERATE = 3, SSM_ALIGN_DIVERGED = 4, SSM_ALIGN_NSUM = 30 };
typedef struct {
    int32_t max_iterations, stride;          /* stride: every k-th point of each cloud is used */
    double z_min, z_max, dist_max, delta, damping, eps_rot, eps_trans;
    int32_t min_inliers, pad;
    double max_shift, max_angle;             /* bounds of the accumulated increment: metres, radians */
    double tol_abs; int32_t tol_rel_ppm, pad2;      /* the depth-edge gate of the view (read by ssm_align_view_create / ssm_align_host) */
} ssm_align_params;
typedef struct {
    int32_t status, iterations;              /* iterations: accumulations run */
    int64_t n_in;                            /* points used (after stride) */
    int64_t tested_first, inliers_first, tested_last, inliers_last;       /* tested: reached a valid pixel */
    double chi2_first, chi2_last;            /* the robustified sum of squared residuals, m^2 */
    double E[16];                            /* the increment, column-major 4 x 4 */
} ssm_align_info;
/* one iteration: 21 lower-triangle entries of H and 6 of b in units of 2^-20, chi2 in units of 2^-30, tested, inliers; E: the 3 x 4 row-major increment it used */
typedef struct { int64_t sums[SSM_ALIGN_NSUM]; double E[12]; } ssm_align_iter;
typedef struct ssm_align_view ssm_align_view;
/* 10, 1, 0.1 m, 80 m, 0.25 m, 0.05 m, 1e-6, 1e-4 rad, 1e-4 m, 1000, 1 m, 0.2 rad, 0.05 m, 20000 ppm */
void ssm_align_params_default(ssm_align_params* p);
/* a view: the depth image goes to device memory once, the normal map is built there, and both stay until ssm_align_view_free.  params: the edge gate (NULL: defaults) */
int  ssm_align_view_create(ssm_ctx* ctx, const uint16_t* depth_host, int w, int h, const ssm_camera* cam, const ssm_align_params* params, ssm_align_view** view_out);
void ssm_align_view_free(ssm_ctx* ctx, ssm_align_view* view);
/* device-resident clouds: nothing is uploaded but the poses and each iteration's E, nothing downloaded but the sums.  Clouds are not modified; size 0 is legal */
int  ssm_align_clouds(ssm_ctx* ctx, const ssm_align_view* view, const double* T_view, ssm_cloud* const* clouds, const double* T_clouds, int m,
                      const ssm_align_params* params, double* T_view_out, ssm_align_info* info);
/* host arrays through the device: pts[k] holds n[k] points of cloud k */
int  ssm_align_points(ssm_ctx* ctx, const ssm_align_view* view, const double* T_view, const ssm_point* const* pts, const int32_t* n, const double* T_clouds, int m,
                      const ssm_align_params* params, double* T_view_out, ssm_align_info* info);
/* the same on the CPU, the same bits; needs no GPU.  valid (w h bytes), normals (w h x 4 floats: x y z 0), record (record_cap entries, *n_record of them
 * written: one per iteration) may be NULL */
int  ssm_align_host(const uint16_t* depth, int w, int h, const ssm_camera* cam, const double* T_view, const ssm_point* const* pts, const int32_t* n,
                    const double* T_clouds, int m, const ssm_align_params* params, double* T_view_out, ssm_align_info* info, uint8_t* valid, float* normals,
                    ssm_align_iter* record, int record_cap, int* n_record);
/* the view's valid mask and normals as ssm_align_host gives them; each may be NULL */
int  ssm_debug_align_normals(ssm_ctx* ctx, const ssm_align_view* view, uint8_t* valid, float* normals);
/* the iterations of the context's last device alignment: *n_record of them (more than cap: SSM_E_CAPACITY) */
int  ssm_debug_align_record(ssm_ctx* ctx, ssm_align_iter* record, int cap, int* n_record);
/* points one pass of the accumulation's persistent grid covers (a larger call loops), for the tests */
int64_t ssm_debug_align_pass_points(void);

/* ---- PoseGraph's optimiser (reference src/pose_graph.cpp:82-305, include/pose_graph.h:53-62): a graph of SE3 vertices and SE3 edges with Huber kernels,
 * Levenberg (g2o's OptimizationAlgorithmLevenberg) over a direct block-envelope L D L^T.  DESIGN.md s.12 is the contract; include/ssm/pgo_core.h holds the
 * arithmetic, ONE function template that the host function runs with one thread and the device path with one 1024-thread block per graph, so device ==
 * host bit for bit.  Poses and measurements are 4 x 4 column-major isometries; an information matrix is its 21 upper-triangle entries row by row (the
 * order of a g2o file), NULL = 100 I (pose_graph.cpp's edges).  Vertices are named by caller ids; edges are numbered in the order they were added. */
enum { SSM_PGO_MAX_ITERS = 32, SSM_PGO_MAX_TRIALS = 10, SSM_PGO_PHASES = 5 };
typedef struct {
    int32_t iterations;                      /* iterations run */
    int32_t active_vertices, active_edges;   /* free vertices with an active edge; edges with a free vertex */
    int32_t solve_failures;                  /* trials whose factorisation met a pivot that is not > 0 */
    int64_t envelope_scalars;                /* doubles of the block envelope */
    double  lambda;                          /* after the last iteration */
    int32_t trials[SSM_PGO_MAX_ITERS];       /* per iteration */
    uint32_t accepted[SSM_PGO_MAX_ITERS];    /* bit t: trial t of the iteration was accepted */
    double  chi2_before[SSM_PGO_MAX_ITERS], chi2_after[SSM_PGO_MAX_ITERS];     /* the robustified active chi2 */
    double  gain[SSM_PGO_MAX_ITERS][SSM_PGO_MAX_TRIALS];
    int64_t clocks[SSM_PGO_PHASES];          /* device path: 100 MHz ticks per phase (ssm_pgo_times converts) */
} ssm_pgo_report;
typedef struct ssm_pgo ssm_pgo;
/* ctx may be NULL: an object for ssm_pgo_optimize_host and the host inspection calls only, which needs no GPU; its errors are in ssm_last_error(NULL) */
int  ssm_pgo_create(ssm_ctx* ctx, ssm_pgo** out);
void ssm_pgo_destroy(ssm_pgo* g);
int  ssm_pgo_clear(ssm_pgo* g);                                          /* no vertices, no edges; the memory stays */
int  ssm_pgo_add_vertex(ssm_pgo* g, int id, const double T[16], int fixed);     /* a duplicate id: SSM_E_INVAL */
/* an unknown id, from == to: SSM_E_INVAL.  Multi-edges are allowed */
int  ssm_pgo_add_edge(ssm_pgo* g, int id_from, int id_to, const double Z[16], const double* info21, int robust);
int  ssm_pgo_set_fixed(ssm_pgo* g, int id, int fixed);
/* mode 0 (pose_graph.cpp:242-246): every vertex free but the first added; mode 1 (:268-276): only the last five added free -- with fewer than six vertices
 * none, the reference's unsigned `i > size() - 6` */
int  ssm_pgo_set_mode(ssm_pgo* g, int local);
int  ssm_pgo_set_pose(ssm_pgo* g, int id, const double T[16]);
int  ssm_pgo_get_poses(const ssm_pgo* g, int32_t* ids, double* T, int cap, int* n_out);      /* insertion order; ids / T may be NULL */
int  ssm_pgo_size(const ssm_pgo* g, int* vertices, int* edges);
int  ssm_pgo_edge_chi2(const ssm_pgo* g, int edge, double* chi2);         /* the plain e^T Om e at the current estimate: what mainLoop accumulates */
/* the envelope (H and the factor, 16 bytes per scalar) may take at most this many bytes: beyond it ssm_pgo_optimize* return SSM_E_CAPACITY and leave the graph
 * as it was.  Default: a quarter of the device memory free at ssm_pgo_create, 1 GiB for a host-only object */
int  ssm_pgo_set_envelope_cap(ssm_pgo* g, size_t bytes);
/* optimize(iterations), 0 <= iterations <= SSM_PGO_MAX_ITERS: one launch, one wait (poses and report).  report may be NULL */
int  ssm_pgo_optimize(ssm_pgo* g, int iterations, ssm_pgo_report* report);
int  ssm_pgo_optimize_host(ssm_pgo* g, int iterations, ssm_pgo_report* report);           /* the same bits on the CPU; needs no GPU */
/* n graphs of ONE context as n blocks of one launch; reports: n entries or NULL */
int  ssm_pgo_optimize_many(ssm_pgo** graphs, int n, int iterations, ssm_pgo_report* reports);
/* the active set of the current graph: free vertices with an active edge, edges with a free vertex.  Plans only: the last report and times stay */
int  ssm_pgo_active(ssm_pgo* g, int* vertices, int* edges);
/* inspection, for the tests; device != 0: the device path.  Linearises the active edges at the current estimate: e / Ji / Jj: active edges x 6 / 36 / 36
 * (row-major; ascending edge number), w: their Huber weights, H: the assembled envelope (ssm_pgo_envelope's layout), b: 6 x active vertices.  Any may be NULL */
int  ssm_pgo_linearize(ssm_pgo* g, int device, double* e, double* Ji, double* Jj, double* w, double* H, double* b);
/* the envelope of the current active set: first[r] = the first block column of block row r (nr_out rows; row r holds the 6 x 6 (r - first[r] + 1) scalars of
 * its block columns first[r] .. r, scalar row by scalar row, rows in order; entries right of the diagonal are not read) */
int  ssm_pgo_envelope(ssm_pgo* g, int32_t* first, int cap, int* nr_out, int64_t* scalars_out);
/* solves (H + lambda I) x = b for a caller-given envelope: nr block rows with first[] (first[r] <= r).  *ok = 0: a pivot was not > 0 (x = 0) */
int  ssm_pgo_factor_solve(ssm_pgo* g, int device, int nr, const int32_t* first, const double* H, const double* b, double lambda, double* x, int* ok);
/* milliseconds of the last device call per phase: linearise, assemble, factor + solves, update + chi2, decide */
int  ssm_pgo_times(const ssm_pgo* g, double ms[SSM_PGO_PHASES]);
/* for the tests: one Levenberg decision by pnp_core.h's lm_update (scaled == 0) or by pgo_core.h's lm_update_scaled fed the same six-term sum (scaled != 0).
 * state: (lambda, nu) in / out; out: (gain, accepted) */
int  ssm_debug_pgo_lm_update(int scaled, double state[2], double chi, double chi_new, int solved, const double x[6], const double b[6], double out[2]);
/* VERTEX_SE3:QUAT id x y z qx qy qz qw / FIX id / EDGE_SE3:QUAT from to x y z qx qy qz qw + the 21 information entries, %.17g: what PoseGraph::save writes.
 * Any other tag: SSM_E_INVAL with the line number in ssm_last_error.  Loaded edges carry the robust flag `robust` */
int  ssm_pgo_save_g2o(const ssm_pgo* g, const char* path);
int  ssm_pgo_load_g2o(ssm_pgo* g, const char* path, int robust);

/* ---- device-resident batched stereo path (BASELINE.json configs[3]): n frames of a rectified stereo sequence, all DEVICE pointers.
 * The reference walks the KITTI sequence one frame at a time: FrameReader::next() computes the depth of the current pair with SGBM
 * (src/rgbdframe.cpp:64-116, src/stereo.cpp:11-30), Tracker::estimateVO builds a QuadFeatureMatch on (current left, current right, previous left,
 * previous right), runs detectFeature + circularMatching (src/track.cpp:45-59, src/quadmatcher.cpp:388-417,548-588) and hands the quad matches to
 * VisualOdometryStereo::Process (src/track.cpp:62, src/vo_stereo.cpp:18-152).  Frame pairs are independent of each other (the pose chain only
 * multiplies the per-frame motions), so this entry point runs those three stages for EVERY frame of the sequence in bulk: frame f is "current",
 * frame f - 1 "previous" (frame 0: the last frame of the previous call when continue_sequence = 1, else it has no quad matches: nquad = -1).
 * The per-pair entry points above (ssm_quad_track, ssm_gftt, ssm_lk_track, ssm_sgbm, ssm_stereo_depth) run the same kernels with one frame. */
enum { SSM_STEREO_QUAD = 1, SSM_STEREO_DEPTH = 2, SSM_STEREO_VO = 4 /* needs SSM_STEREO_QUAD */ };
typedef struct {
    const uint8_t* left;      /* n x h x w, 8-bit gray, packed */
    const uint8_t* right;     /* n x h x w */
    int n, w, h;
    int continue_sequence;    /* 1: frame 0's previous pair is the last frame of the previous call on this context (same w, h; a per-pair stereo call in between ends the sequence) */
    int stages;               /* bit mask of SSM_STEREO_*, 0 = all */
    int max_corners;          /* cv::goodFeaturesToTrack maxCorners; QuadFeatureMatch uses the OpenCV default 1000 */
    ssm_sgbm_params sgbm;     /* ssm_sgbm_params_default = src/stereo.cpp:16-27 */
    double baseline, cu, cv, f, roix, roiy, roiz, scale;      /* the depth conversion, as in ssm_stereo_depth */
    ssm_vo_params vo;
    int ransac_iters;         /* VisualOdometryStereo::parameters::ransac_iters (200) */
    /* n * ransac_iters * 3 RAW rand() outputs, in the order VisualOdometry::getRandomSample (src/vo.cpp:74-93) would draw them: the host class owns
     * the stream (srand(0) in its constructor).  A frame with >= 6 quad matches consumes 3 * ransac_iters draws (r % N, r % (N-1), r % (N-2) per
     * hypothesis), a frame with fewer consumes none (src/vo_stereo.cpp:61-63); *rand_draws_used of the output says how far the stream advanced. */
    const uint32_t* rand_stream;
} ssm_stereo_frames_dev;
typedef struct {              /* DEVICE pointers owned by the context, valid until the next ssm_stereo_seq_process / per-pair stereo call / destroy */
    const ssm_pmatch* quad;   /* n x max_corners: QuadFeatureMatch::quadmatches of frame f */
    const int32_t* nquad;     /* n ; -1 = frame without a previous frame */
    const float*   corners;   /* n x max_corners x 2: the GFTT corners of the current-left image (strength order) */
    const int32_t* ncorners;  /* n */
    const int16_t* disp;      /* n x h x w: cv::StereoSGBM output (x16 fixed point) */
    const uint16_t* depth;    /* n x h x w: FrameReader's depth image */
    const double*  tr;        /* n x 6: (rx, ry, rz, tx, ty, tz) as ssm_vo_estimate */
    const int32_t* inliers;   /* n x max_corners: consensus set in index order */
    const int32_t* vo_result; /* n x 2: {n_inliers, success} */
    const int32_t* rand_draws_used;   /* 1 int: draws of rand_stream consumed by this call */
    int max_corners;
} ssm_stereo_out_dev;
int ssm_stereo_seq_process(ssm_ctx* ctx, const ssm_stereo_frames_dev* in, ssm_stereo_out_dev* out);
/* frame pairs per launch of the stereo path: ssm_config.stereo_batch, else min(config max_batch, 128) (0.23 GB of SGBM workspace per pair in the default
   formulation -- three cost-volume-sized buffers at 1241 x 376 x 80 --, two workspaces; 128 per launch measured 1 % above 64) */
int ssm_stereo_batch(const ssm_ctx* ctx);

/* ---- Classifier (include/segnet.h:22-46, src/segnet.cpp): SegNet driving_webdemo forward, fp16 MFMA, on the device.
 * Topology is fixed (VGG-16 encoder / mirrored decoder, 26 conv3x3 layers, 12 classes, 480x360 net input); weights
 * are DATA: the .caffemodel is not in the reference tree (README.md:25-32), so the caller supplies every layer.
 * layer l: weight[Cout][Cin][3][3] fp32 (Caffe blob order), scale[Cout], shift[Cout] = conv bias + BatchNorm folded:
 * y = scale * conv(x) + shift, then ReLU for every layer but the last. */
int ssm_segnet_num_layers(void);
int ssm_segnet_layer_shape(int layer, int* cin, int* cout, int* h, int* w);
int ssm_segnet_set_layer(ssm_ctx* ctx, int layer, const float* weight, const float* scale, const float* shift);
/* Classifier::Classify on one host frame (any size equal to the context geometry): Preprocess (cv::resize to 480x360,
 * float, mean 0; segnet.cpp:130-167) -> forward -> ArgMax.  labels_net: 360*480 class ids (may be NULL).
 * sem_bgr (may be NULL): the colour-label image at FRAME size produced like experiment/segnet.cpp:80-83,131-146
 * (Pavement->Road remap, resize of the ids, LUT through the 12-colour palette). */
int ssm_segnet_forward(ssm_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, uint8_t* labels_net, uint8_t* sem_bgr);
/* n device frames (packed BGR); outputs are device buffers or NULL.  flags: bit0 = nearest-neighbour resize of the ids
 * instead of the reference's bilinear-on-ids, bit1 = skip the Pavement->Road remap, bit2 = materialise the class logits
 * (ssm_segnet_logits can then read frame 0 of the last sub-batch; without it the ArgMax runs in the last layer's epilogue
 * and the logits never reach memory -- the labels are identical either way) */
int ssm_segnet_forward_dev(ssm_ctx* ctx, const uint8_t* bgr_dev, int n, uint8_t* labels_net_dev, uint8_t* sem_bgr_dev, int flags);
/* single layer ops on host NHWC fp16 tensors, for exact per-op tests (integer-valued data makes fp16/fp32 exact):
 * op 0 = conv layer `arg` on in[H][W][CinPad16] -> out[H][W][CoutPad16]; op 1 = max-pool 2x2 s2 ceil with C = arg:
 * in[H][W][C] -> out[PH][PW][C] + code[PH][PW][C]; op 2 = unpool: in[PH][PW][C] + code -> out[H][W][C];
 * op 3 = conv layer `arg` + max-pool through the fused kernel: out[PH][PW][CoutPad16] + code (same shape);
 * op 4 = un-pool + conv layer `arg` through the fused kernel: in[PH][PW][CinPad16] + code (same shape) -> out[H][W][CoutPad16];
 * op 5 = conv layer `arg` (Cout <= 12: the last one) + class ArgMax through the fused epilogue the network runs: in[H][W][CinPad16] ->
 * code[H][W] (the labels; `out` is not written) */
int ssm_segnet_debug_op(ssm_ctx* ctx, int op, int arg, const uint16_t* in, int H, int W, uint16_t* out, uint8_t* code);
/* the image pyramid of n frames (host, w x h x channels each, rows packed; n <= max_batch) -> out (n x the pyramid buffer of one frame: every level,
 * rows padded to 16 bytes), for exact tests of the fused pyramid kernel: bands < 0 = gray_kernel + one resize launch per level, 0 = what the ORB
 * calls run, > 0 = the fused kernel with that many bands (SSM_E_INVAL where the geometry has no fused form at that band count).  *bytes: one frame's
 * buffer (img and out both NULL: only that) */
int ssm_debug_pyramid(ssm_ctx* ctx, const uint8_t* img, int channels, int n, int bands, uint8_t* out, int* bytes);
/* the BLURRED pyramid of n frames (host, as for ssm_debug_pyramid; n <= max_batch), for exact tests of the blur kernels on every pixel: the pyramid is built the
 * way the ORB calls build it, then blurred by the launch they make -- the variant the context was created with (SSM_BLUR_VARIANT=0 at ssm_create: the VALU
 * kernel, else the matrix-core one).  out: n x ssm_debug_pyramid's buffer, in ITS layout -- level l at the same offset, rows of `stride` bytes -- so that
 * byte i here is the 7x7 Gaussian (taps 18 34 49 55 49 34 18 / 256, BORDER_REFLECT_101, (v + 2^15) >> 16, saturated) at the pixel whose level image is byte i
 * there.  The padding columns [w, stride) of every row are zero.  The device keeps the blurred pyramid in tiles of 8 rows x 16 columns; the un-tiling is a
 * host loop over that layout, so a wrong tile offset shows as wrong pixels.  *bytes: one frame's buffer (img and out both NULL: only that) */
int ssm_debug_orb_blur(ssm_ctx* ctx, const uint8_t* img, int channels, int n, uint8_t* out, int* bytes);
/* the describe stage (slot bookkeeping, orientation moments, angle + sin / cos + keypoint record + position, steered BRIEF) on a PLANTED selection, for exact
 * tests at chosen keypoints: pyramid and blurred pyramid of n frames as above, then the describe launches exactly as the ORB calls make them, with the
 * selection uploaded in place of FAST's and the quad-tree's.
 *   nsel     n x orb_levels counts; count of level l: 0 .. (features of the level + 3), the slots the level has
 *   sel      the planted keypoints of all frames, frame by frame and level by level, sum(nsel) words x | y << 12 | score << 24 in level coordinates.
 *            Every point must lie in [19, w_l - 19) x [19, h_l - 19): the window FAST reports in and the kernels rely on (their patch loads have no border case)
 *   depth    NULL, or n depth images (w x h uint16, rows packed); moments: NULL, or (m10, m01) per planted keypoint, in sel's order: they replace the
 *            orientation kernel's sums before the angle is taken from them, so any pair can be put through atan2 / sin / cos and the BRIEF that follows
 *   outputs  nkp: n counts; kps, desc (32 bytes each), pos3d (3 floats each), moments_out (m10, m01) and sincos_out (sin, cos): n x ssm_orb_capacity
 *            records each, frame f from f x capacity on, in output order = sel's order; all required.  Records from nkp[f] on are not written by the kernels
 *            and come back as bytes 0xA5.  pos3d is project2dTo3d at the truncated level-0 position, zero without a depth image or at depth 0
 * SSM_E_INVAL, on the host and before anything is launched: n outside 1 .. max_batch, a count outside its range, a point outside its window.  The context's
 * later ORB calls are not affected (they overwrite the selection). */
int ssm_debug_orb_describe(ssm_ctx* ctx, const uint8_t* img, int channels, int n, const uint16_t* depth, const int32_t* nsel, const uint32_t* sel,
                           const int32_t* moments, int32_t* nkp, ssm_keypoint* kps, uint8_t* desc, float* pos3d, int32_t* moments_out, float* sincos_out);
/* the quad-tree selection (ORBextractor::DistributeOctTree, one block per (frame, level)) ALONE on PLANTED candidate lists, for exact tests of its list order,
 * its two split phases and its drop rule: the lists and the cell maxima of n frames are uploaded in place of FAST's, then the one launch the ORB calls make.
 *   geom     may be NULL; else orb_levels x SSM_OCTREE_GEOM_LEVEL_INTS ints -- per level w, h, minBorder, nCols, nRows, wCell, hCell, features, root nodes, candidate
 *            capacity, selection slots -- then cells_total, cand_total, sel_total (per frame) and the node capacity (256 / 512 / 1024) of the kernel instance that
 *            runs.  With ncand, cand and cellmax all NULL only this is filled, and nothing is launched
 *   ncand    n x orb_levels counts, each 0 .. the level's candidate capacity
 *   cand     the candidates of all (frame, level) pairs, frame by frame and level by level, in the order they shall lie in the buffer: sum(ncand) pairs of words
 *            x | y << 12 | score << 24 (x, y relative to minBorder, score = the FAST response) and cell << 14 | yInCell << 7 | xInCell (the rank word: detection
 *            order).  With W = w - 2 * minBorder, H = h - 2 * minBorder: 3 <= x < W - 3, 3 <= y < H - 3; cell = ((y - 3) / hCell) * nCols + (x - 3) / wCell,
 *            xInCell = x - ((x - 3) / wCell) * wCell, yInCell likewise: what the FAST kernel writes
 *   cellmax  n x cells_total: per FAST cell the largest S = score + 1 among its kept maxima, 0 .. 255 (a candidate survives iff S > (cellmax > ini ? ini : min))
 *   outputs  nsel: n x orb_levels; sel: n x sel_total words x | y << 12 | score << 24 in level coordinates, level l of frame f from f * sel_total + the sum of the
 *            lower levels' slots on, in output order (slots the kernel did not write hold the bytes 0xA5); status: the ORB scratch-overflow word of this launch;
 *            nodeof (may be NULL): n x cand_total, the kernel's global node-id scratch after the launch, laid out like the candidate buffer -- a level with more
 *            than 2048 candidates keeps the node id of every candidate there (its final node, or 0xFFFF where the drop rule removed it), every other entry
 *            still holds the bytes 0xA5
 * SSM_E_INVAL, on the host and before anything is launched: n outside 1 .. max_batch, a count outside its range, a position outside its window, a cell id outside
 * the level, a rank word that does not match its position, a cell maximum outside 0 .. 255.  The status word is zero again when the call returns, and the
 * context's later ORB calls are not affected (they overwrite every buffer). */
#define SSM_OCTREE_GEOM_LEVEL_INTS 11
int ssm_debug_orb_octree(ssm_ctx* ctx, int n, const int32_t* ncand, const uint32_t* cand, const int32_t* cellmax, int32_t* geom, int32_t* nsel, uint32_t* sel,
                         int32_t* status, uint16_t* nodeof);
/* the FAST tile plan of a configuration, on the host only (no context, no device): for exact tests of the tiling.  Per tile, 16 ints:
 * level, interior x0, x1, y0, y1 (half-open), scored rectangle xs0, xs1, ys0, ys1 (interior + 1 on each side, clipped to the FAST window
 * [19, w - 19) x [19, h - 19)), 4-column groups, scored rows, cell columns and cell rows the scored rectangle touches, level w, h, stride.
 * *ntiles: the tile count (tiles NULL: only that; SSM_E_INVAL when cap is smaller).  limits (6 ints, may be NULL): the static LDS bytes of the FAST
 * kernel, the most groups and scored rows its arrays hold, the staged pixel row width and row count, the staging area (candidates) */
int ssm_debug_fast_plan(const ssm_config* cfg, int32_t* tiles, int cap, int* ntiles, int32_t* limits);
/* the FAST kernel's compass quick test (include/ssm/fast_quick_core.h, the code the kernel runs), on the host only: n groups of four horizontally
 * adjacent positions.  words: per group the five pixel dwords the kernel reads -- the centres (byte j = position j), the dwords left and right of
 * them in the row, the dwords 3 rows up and 3 rows down.  threshold: 0 .. 255; valid: 1 .. 4, the positions of the group inside the scored
 * rectangle (the others never pass).  out: per group one byte, bit j = position j passes */
int ssm_debug_fast_quick(const uint32_t* words, int n, int threshold, int valid, uint8_t* out);
/* the fused pyramid's plan of a configuration, on the host only (no context, no device): the work items of every (band, level >= 1), listed by the
 * decomposition the kernel uses.  bands > 0: that band count; 0: what batches run; -1: what the one-frame call runs (4-pixel items on every level).  Per item, 12 ints: level, band,
 * pixels per item (8, or 4 where the level's groups do not fit the 8-pixel layout), column group, first and last output row it writes, first and last
 * source row it reads, the byte range [lo, hi) its windows read in the source level's LDS buffer and the byte range [lo, hi) it writes in its own.
 * *nitems: the item count (items NULL: only that; SSM_E_INVAL when cap is smaller).  band_tab (may be NULL): bands x levels x (comp_lo, comp_hi,
 * own_lo, own_hi), rows inclusive.  limits (52 ints, may be NULL): band count (0: the geometry has no fused plan at this count; nothing else is
 * listed), LDS bytes, offset of the odd levels' buffer, slack bytes behind each buffer, threads per block, LDS limit, levels, bit masks per level
 * (has the 4-pixel table; fits the 8-pixel layout; the plan uses the 8-pixel item), six
 * reserved, then (w, h, stride) of each level */
int ssm_debug_pyramid_plan(const ssm_config* cfg, int bands, int32_t* items, int cap, int* nitems, int32_t* band_tab, int32_t* limits);
/* the SGBM post stages alone, as the last steps of ssm_sgbm launch them, on n stacked int16 maps (host, w x h each, rows packed) -> out (same shape):
 * op bit 0 = medianBlur 3x3 (replicate border), bit 1 = filterSpeckles (4-neighbours, both != new_val, |a - b| <= max_diff; components of at most
 * max_size pixels become new_val) on the median's output, or on the input without bit 0.  For exact tests of the kernels on constructed maps */
int ssm_debug_sgbm_post(ssm_ctx* ctx, const int16_t* disp, int w, int h, int n, int op, int new_val, int max_size, int max_diff, int16_t* out);
/* one level (0 .. 3) of the LK pyramid that the last ssm_lk_track built and its Scharr derivatives, for exact tests of the pyramid and derivative kernels on
 * every pixel: side 0 = the previous image, 1 = the next; img receives *w x *h bytes, der *w x *h (dx, dy) int16 pairs, rows packed (either may be NULL: only
 * the size).  SSM_E_INVAL when the last stereo call on the context was not an ssm_lk_track with n > 0 */
int ssm_debug_quad_pyramid(ssm_ctx* ctx, int side, int level, uint8_t* img, int16_t* der, int* w, int* h);
/* what the library itself holds at this moment, process-wide (every context with its lanes, every tracker): live buffers, their device bytes and their
 * page-locked host bytes, each as asked for.  Memory handed to the caller (ssm_dev_alloc, ssm_host_alloc) is not counted.  Any pointer may be NULL.  For
 * tests of ownership: exact, unlike the device's free memory, which moves with other processes */
void ssm_debug_live_allocations(int* buffers, size_t* device_bytes, size_t* pinned_bytes);
/* likewise the streams and events the library itself holds (contexts with their side lanes and SGBM fans, the profiling pool, trackers with a stream of
 * their own): every one is a Stream / Event of csrc/ssm_ctx.h.  Either pointer may be NULL */
void ssm_debug_live_handles(int* streams, int* events);
/* class logits (12 floats per net pixel, 360*480 pixels) of frame 0 of the most recent forward: for tolerance tests */
int ssm_segnet_logits(ssm_ctx* ctx, float* out);

/* per-stage device time of the most recent ssm_seq_process, measured with hipEvents on the stream each stage runs on.
 * ssm_seq_process runs the (SegNet ->) map stage of a sub-batch on a second stream beside the ORB -> match chain, so with
 * on = 1 the stage times overlap (their sum exceeds the wall time); on = 2 additionally keeps everything on the context
 * stream, which gives each stage's undisturbed duration (and a lower throughput).  0 = off.
 * names/ms/launches hold cap entries; returns count in *n_out. */
int ssm_set_profiling(ssm_ctx* ctx, int on);
int ssm_get_stage_times(ssm_ctx* ctx, const char** names, float* ms, int* launches, int cap, int* n_out);

/* ---- utilities (device memory without torch; synthetic stream generator for bench/tests) */
int ssm_dev_alloc(ssm_ctx* ctx, size_t bytes, void** out);
int ssm_dev_free(ssm_ctx* ctx, void* p);
int ssm_dev_mem_info(ssm_ctx* ctx, size_t* free_bytes, size_t* total_bytes);      /* hipMemGetInfo on the context's device */
int ssm_memcpy_h2d(ssm_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int ssm_memcpy_d2h(ssm_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* the same upload, enqueued on the context stream without waiting: src_host must stay valid and unchanged until the next ssm_sync / synchronous call of the context
 * (BatchTracker uploads a frame when it is queued, while the caller reads the next one) */
int ssm_memcpy_h2d_async(ssm_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
/* the download, enqueued without waiting: dst_host holds the data after the next ssm_sync (page-locked dst_host: a plain DMA; BatchStereoTracker fetches a chunk's depth images so) */
int ssm_memcpy_d2h_async(ssm_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* page-locked host memory for frame buffers (the reference's cv::Mat data comes from cv::imread / a camera driver: a cv::Mat can wrap user memory, cv::Mat(rows, cols,
 * type, ptr)).  The host-pointer calls stage pageable inputs through a pinned ring (one extra pass over every image: ~0.06 ms of ssm_orb_extract's 0.25 for a 640 x 480
 * frame); inputs that already live in memory from ssm_host_alloc are read by the DMA engine / the kernels where they are.  Any device of the process may use the
 * memory.  ssm_host_free(NULL) is a no-op. */
int ssm_host_alloc(size_t bytes, void** out);
int ssm_host_free(void* p);
/* synthetic 640x480 RGB-D + 12-class stream of BASELINE.json configs[1]; device pointers;
 * label_ids may be NULL */
int ssm_synth_frames_dev(ssm_ctx* ctx, uint64_t seed, int first_frame, int n, int w, int h,
                         uint8_t* bgr, uint16_t* depth, uint8_t* sem_bgr, uint8_t* label_ids, double* pose);

#ifdef __cplusplus
}
#endif
#endif
