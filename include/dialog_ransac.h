/*
 * dialog_ransac.h -- C ABI of the MI355X-native RANSAC plane-segmentation path.
 *
 * Drop-in boundary for czh55/Dialog's plane stage.  The reference has no FFI of its own: its
 * plane stage is a header "module" of free functions over globals (Dialog/PlaneDetect.h:143-211,
 * source_cloud :104, source_normal :107, plane_clouds :100) that calls PCL.  These entry points
 * replace the PCL calls that sit under PlaneDetect.h's functions:
 *
 *   dlg_sac_segment      <- pcl::SACSegmentation<PointXYZ>::segment(PointIndices&, ModelCoefficients&)
 *                           with SACMODEL_PLANE / SAC_RANSAC (reference call pattern
 *                           Dialog/SimplifyVerticesSize.cpp:62-67, :86-87)
 *   dlg_extract_planes   <- the segmentation slot Dialog/PlaneDetect.h:667-1355 (createPS ..
 *                           mergePlanes) re-filled by sequential extract-and-remove RANSAC, the
 *                           analogue of the re-run loop PCLViewer.cpp:1120-1177 /
 *                           PlaneDetect.h:1500-1573; output feeds plane_clouds (PlaneDetect.h:100)
 *   dlg_estimate_normals <- estimateNormal(), Dialog/PlaneDetect.h:515-545
 *                           (pcl::NormalEstimationOMP, radius r_for_estimate_normal)
 *   dlg_regulate_normals <- regulateNormal(), Dialog/PlaneDetect.h:547-665
 *
 * Conventions: inputs are borrowed for the duration of a call; outputs go to caller buffers
 * (capacity given; DLG_ERR_CAPACITY + required size when too small).  No exceptions cross the
 * ABI.  "No model" is DLG_OK with *n_inliers == 0 and a zeroed coefficient vector (the C++ shim
 * maps it to PCL's empty indices/values).  One context per host thread; calls block until the
 * device work of the call has finished.  Every compute entry point runs on the GPU: there is no
 * CPU fallback, and creating a context without a usable HIP device fails with DLG_ERR_NO_DEVICE.
 */
#ifndef DIALOG_RANSAC_H
#define DIALOG_RANSAC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: dlg_extract_stats gained lean_rounds, spec_misses, pcl_host_checks; dlg_score_benchmark's
 * 4th argument is a DLG_SCORE_* kernel; execution paths are context options, not environment
 * variables.  3: dlg_extract_stats gained refit_walk_ms; dlg_float_sums, dlg_cloud_estimate_normals
 * and dlg_plane_border were added; dlg_cloud_drop_spatial keeps the copy's buffers.
 * 4: dlg_extract_stats gained refit_repair_ms (refit_walk_ms is k_fs_walk alone on every rank);
 * DLG_OPT_FS_POISON; dlg_cloud_regulate_normals; DLG_OPT_HYP_SHARD; DLG_OPT_FS_ONE_WALK;
 * dlg_extract_stats gained refit_repairs; dlg_prune_stats fills 8 counters; DLG_OPT_FS_SEGMENTS;
 * the tile-scorer option's getter returns the value set.
 * 5: a failing rank aborts its group (peers return DLG_ERR_COMM); DLG_OPT_FAULT_INJECT,
 * DLG_OPT_SYNC_CHECK, DLG_OPT_COMM_TIMEOUT_MS, DLG_OPT_SEL1_TICKET, DLG_OPT_BOUNDS_STREAM;
 * DLG_OPT_SPATIAL_CURVE, DLG_OPT_FS_JOIN, DLG_OPT_UNREFINED_LIST (same ABI version: added options);
 * DLG_OPT_HYP_SHARD defaults to -1 (automatic); dlg_shard_range; dlg_cloud_signature (same ABI
 * version: an added entry); DLG_SACMODEL_PERPENDICULAR_PLANE, DLG_SACMODEL_PARALLEL_PLANE,
 * dlg_ctx_set_axis / dlg_ctx_get_axis, dlg_score_samples, dlg_axis_verdicts (same ABI version: an
 * added enum value and added entries); dlg_voxel_grid, dlg_voxel_grid_cloud, dlg_voxel_params,
 * dlg_voxel_stats, DLG_OPT_VOXEL_LONG_RUN (same ABI version: added entries and an added option);
 * dlg_statistical_outlier_removal, dlg_statistical_outlier_removal_cloud, dlg_sor_params,
 * dlg_sor_stats, DLG_OPT_SOR_LITERAL (same ABI version: added entries and an added option);
 * dlg_moving_least_squares, dlg_moving_least_squares_cloud, dlg_mls_params, dlg_mls_stats (same ABI
 * version: added entries); dlg_icp_align, dlg_icp_correspondences, dlg_icp_params_default,
 * dlg_icp_params, dlg_icp_stats, dlg_icp_iteration, DLG_OPT_ICP_REVERSED (same ABI version: added
 * entries and an added option); DLG_OPT_ICP_MAX_BLOCKS (same ABI version: an added option);
 * DLG_OPT_CULL, dlg_cull_stats, DLG_SCORE_BOUND / DLG_SCORE_CULLED (same ABI version: an added
 * option, entry and benchmark ids); dlg_fpfh_estimate, dlg_cloud_fpfh, dlg_fpfh_params,
 * dlg_fpfh_stats (same ABI version: added entries); dlg_sac_ia_align, dlg_sac_ia_score,
 * dlg_fpfh_knn, dlg_sac_ia_params_default, dlg_sac_ia_params, dlg_sac_ia_hypothesis,
 * dlg_sac_ia_stats (same ABI version: added entries); DLG_OPT_CULL_FUSE (same ABI version: an added
 * option); dlg_gs_params_default, dlg_gs_space, dlg_gs_vote, dlg_gs_segment, dlg_cloud_gs_segment,
 * dlg_gs_params, dlg_gs_stats, dlg_gs_result (same ABI version: added entries); dlg_knn_stats,
 * dlg_knn_record (same ABI version: an added entry) */
#define DLG_ABI_VERSION 5

typedef enum {
  DLG_OK = 0,
  DLG_ERR_INVALID = 1,    /* bad argument */
  DLG_ERR_HIP = 2,        /* HIP runtime error */
  DLG_ERR_NO_DEVICE = 3,  /* no usable gfx950 device */
  DLG_ERR_COMM = 4,       /* RCCL / communicator error; several ranks: the group was aborted
                             (a peer's call failed -- dlg_last_error names the rank and its
                             error -- or a wait timed out).  An aborted group stays aborted:
                             destroy its contexts */
  DLG_ERR_CAPACITY = 5,   /* output buffer too small; required size reported */
  DLG_ERR_INTERNAL = 6
} dlg_status;

/* pcl::SacModel values (pcl/sample_consensus/model_types.h) */
enum {
  DLG_SACMODEL_PLANE = 0,
  DLG_SACMODEL_NORMAL_PLANE = 11,
  /* SACMODEL_PLANE with isModelValid against the context's axis (dlg_ctx_set_axis): a
     hypothesis that fails it counts 0 inliers inside the RANSAC loop and selects none */
  DLG_SACMODEL_PERPENDICULAR_PLANE = 9, /* the plane's normal within eps_angle of the axis */
  DLG_SACMODEL_PARALLEL_PLANE = 15      /* the plane's normal perpendicular to the axis within
                                           eps_angle (the plane is parallel to the axis) */
};
/* refit of the winning model (SampleConsensusModelPlane::optimizeModelCoefficients) */
enum {
  DLG_REFIT_PCL = 0,   /* PCL's float refit: computeMeanAndCovarianceMatrix's single-pass float
                          sums in list order + float eigen33, bit-exact with PCL.  The sums run
                          on the device, exactly (fsum.hpp); several ranks hand the chains'
                          values from rank to rank in list order (RCCL send/recv) */
  DLG_REFIT_FAST = 1   /* NOT PCL's arithmetic: exact integer moments of the inliers + a double
                          Jacobi solve (the least-squares plane to within float rounding; order-
                          and rank-count-independent).  Its planes differ from PCL's by up to
                          ~1e-4 and can change which plane a later extract round picks */
};

typedef struct dlg_ctx dlg_ctx;
typedef struct dlg_cloud dlg_cloud;

/* Host points, borrowed.  stride_bytes 16 = pcl::PointXYZ (x, y, z, pad), 12 = packed xyz. */
typedef struct {
  const float* xyz;
  int64_t n;
  int64_t stride_bytes;
} dlg_points;

typedef struct {
  double threshold;            /* setDistanceThreshold */
  int max_iterations;          /* setMaxIterations (PCL default 50) */
  double probability;          /* setProbability (PCL default 0.99) */
  int optimize;                /* setOptimizeCoefficients (PCL default 1) */
  uint32_t seed;               /* 12345u = PCL's non-random seed */
  int model;                   /* DLG_SACMODEL_PLANE | DLG_SACMODEL_NORMAL_PLANE (needs normals) |
                                  DLG_SACMODEL_PERPENDICULAR_PLANE | DLG_SACMODEL_PARALLEL_PLANE
                                  (axis and eps_angle: dlg_ctx_set_axis) */
  double normal_distance_weight; /* SACSegmentationFromNormals::setNormalDistanceWeight (0.1) */
  int refit_mode;              /* DLG_REFIT_PCL (default) | DLG_REFIT_FAST */
  int hypotheses_per_launch;   /* upper bound of one scoring launch; 0 = 4096 */
  int gather_inliers;          /* multi-rank: 1 = every rank receives the global inlier list */
} dlg_sac_params;

typedef struct {
  int iterations;              /* RandomSampleConsensus iterations_ at exit */
  int skipped;
  int has_model;
  int launches;                /* scoring launches */
  int64_t draws;               /* drawIndexSample calls */
  int32_t best_sample[3];      /* global indices of the winning triple */
  float coeff_unrefined[4];
  int64_t n_unrefined;         /* inliers of the unrefined model */
  int64_t n_active;            /* points the model was fitted on (all ranks) */
  int64_t tests;               /* point-plane tests PCL's loop evaluates (iterations x n_active) */
  int64_t tests_scored;        /* point-plane tests the GPU scored (>= tests: batch tail) */
  double score_ms;             /* device time of the scoring launches (HIP events) */
} dlg_sac_stats;

typedef struct {
  int rounds;                  /* segment() calls */
  int64_t tests;
  int64_t tests_scored;
  int score_launches;
  double score_ms;             /* sum of scoring-kernel device time */
  double select_ms;            /* sum of select/compact/moments device time */
  double wall_ms;              /* host wall time of the call */
  int lean_rounds;             /* rounds that took the single-pass (lean-list) select */
  int spec_misses;             /* speculative device picks the host replay overturned */
  int pcl_host_checks;         /* device PCL refits whose tail the host recomputed (an eigen33
                                  transcendental near a float rounding boundary) */
  double refit_walk_ms;        /* of select_ms: the device PCL refit's chain walks (k_fs_walk,
                                  latency-bound sequential chains), lean rounds */
  double refit_repair_ms;      /* several ranks: the PCL refit's repair phase on the stream (the
                                  exactness checks and the repair walks, k_fs_repair), summed
                                  over the rounds */
  int refit_repairs;           /* several ranks: the PCL refit's repair steps summed over the
                                  rounds (hand-over: W - 1 a round; DLG_OPT_FS_ONE_WALK 2: the
                                  parallel repair iterations) */
  double refit_rebase_ms;      /* several ranks, rank > 0, DLG_OPT_FS_ONE_WALK 0 / 2: the time
                                  between the first walk's end and the second walk's start (the
                                  allgather of the walks' ends + the rebase kernels); refit_walk_ms
                                  then holds the two walks alone */
} dlg_extract_stats;

void dlg_sac_params_default(dlg_sac_params* p);   /* PCL SACSegmentation defaults */
const char* dlg_status_string(dlg_status s);
int dlg_abi_version(void);
/* sizeof of the ABI's structs, for bindings to check their layouts: 0 dlg_points, 1 dlg_sac_params,
 * 2 dlg_sac_stats, 3 dlg_extract_stats, 4 dlg_planes, 5 dlg_postprocess_params, 6 dlg_voxel_params,
 * 7 dlg_voxel_stats, 8 dlg_sor_params, 9 dlg_sor_stats, 10 dlg_mls_params, 11 dlg_mls_stats,
 * 13 dlg_icp_params, 14 dlg_icp_stats, 15 dlg_icp_iteration, 17 dlg_fpfh_params, 18 dlg_fpfh_stats,
 * 19 dlg_sac_ia_params, 20 dlg_sac_ia_hypothesis, 21 dlg_sac_ia_stats, 23 dlg_gs_params,
 * 24 dlg_gs_stats, 25 dlg_gs_result, 26 dlg_knn_record (12, 16 and 22 are unassigned); -1 otherwise */
int64_t dlg_abi_struct_size(int which);

/* ---- contexts ------------------------------------------------------------------------------ */
dlg_status dlg_ctx_create(dlg_ctx** out, int device);
/* one process per GPU: rank/world over RCCL (xGMI).  unique_id: 128 bytes from dlg_get_unique_id
 * on rank 0, distributed out of band (e.g. torch.distributed gloo).  world 1 with a NULL id is a
 * plain context; world 1 with an id runs a 1-rank RCCL communicator. */
dlg_status dlg_get_unique_id(void* unique_id_128);
dlg_status dlg_ctx_create_dist(dlg_ctx** out, int device, int rank, int world,
                               const void* unique_id_128);
/* in-process group of `world` ranks sharing one device, one host thread per rank (test and
 * rehearsal of the sharded path on a single GPU); the group's contexts must be driven
 * concurrently, rank r from its own thread. */
dlg_status dlg_ctx_create_loopback_group(dlg_ctx** out_array, int world, int device);
dlg_status dlg_ctx_destroy(dlg_ctx* ctx);
const char* dlg_last_error(const dlg_ctx* ctx);
/* SACSegmentation::setAxis / setEpsAngle: the axis (not normalised by the caller or on storing) and
 * the angle in radians that DLG_SACMODEL_PERPENDICULAR_PLANE and DLG_SACMODEL_PARALLEL_PLANE test
 * a hypothesis against; context state, (0, 0, 0) and 0 by default, read by every call whose
 * prm->model is one of the two.  eps_angle <= 0 accepts every plane (both models are then
 * SACMODEL_PLANE bit for bit).  A NaN or infinite axis component or a NaN eps_angle:
 * DLG_ERR_INVALID.  Several ranks: every rank must set the same values (DLG_OPT_SYNC_CHECK
 * compares them).  The arithmetic is PCL 1.8's isModelValid restated from memory (parity
 * unpinned):
 *   Cn = (c0, c1, c2, 0).normalized() of the plane's float coefficients
 *   perpendicular: rad = clamp(axis.normalized() . Cn, -1, 1) (float dot, double clamp),
 *                  invalid when min(acos(rad), M_PI - acos(rad)) > eps_angle
 *   parallel     : invalid when |axis . Cn| (float, the axis as given) > |sin(eps_angle)|
 * An invalid hypothesis from a good sample is an ordinary iteration with 0 inliers (it is not a
 * skipped sample), so when every hypothesis is invalid the first good draw wins: has_model = 1,
 * its real coefficients reported, 0 inliers.  The refit is SACMODEL_PLANE's (unconstrained); a
 * refined plane that fails the test is reported with 0 inliers. */
dlg_status dlg_ctx_set_axis(dlg_ctx* ctx, const float axis[3], double eps_angle);
dlg_status dlg_ctx_get_axis(const dlg_ctx* ctx, float axis[3], double* eps_angle);
dlg_status dlg_ctx_info(const dlg_ctx* ctx, int* rank, int* world, int* device);

/* ---- device-resident clouds (this rank's contiguous shard of the global index order) -------- */
/* The active list starts as point xyz[k] for k = indices[i] (pcl setIndices(); any order,
 * duplicates allowed) or k = 0..n-1 when indices is NULL; its global id is id_base + k.
 * Multi-rank: each rank uploads its contiguous shard with id_base = the shard's first global id;
 * the global active list is the concatenation of the ranks' lists in rank order. */
dlg_status dlg_cloud_upload(dlg_ctx* ctx, const dlg_points* pts, const int32_t* indices,
                            int64_t n_indices, int32_t id_base, dlg_cloud** out);
dlg_status dlg_cloud_destroy(dlg_cloud* cloud);
/* re-activate every point of the cloud (undo extract-and-remove) */
dlg_status dlg_cloud_reset(dlg_cloud* cloud);
/* Morton-ordered copy of the cloud's finite points + tile bounding spheres for the pruned
 * scoring kernel (same counts, fewer evaluated tests).  Built by dlg_cloud_upload for clouds of
 * >= 131072 points (context option DLG_OPT_PRUNE: 0 never, 1 always); this forces it for any cloud
 * (call right after upload or dlg_cloud_reset).  Kept in step by SACMODEL_PLANE extraction. */
dlg_status dlg_cloud_build_spatial(dlg_ctx* ctx, dlg_cloud* cloud);
/* drop the Morton copy (the exhaustive scoring kernels take over until it is built again; its
 * device buffers are kept for the next build and freed by dlg_cloud_destroy); resets the cloud to
 * all points active.  With dlg_cloud_build_spatial it times the index build on device-resident
 * points. */
dlg_status dlg_cloud_drop_spatial(dlg_cloud* cloud);
dlg_status dlg_cloud_active(const dlg_cloud* cloud, int64_t* n_active_local);
/* Content signature of the cloud as uploaded (every point, whatever has been extracted since):
 * the sum modulo 2^64 over list positions i = 0..n-1 of h(i, x, y, z, id), where x, y, z are the
 * point's float bit patterns (-0.0 differs from +0.0, NaN payloads count), id its global id, and
 *   h = (i + 1) * 0x9E3779B97F4A7C15;  h ^= x | y << 32;   h *= 0xBF58476D1CE4E5B9;  h ^= h >> 29;
 *   h ^= z | id << 32;  h *= 0x94D049BB133111EB;  h ^= h >> 32        (64-bit, wrapping)
 * so any changed bit of one point and (up to a 2^-64 coincidence) any reordering change it; 0 for
 * an empty cloud.  Two ranks hold the same cloud exactly when their counts, id_base and
 * signatures agree.  One reduction on the device, run at the first request and kept; nothing
 * else computes it (DLG_OPT_HYP_SHARD's automatic decision does not read it yet: see its
 * comment). */
dlg_status dlg_cloud_signature(dlg_ctx* ctx, dlg_cloud* cloud, uint64_t* signature_out);
/* SACSegmentationFromNormals::setInputNormals: one normal record per uploaded point (n = the
 * dlg_points n of dlg_cloud_upload; the cloud's indices select from it like from the points).
 * stride_bytes 16 = (nx, ny, nz, curvature), >= 32 = pcl::Normal (curvature at byte 16).
 * Required by DLG_SACMODEL_NORMAL_PLANE; resets the cloud to all points active. */
dlg_status dlg_cloud_set_normals(dlg_ctx* ctx, dlg_cloud* cloud, const float* normals, int64_t n,
                                 int64_t stride_bytes);

/* ---- RANSAC ----------------------------------------------------------------------------------- */
/* SACSegmentation::segment on the cloud's active points (not removed).  inliers_out receives
 * global ids in active-list order (this rank's part, or all ranks' if gather_inliers). */
dlg_status dlg_sac_segment(dlg_ctx* ctx, dlg_cloud* cloud, const dlg_sac_params* prm,
                           float coeff_out[4], int32_t* inliers_out, int64_t cap,
                           int64_t* n_inliers, dlg_sac_stats* stats);

/* Host-buffer convenience: upload, segment, free (PCL setInputCloud + setIndices + segment). */
dlg_status dlg_sac_segment_host(dlg_ctx* ctx, const dlg_points* pts, const int32_t* indices,
                                int64_t n_indices, const dlg_sac_params* prm, float coeff_out[4],
                                int32_t* inliers_out, int64_t cap, int64_t* n_inliers,
                                dlg_sac_stats* stats);

/* Sequential extract-and-remove: round r runs segment() on the remaining points (RNG reseeded,
 * shuffled list = remaining list), records the plane and removes its inliers.  Stops when fewer
 * than max(3, min_inliers) points remain, when no model is found, or when a plane has fewer than
 * min_inliers inliers (not recorded).  coeffs_out: 4*max_planes floats; offsets_out:
 * max_planes+1 (offsets into inliers_out); inliers_out capacity `cap` ids. */
dlg_status dlg_extract_planes(dlg_ctx* ctx, dlg_cloud* cloud, const dlg_sac_params* prm,
                              int max_planes, int64_t min_inliers, float* coeffs_out,
                              int64_t* offsets_out, int32_t* inliers_out, int64_t cap,
                              int* n_planes, dlg_extract_stats* stats);

/* ---- normals (Dialog/PlaneDetect.h:515-665) -------------------------------------------------- */
/* pcl::NormalEstimation(OMP)::compute on every point of pts (estimateNormal(),
 * PlaneDetect.h:515-545): neighbours = radius search (k_nn == 0, radius > 0; PCL's radius
 * r_for_estimate_normal, config.txt:4) or the k_nn nearest (k_nn in 1..64; PCLViewer.cpp:507-522
 * uses 20), as KdTreeFLANN returns them; normal = eigenvector of the smallest eigenvalue of the
 * neighbourhood covariance, curvature = lambda0 / (lambda0 + lambda1 + lambda2), flipped towards
 * viewpoint (NULL = origin).  < 3 neighbours or a non-finite point -> NaN normal and curvature.
 * normals_out: n records of out_stride_bytes: 16 = (nx, ny, nz, curvature); >= 32 = pcl::Normal
 * (normal_x/y/z at bytes 0-11, curvature at byte 16, other fields zeroed). */
dlg_status dlg_estimate_normals(dlg_ctx* ctx, const dlg_points* pts, float radius, int k_nn,
                                const float viewpoint[3], float* normals_out,
                                int64_t out_stride_bytes);
/* dlg_estimate_normals with an arithmetic mode:
 *   DLG_NORMALS_PCL_FLOAT (what dlg_estimate_normals uses): PCL 1.8's computePointNormal --
 *     computeMeanAndCovarianceMatrix's single-pass float sums over the neighbours in FLANN's
 *     (d2, index) order, pcl::eigen33 in float, curvature |lambda0 / trace| in float, the
 *     viewpoint flip; bit-exact with the oracle's restatement of it
 *   DLG_NORMALS_CENTRED_DOUBLE: the same neighbourhoods, moments centred on the query in double
 *     and eigen33 in double (better conditioned far from the origin; not PCL's rounding) */
enum { DLG_NORMALS_PCL_FLOAT = 0, DLG_NORMALS_CENTRED_DOUBLE = 1 };
dlg_status dlg_estimate_normals_ex(dlg_ctx* ctx, const dlg_points* pts, float radius, int k_nn,
                                   const float viewpoint[3], float* normals_out,
                                   int64_t out_stride_bytes, int mode);
/* estimateNormal() on a cloud already on the device (the C5 chain: normals fused ahead of the
 * NORMAL_PLANE segmentation without a host round trip): the normals of dlg_estimate_normals_ex
 * (same neighbourhoods, same arithmetic for `mode`) over the cloud's uploaded points, attached
 * to the cloud as dlg_cloud_set_normals would attach them (the cloud is reset).  normals_out
 * (nullable): also copied out, records of out_stride_bytes as dlg_estimate_normals writes them.
 * One rank only: a context of a communicator with world > 1 holds a shard, whose points near the
 * cut would lose the neighbours on other ranks (PCL's normals are over the whole cloud), so it
 * gets DLG_ERR_INVALID -- estimate the normals over the whole cloud (dlg_estimate_normals_ex) and
 * attach each rank's slice with dlg_cloud_set_normals. */
dlg_status dlg_cloud_estimate_normals(dlg_ctx* ctx, dlg_cloud* cloud, float radius, int k_nn,
                                      const float viewpoint[3], int mode, float* normals_out,
                                      int64_t out_stride_bytes);
/* regulateNormal() first-round branch (PlaneDetect.h:586-646): flip the seed normal unless
 * seed_is_outward (is_norm_direction_valid), then BFS over radius-`radius` neighbourhoods
 * (r_for_regulate_normal, config.txt:9) in PCL's queue order, flipping each newly reached normal
 * whose float dot with the normal of the point that reached it is < 0.  normals_inout: n records
 * of stride_bytes (>= 12, multiple of 4); only normal_x/y/z are written.  processed_out
 * (nullable): n bytes, 1 = reached (isProcessed).  seed_idx < 0 is PCL's "invalid point index":
 * DLG_OK, nothing changed, *n_processed = 0. */
dlg_status dlg_regulate_normals(dlg_ctx* ctx, const dlg_points* pts, float* normals_inout,
                                int64_t stride_bytes, int64_t seed_idx, int seed_is_outward,
                                float radius, uint8_t* processed_out, int64_t* n_processed);

/* regulateNormal() first-round branch on a cloud's device copy and the normals attached to it
 * (dlg_cloud_estimate_normals or dlg_cloud_set_normals): the same BFS as dlg_regulate_normals
 * over the cloud's uploaded points, with no host round trip; the flipped normals replace the
 * attached ones (so a following SACMODEL_NORMAL_PLANE extraction uses them) and the cloud is
 * reset.  seed_idx indexes the cloud's points (upload order; with setIndices, the index list's
 * order).  processed_out (nullable): one byte per point; normals_out (nullable): the regulated
 * normals, stride 16 (x, y, z, curvature) or >= 32 (pcl::Normal).  One rank only. */
dlg_status dlg_cloud_regulate_normals(dlg_ctx* ctx, dlg_cloud* cloud, int64_t seed_idx,
                                      int seed_is_outward, float radius, uint8_t* processed_out,
                                      int64_t* n_processed, float* normals_out,
                                      int64_t out_stride_bytes);

/* regulateNormal() later-round branch (PlaneDetect.h:553-584, !isFirstPostProcess): each point
 * of pts takes the orientation of its nearest neighbour in the backup cloud ref_pts
 * (KdTreeFLANN::nearestKSearch k = 1; equidistant neighbours -> lowest index): its normal flips
 * when Vector3f(n).dot(Vector3f(n_ref)) < 0.  Only normal_x/y/z of normals_inout are written. */
dlg_status dlg_orient_normals_nn(dlg_ctx* ctx, const dlg_points* pts, float* normals_inout,
                                 int64_t stride_bytes, const dlg_points* ref_pts,
                                 const float* ref_normals, int64_t ref_stride_bytes);

/* ---- preprocessing (Dialog/PlaneDetect.h:448-512, PCLViewer.cpp:781-805) -------------------- */
/* preProcess(): pcl::removeNaNFromPointCloud, then (translate != 0) the translation of the cloud
 * to its centroid (sequential float sums / float(n), as the reference; translation[3] receives
 * it), then the redundancy removal: walking the points in order, a point is kept unless an
 * already kept point lies within min_dist (KdTreeFLANN radius test), i.e. the index-ordered
 * maximal independent set of the radius graph.  out_xyz: the kept (translated) points in input
 * order, records of out_stride_bytes (12 = xyz, 16 = pcl::PointXYZ with pad 1.0); out_index: their
 * input index.  *n_out = kept points (also on DLG_ERR_CAPACITY when cap is too small).  With
 * translate = 0 this is on_removeRedundantPointsAction_triggered (PCLViewer.cpp:781-805). */
dlg_status dlg_preprocess(dlg_ctx* ctx, const dlg_points* pts, int translate, float min_dist,
                          float* out_xyz, int64_t out_stride_bytes, int32_t* out_index,
                          int64_t cap, int64_t* n_out, float translation[3]);

/* ---- voxel-grid downsampling (Dialog/PCLViewer.cpp:245-253, 283-300, 313-332) ---------------- */
/* pcl::VoxelGrid<pcl::PointXYZ>::filter: the cloud replaced by one point per occupied voxel of a
 * grid with edge lengths leaf[], the centroid of the voxel's points.  PCL 1.8's applyFilter
 * restated from memory (parity unpinned); all arithmetic float, no contraction.
 * The list is indices[0..n_indices) (setIndices; any order, duplicates allowed) or 0..n-1:
 *   inv[a] = 1.0f / leaf[a]; entries with a non-finite x, y or z are skipped everywhere;
 *   min_p / max_p = bounds of the finite entries; no finite entry: 0 voxels, DLG_OK;
 *   (int64)((max_p[a] - min_p[a]) * inv[a]) + 1 multiplied over the axes > INT32_MAX: PCL's "Leaf
 *   size is too small" -> DLG_ERR_INVALID, dlg_last_error "leaf size too small: voxel indices would
 *   overflow" (PCL warns and copies the input through; the C++ shim does that).  A
 *   floorf(min_p * inv) or floorf(max_p * inv) outside the int range: DLG_ERR_INVALID as well;
 *   min_b[a] = (int)floorf(min_p[a] * inv[a]), max_b likewise, div[a] = max_b[a] - min_b[a] + 1;
 *   key = ijk0 + ijk1 * div0 + ijk2 * div0 * div1 in unsigned 32-bit arithmetic, ijk[a] =
 *   (int)(floorf(p[a] * inv[a]) - (float)min_b[a]);
 *   the entries sorted by key; PCL's std::sort leaves the order inside a voxel unspecified, here
 *   it is list order (a stable sort) -- sums over voxels of more than two points depend on it;
 *   voxels of fewer than min_points_per_voxel entries are dropped;
 *   each kept voxel, in key order: s = (0, 0, 0); s[a] += p[a] over its entries in that order
 *   (three sequential float chains); out[a] = s[a] / (float)count.
 * out_xyz: cap records of out_stride_bytes (12 = xyz, 16 = pcl::PointXYZ with pad 1.0f);
 * counts_out (nullable): cap entries, the points of each output voxel; voxel_of_entry (nullable):
 * one per list entry, its output row, or -1 when the entry is non-finite or its voxel was dropped
 * (written whenever the call returns DLG_OK).  *n_out = output voxels, also on DLG_ERR_CAPACITY
 * (cap too small: no output is written).  An index outside [0, pts->n), n_indices or pts->n above
 * INT32_MAX, a leaf that is not finite and > 0, min_points_per_voxel < 0: DLG_ERR_INVALID.  One
 * rank only: on a context of a communicator with world > 1 the points are one rank's shard, whose
 * voxels at the cut would lose the members on other ranks (as dlg_cloud_estimate_normals):
 * DLG_ERR_INVALID. */
typedef struct {
  float leaf[3];                /* setLeafSize; each finite and > 0, else DLG_ERR_INVALID */
  int32_t min_points_per_voxel; /* setMinimumPointsNumberPerVoxel, >= 0 */
} dlg_voxel_params;             /* dlg_abi_struct_size(6) */

typedef struct {
  int64_t n_finite;      /* entries that took part */
  int64_t n_voxels;      /* occupied voxels before the min_points filter */
  int32_t div[3];        /* div_b */
  int32_t min_b[3];
  double  device_ms;     /* HIP events around the call's device work, from the first kernel to the
                            last (the host copies in and out excluded, the two small read-backs
                            between included), when profiling is on; else 0 */
} dlg_voxel_stats;       /* dlg_abi_struct_size(7) */

dlg_status dlg_voxel_grid(dlg_ctx* ctx, const dlg_points* pts, const int32_t* indices,
                          int64_t n_indices, const dlg_voxel_params* params, float* out_xyz,
                          int64_t out_stride_bytes, int64_t cap, int64_t* n_out,
                          int32_t* counts_out, int32_t* voxel_of_entry, dlg_voxel_stats* stats);
/* The same filter with the result left on the device: *out is a cloud equal in every observable
 * way to dlg_cloud_upload (indices NULL, the same id_base) of the points dlg_voxel_grid writes --
 * the same extents, a spatial copy under the same DLG_OPT_PRUNE rule, an equal
 * dlg_cloud_signature, global id = id_base + row -- so normals and planes can be computed on the
 * downsampled cloud with no host round trip, and voxel_of_entry (nullable) maps them back to the
 * input.  min_points_per_voxel applies as above.  stats nullable. */
dlg_status dlg_voxel_grid_cloud(dlg_ctx* ctx, const dlg_points* pts, const int32_t* indices,
                                int64_t n_indices, const dlg_voxel_params* params, int32_t id_base,
                                dlg_cloud** out, int64_t* n_out, int32_t* voxel_of_entry,
                                dlg_voxel_stats* stats);

/* ---- statistical outlier removal (Dialog/PCLViewer.cpp:334-358) ------------------------------ */
/* pcl::StatisticalOutlierRemoval<pcl::PointXYZ>::filter.  PCL 1.8's applyFilterIndices restated
 * (from memory: parity unpinned) over the list indices[0..n_indices) (any
 * order, duplicates allowed; NULL: 0..n-1):
 *   the search structure holds every finite point of the cloud, listed or not;
 *   a list entry with a non-finite coordinate: distances[e] = 0.0f, not counted as valid;
 *   otherwise d2[0..mean_k] = the mean_k + 1 smallest KdTreeFLANN squared distances (float,
 *   ((0 + dx^2) + dy^2) + dz^2) from the entry to the finite points, ascending; d2[0] (the entry
 *   itself or a duplicate) is dropped; double s = 0; s += (double)sqrtf(d2[k]) for k = 1..mean_k;
 *   distances[e] = (float)(s / (double)mean_k);
 *   double sum, sq_sum over the list in order: sum += d, sq_sum += (double)(d * d) (a float product);
 *   mean = sum / valid; variance = (sq_sum - sum * sum / valid) / (valid - 1);
 *   threshold = mean + stddev_mul * sqrt(variance), all double (one valid entry: inf or NaN, as PCL);
 *   entry e is removed when (double)distances[e] > threshold (negative != 0: when it is <=);
 *   kept_out / removed_out: the index values of the kept / removed entries in list order.
 * A NaN threshold removes nothing; non-finite entries (distance 0) are kept whenever
 * threshold >= 0.  Where PCL reads past FLANN's result -- fewer than mean_k + 1 finite points --
 * the call returns DLG_ERR_INVALID ("fewer than mean_k + 1 finite points"), whatever the list (an
 * empty list over a cloud with enough finite points is DLG_OK with nothing kept).  Also DLG_ERR_INVALID:
 * mean_k outside 1..255, a non-finite stddev_mul, an index outside [0, n), n or n_indices above
 * INT32_MAX, a context of a communicator with world > 1 (one rank's shard lacks the neighbours
 * across the cut, as dlg_cloud_estimate_normals).  *n_kept and *n_removed are set on
 * DLG_ERR_CAPACITY too (a buffer too small for its list: nothing is written to it).
 * removed_out, n_removed, distances_out (one float per list entry) and stats are nullable. */
typedef struct {
  int32_t mean_k;    /* setMeanK, 1..255 */
  int32_t negative;  /* setNegative */
  double stddev_mul; /* setStddevMulThresh, finite */
} dlg_sor_params;    /* dlg_abi_struct_size(8) */

typedef struct {
  int64_t n_finite, n_valid;  /* finite points of the cloud; valid list entries */
  double sum, sq_sum, mean, stddev, threshold;
  int64_t literal_queries;    /* queries whose distance sum took the literal loop */
  int32_t exact_sums;         /* 1: the two statistics sums were certified on the device;
                                 0: literal host loop */
  double device_ms;           /* HIP events around the call's device work when profiling is on
                                 (the copies in and out excluded, the small read-backs between
                                 included); else 0 */
} dlg_sor_stats;              /* dlg_abi_struct_size(9) */

dlg_status dlg_statistical_outlier_removal(dlg_ctx* ctx, const dlg_points* pts,
                                           const int32_t* indices, int64_t n_indices,
                                           const dlg_sor_params* params, int32_t* kept_out,
                                           int64_t cap, int64_t* n_kept, int32_t* removed_out,
                                           int64_t cap_removed, int64_t* n_removed,
                                           float* distances_out, dlg_sor_stats* stats);
/* The same filter with the kept points left on the device: *out is a cloud equal in every
 * observable way to dlg_cloud_upload (indices NULL, the same id_base) of the kept points in list
 * order -- extents, the spatial copy under the same DLG_OPT_PRUNE rule, dlg_cloud_signature, global
 * id = id_base + row.  kept_out (nullable): room for one entry per list entry. */
dlg_status dlg_statistical_outlier_removal_cloud(dlg_ctx* ctx, const dlg_points* pts,
                                                 const int32_t* indices, int64_t n_indices,
                                                 const dlg_sor_params* params, int32_t id_base,
                                                 dlg_cloud** out, int64_t* n_kept,
                                                 int32_t* kept_out, dlg_sor_stats* stats);

/* ---- moving least squares (Dialog/PCLViewer.cpp:387-423, "rebuild plane") --------------------- */
/* pcl::MovingLeastSquares<pcl::PointXYZ, pcl::PointNormal>::process with upsampling NONE.  PCL
 * 1.8's computeMLSPointNormal restated (from memory: parity unpinned) over the
 * list indices[0..n_indices) (any order, duplicates allowed; NULL: 0..n-1).  All arithmetic double
 * unless marked float:
 *   the search structure holds every finite point of the cloud, listed or not;
 *   a list entry with a non-finite coordinate gives no output row (PCL asserts there);
 *   the neighbours of a query q: KdTreeFLANN's radius search, float ((0 + dx^2) + dy^2) + dz^2 <
 *   (float)((double)r * (double)r), q included; fewer than 3: no output row;
 *   centroid = (sum p) / m; C = sum (p - centroid)(p - centroid)^T, unnormalised;
 *   (lambda, n) = pcl::eigen33(C); d = -(n . centroid); dist = q . n + d; point = q - dist n;
 *   curvature = trace(C), non-zero: |lambda / trace|, cast to float;
 *   polynomial_fit != 0 and m >= nr_coeff = (order + 1)(order + 2) / 2: v = n.unitOrthogonal()
 *   (Eigen), u = n x v; per neighbour de = p - point, sq = (float)(de . de), w = exp(-(double)sq /
 *   sqr_gauss_param), uc = de . u, vc = de . v, f = de . n, t_j = uc^ui vc^vi (ui = 0..order, vi =
 *   0..order - ui); A = sum (t w) t^T, b = sum (t w) f; c = A.llt().solve(b) with no success check
 *   (Eigen's unblocked Cholesky stops at the first pivot <= 0; the solves run over what it left);
 *   isfinite(c[0]): point += c[0] n and normal = n - c[order + 1] u - c[1] v, not normalised (PCL
 *   1.8); otherwise the projected point and n stand.
 * The order of the sums over the neighbours is not part of the contract.
 * Output rows in list order: out_xyz (records of out_stride_bytes: 12 = xyz, 16 = pcl::PointXYZ with
 * pad 1.0f), out_normals (nullable; 16-byte rows nx, ny, nz, curvature; all zero when
 * compute_normals == 0), src_index (nullable; the row's index value, getCorrespondingIndices);
 * neighbours (nullable): one per list entry, its neighbour count, -1 for a non-finite entry.
 * *n_out = rows, also on DLG_ERR_CAPACITY (cap too small: no output row is written).
 * DLG_ERR_INVALID: polynomial_order outside 1..3, a search_radius that is not finite and > 0, an
 * index outside [0, n), n or n_indices above INT32_MAX, a context of a communicator with world > 1
 * (one rank's shard lacks the neighbours across the cut). */
typedef struct {
  float search_radius;      /* setSearchRadius; finite and > 0 */
  int32_t polynomial_fit;   /* setPolynomialFit */
  int32_t polynomial_order; /* setPolynomialOrder, 1..3 (PCL's default: 2) */
  int32_t compute_normals;  /* setComputeNormals */
  double sqr_gauss_param;   /* setSqrGaussParam; <= 0: search_radius^2 (PCL's default) */
} dlg_mls_params;           /* dlg_abi_struct_size(10) */

typedef struct {
  int64_t n_finite;         /* finite points of the cloud */
  int64_t n_out;            /* output rows */
  int64_t n_too_few;        /* finite list entries with fewer than 3 neighbours (no row) */
  int64_t n_plane_only;     /* rows without a polynomial fit (polynomial_fit off or m < nr_coeff) */
  int64_t n_fit_nonfinite;  /* rows whose fit gave a non-finite c[0]: the projection stands */
  int64_t max_neighbours;   /* the largest neighbour count of a finite list entry */
  int64_t n_lds_overflow;   /* finite list entries whose neighbours were read again from the grid
                               (more than the kernel's on-chip buffer holds) */
  double device_ms;         /* HIP events around the call's device work when profiling is on (the
                               copies in and out excluded, the small read-backs between included) */
} dlg_mls_stats;            /* dlg_abi_struct_size(11) */

dlg_status dlg_moving_least_squares(dlg_ctx* ctx, const dlg_points* pts, const int32_t* indices,
                                    int64_t n_indices, const dlg_mls_params* params, float* out_xyz,
                                    int64_t out_stride_bytes, float* out_normals, int64_t cap,
                                    int64_t* n_out, int32_t* src_index, int32_t* neighbours,
                                    dlg_mls_stats* stats);
/* The same filter with the result left on the device: *out is a cloud equal in every observable way
 * to dlg_cloud_upload (indices NULL, the same id_base) of the rows dlg_moving_least_squares writes,
 * and with compute_normals != 0 its normals are attached as dlg_cloud_set_normals would attach
 * out_normals, so dlg_extract_planes can run (SACMODEL_NORMAL_PLANE too) with no host round trip.
 * src_index (nullable): room for one entry per list entry. */
dlg_status dlg_moving_least_squares_cloud(dlg_ctx* ctx, const dlg_points* pts,
                                          const int32_t* indices, int64_t n_indices,
                                          const dlg_mls_params* params, int32_t id_base,
                                          dlg_cloud** out, int64_t* n_out, int32_t* src_index,
                                          dlg_mls_stats* stats);

/* ---- rigid registration (Dialog/PCLViewer.cpp:581-636, "registration ICP") ------------------- */
/* pcl::IterativeClosestPoint<PointXYZ, PointXYZ>::align(output, guess) of PCL 1.8, restated (from
 * memory: parity unpinned) with no reciprocal correspondences and no RANSAC
 * rejector; min_number_correspondences is 3.
 *   Source: the list indices[0..n_indices) over src (any order, duplicates allowed; NULL: 0..n-1);
 *   the target search structure holds every finite target point.  final = guess (NULL: identity);
 *   the working cloud W = the listed source points, moved by guess unless it is bit-equal to the
 *   identity.  A point through a row-major 4x4 m, in float without contraction:
 *   x' = ((m00 x + m01 y) + m02 z) + m03, y' and z' alike.
 *   One iteration:
 *   1. every W entry with finite coordinates pairs with its nearest finite target point, float
 *      d2 = ((0 + dx^2) + dy^2) + dz^2 (FLANN), equal distances to the lowest index; the pair is
 *      dropped when (double)d2 > max_dist^2 (double; a product above DBL_MAX counts as DBL_MAX).
 *      Fewer than 3 pairs: state NO_CORRESPONDENCES, converged = 0, W and final stay.
 *   2. exact integer moments of the pairs (csrc/icp_model.hpp): e = the binary exponent with
 *      F < 2^e, F the larger of the target's and W's largest finite |coordinate|;
 *      q(v) = trunc(v 2^(48 - e)); m, S_a = sum q(w_a), T_a = sum q(t_a), P_ab = sum q(w_a) q(t_b);
 *      M_ab = RN(m P_ab - S_a T_b), cs_a = RN(S_a) / m 2^(e - 48), ct alike.  No visiting order,
 *      grouping or launch shape shows in any bit.
 *   3. R by Horn's closed form on M (double + - * / sqrt only: a fixed cyclic Jacobi on the 4x4
 *      N(M)), t = ct - R cs; T = (R | t) cast to float.
 *   4. W <- T W; final <- T final (float 4x4 product, each entry's four products summed left to
 *      right); ++iterations.
 *   5. DefaultConvergenceCriteria in this order: iterations >= max_iterations -> ITERATIONS;
 *      0.5 (T00 + T11 + T22 - 1) >= 1 - transformation_epsilon and |t|^2 <= transformation_epsilon
 *      -> TRANSFORM; |mse - prev| < 1e-12 -> ABS_MSE; |mse - prev| / prev <
 *      euclidean_fitness_epsilon -> REL_MSE; else prev = mse (DBL_MAX at first) and the loop goes
 *      on.  mse = RN(D) / m 2^(e2 - 48), D = sum trunc(d2 2^(48 - e2)), e2 the exponent of the
 *      iteration's largest kept d2.  The similar-transform counter of PCL is left out.
 *   getFitnessScore(fitness_max_range) when compute_fitness != 0: one more correspondence pass of
 *   the final W keeping d2 <= max_range, summed as the mse is; DBL_MAX when nothing is kept (a NaN
 *   or a negative max_range keeps nothing).
 * DLG_ERR_INVALID: a context of a communicator with world > 1 (one rank's target shard lacks the
 * neighbours beyond its cut), an index outside [0, n), n, n_indices or the target's n above
 * INT32_MAX, a target with no finite point, max_iterations < 1, a non-finite guess, a
 * max_correspondence_distance that is NaN or <= 0. */
enum {
  DLG_ICP_NOT_CONVERGED = 0,
  DLG_ICP_ITERATIONS = 1,
  DLG_ICP_TRANSFORM = 2,
  DLG_ICP_ABS_MSE = 3,
  DLG_ICP_REL_MSE = 4,
  DLG_ICP_NO_CORRESPONDENCES = 5
};

typedef struct {
  int32_t max_iterations;             /* setMaximumIterations (10) */
  int32_t compute_fitness;            /* != 0: stats->fitness = getFitnessScore(fitness_max_range) */
  double max_correspondence_distance; /* setMaxCorrespondenceDistance (sqrt(DBL_MAX)) */
  double transformation_epsilon;      /* setTransformationEpsilon (0) */
  double euclidean_fitness_epsilon;   /* setEuclideanFitnessEpsilon (-DBL_MAX) */
  double fitness_max_range;           /* getFitnessScore's max_range (DBL_MAX) */
} dlg_icp_params;                     /* dlg_abi_struct_size(13) */

typedef struct {
  int32_t iterations;       /* nr_iterations_ */
  int32_t converged;        /* hasConverged */
  int32_t state;            /* DLG_ICP_* (getConvergeCriteria()->getConvergenceState()) */
  int32_t levels;           /* hierarchy levels a query of the call reached */
  int64_t n_corr;           /* pairs of the last correspondence pass of the loop */
  int64_t n_src_finite;     /* list entries whose source point is finite */
  int64_t n_tgt_finite;     /* finite target points */
  int64_t host_syncs;       /* stream synchronisations inside the iteration loop */
  double mse;               /* of the last iteration */
  double fitness;           /* compute_fitness != 0, else 0 */
  double build_ms;          /* profiling: the one-off target hierarchy build (its read-backs included) */
  double device_ms;         /* HIP events around the call's device work after the build when
                               profiling is on (the copies in and out excluded, the small
                               read-backs between included) */
} dlg_icp_stats;            /* dlg_abi_struct_size(14) */

typedef struct {
  int64_t n_corr;
  double mse;
  int32_t e, e2;
  float T[16];              /* the iteration's transformation, row-major */
} dlg_icp_iteration;        /* dlg_abi_struct_size(15) */

void dlg_icp_params_default(dlg_icp_params* p);
/* guess (nullable): row-major 4x4.  final_out: 16 floats.  aligned_out (nullable): W, one record of
 * out_stride_bytes (12, or 16 with pad 1.0f) per list entry.  history_out (nullable): one record
 * per iteration, the first history_cap of them. */
dlg_status dlg_icp_align(dlg_ctx* ctx, const dlg_points* src, const int32_t* indices,
                         int64_t n_indices, const dlg_points* tgt, const dlg_icp_params* params,
                         const float* guess, float* final_out, float* aligned_out,
                         int64_t out_stride_bytes, dlg_icp_iteration* history_out,
                         int64_t history_cap, dlg_icp_stats* stats);
/* CorrespondenceEstimation::determineCorrespondences by the kernel the iteration runs: per list
 * entry (moved by transform unless it is NULL or bit-equal to the identity) nn_out = the target
 * index and d2_out, or -1 and 0 for a dropped or non-finite entry; *n_corr = the pairs kept. */
dlg_status dlg_icp_correspondences(dlg_ctx* ctx, const dlg_points* src, const int32_t* indices,
                                   int64_t n_indices, const dlg_points* tgt, const float* transform,
                                   double max_dist, int32_t* nn_out, float* d2_out,
                                   int64_t* n_corr);

/* ---- FPFH descriptors (Dialog/PCLViewer.cpp:524-543, "registration" before SAC-IA) ------------ */
/* pcl::FPFHEstimation<pcl::PointXYZ, pcl::Normal, pcl::FPFHSignature33>::compute with
 * setRadiusSearch, the search surface being the input cloud, over the list indices[0..n_indices)
 * (any order, duplicates allowed; NULL: 0..n-1).  PCL 1.8's computePairFeatures,
 * computePointSPFHSignature and weightPointSPFHSignature restated (from memory: parity unpinned,
 * DESIGN.md section 2).  All arithmetic float unless marked double:
 *   the search structure holds every finite point of the cloud, listed or not;
 *   the neighbours of a point: KdTreeFLANN's radius search, float ((0 + dx^2) + dy^2) + dz^2 <
 *   (float)((double)r * (double)r), the point included, in (d2, index) order; m = their number;
 *   pair features of (p, n_p) = the SPFH's own point and (q, n_q) = a neighbour: d = q - p, f4 =
 *   sqrt((dx^2 + dy^2) + dz^2), 0: the pair fails; a1 = (n_p . d) / f4, a2 = (n_q . d) / f4 (dots
 *   summed left to right); acos(|a1|) > acos(|a2|): u = n_q, t = n_p, d = -d, f3 = -a2, otherwise
 *   u = n_p, t = n_q, f3 = a1; v = d x u, |v| = sqrt of its squared norm, 0: the pair fails;
 *   v /= |v|; w = u x v; f2 = v . t; f1 = atan2(w . t, u . t);
 *   acos and atan2 are the correctly rounded floats of the real functions (the one definition that
 *   does not depend on a maths library; unpinned against PCL's libm);
 *   SPFH of a point, three 11-bin histograms: incr = 100.0f / float(m - 1); every neighbour other
 *   than the point itself (by index) whose pair does not fail adds incr to bin
 *   floor(11 ((f1 + M_PI) d_pi)), floor(11 ((f2 + 1.0) 0.5)) and floor(11 ((f3 + 1.0) 0.5)) of the
 *   three (double; d_pi = 1.0f / (2.0f * float(M_PI)); clamped to 0..10, a NaN to 0): a bin's value
 *   is the c-fold sequential float sum of incr, c = its count.  A pair in which either normal has a
 *   non-finite component adds nothing (PCL casts a NaN to int there: undefined, unpinned);
 *   FPFH of a list entry: its neighbours in (d2, index) order, those with d2 == 0 skipped; w =
 *   1.0f / d2; per bin val = spfh[neighbour][b] * w, hist[b] += val (float), sum_g += val (double,
 *   g = the bin's histogram), neighbour-major and bin-minor; then hist[b] *= (float)(100.0 / sum_g)
 *   for each g with sum_g != 0.
 * normals: one record of normals_stride_bytes (>= 12, a multiple of 4) per point, nx, ny, nz first.
 * hist_out: one record of hist_stride_bytes (>= 132, a multiple of 4) per list entry, 33 floats
 * first (the rest of a record is not written); 33 quiet NaNs for an entry with a non-finite
 * coordinate, 33 zeros for one with no neighbour but itself.  neighbours (nullable): one per list
 * entry, m, -1 for a non-finite entry.  spfh_counts (nullable): n x 33 int32, the integer bin counts
 * of every finite point's SPFH (rows of non-finite points are zero).
 * DLG_ERR_INVALID: a search_radius that is not finite and > 0, an index outside [0, n), n or
 * n_indices above INT32_MAX, null normals, a bad stride, a context of a communicator with world > 1
 * (one rank's shard lacks the neighbours across the cut). */
typedef struct {
  float search_radius;      /* setRadiusSearch; finite and > 0 */
} dlg_fpfh_params;          /* dlg_abi_struct_size(17) */

typedef struct {
  int64_t n_finite;         /* finite points of the cloud */
  int64_t n_nan_rows;       /* list entries with a non-finite coordinate (rows of NaNs) */
  int64_t n_zero_rows;      /* finite list entries with no neighbour but themselves */
  int64_t max_neighbours;   /* the largest neighbour count of a finite list entry */
  int64_t n_lds_overflow;   /* finite list entries with more neighbours than the weighting kernel's
                               on-chip buffer holds (sorted and walked in several windows) */
  int64_t n_pairs;          /* pairs that added to the SPFH of a finite list entry (per entry) */
  int64_t n_pairs_failed;   /* the other neighbours of those entries, themselves excluded: failed
                               pairs and pairs with a non-finite normal */
  int64_t n_sum_literal;    /* finite list entries whose double sums took the literal loop (the
                               exactness certificate of DESIGN.md section 5j missed) */
  double device_ms;         /* HIP events around the call's device work when profiling is on (the
                               copies in and out excluded, the small read-backs between included) */
  double build_ms;          /* ... its parts: the grid build, */
  double spfh_ms;           /*     the SPFH pass (with the gather of the normals), */
  double weight_ms;         /*     the weighting pass */
} dlg_fpfh_stats;           /* dlg_abi_struct_size(18) */

dlg_status dlg_fpfh_estimate(dlg_ctx* ctx, const dlg_points* pts, const float* normals,
                             int64_t normals_stride_bytes, const int32_t* indices,
                             int64_t n_indices, const dlg_fpfh_params* params, float* hist_out,
                             int64_t hist_stride_bytes, int32_t* neighbours, int32_t* spfh_counts,
                             dlg_fpfh_stats* stats);
/* The same descriptors of every point of a cloud's device copy (upload order) with its attached
 * normals (dlg_cloud_set_normals, dlg_cloud_estimate_normals, dlg_cloud_regulate_normals): upload ->
 * normals -> FPFH has no host round trip on the input side.  DLG_ERR_INVALID when no normals are
 * attached. */
dlg_status dlg_cloud_fpfh(dlg_ctx* ctx, dlg_cloud* cloud, const dlg_fpfh_params* params,
                          float* hist_out, int64_t hist_stride_bytes, int32_t* neighbours,
                          dlg_fpfh_stats* stats);

/* ---- SAC-IA initial alignment (Dialog/PCLViewer.cpp:546-558, "registration" before ICP) ------- */
/* pcl::SampleConsensusInitialAlignment<PointXYZ, PointXYZ, FPFHSignature33>::align(output, guess)
 * of PCL 1.8 with the default TruncatedError, restated (from memory: parity unpinned, DESIGN.md
 * section 2; csrc/sacia_model.hpp holds the arithmetic).
 *   final = guess (NULL: identity).  A guess that is not approximately the identity -- in double
 *   from the float entries, sum (g - I)^2 > (double)(0.01f * 0.01f) * min(sum g^2, 4) -- is scored
 *   as iteration 0 and the drawn iterations start at 1.
 *   One iteration, all of whose draws depend on the source coordinates alone:
 *   1. selectSamples: getRandomIndex(n) = (int)(n * (rand() / (RAND_MAX + 1.0))) (double) until
 *      nr_samples indices are accepted; a draw is rejected when it equals an accepted index or when
 *      its float distance sqrtf((dx^2 + dy^2) + dz^2) to an accepted sample is < the call's copy of
 *      min_sample_distance; 3 n consecutive rejections multiply that copy by 0.5f.
 *   2. findSimilarFeatures: per sample, in order, the k_correspondences nearest valid target rows
 *      of its descriptor in (d, index) order, d = FLANN's L2_Simple (r = 0; r += (a_j - b_j) *
 *      (a_j - b_j), j = 0..32, float, no contraction); one getRandomIndex(k) picks the rank.
 *   3. the rigid estimate of the nr_samples pairs: the exact integer moments of dlg_icp_align
 *      (e = the exponent of the pairs' largest |coordinate|), Horn's closed form, t = ct - R cs,
 *      cast to float.  PCL's float umeyama is not used.
 *   4. the error: per source point moved through T (as dlg_icp_align moves one), e = the squared
 *      distance to the nearest valid target point (ties cannot show), term = e <= thr ? e / thr :
 *      1.0f with thr = (float)max_correspondence_distance (out of range: +inf; compared with the
 *      SQUARED distance, as PCL does; a NaN term counts as 1.0f), E = sum trunc(term 2^48), an exact
 *      integer: no visiting order, batch size or launch shape shows in any bit.  A source point that
 *      is not finite before or after the transformation adds nothing.
 *   5. the hypothesis is adopted when nothing has been scored yet or E is strictly below the lowest
 *      E so far; adopting sets converged.
 *   A target row is valid when its point and its 33 descriptor values are finite.  A draw that
 *   lands on a source point or a source row that is not finite is still a draw, and the rank draws
 *   are consumed; the hypothesis is invalid: not searched, not estimated, never adopted.
 *   With PCL's default max_correspondence_distance thr is +inf, every E is 0 and the result is the
 *   first valid hypothesis: the reference's own configuration (it sets no distance).
 *   rand() is glibc's (rng 0) or the Visual C++ runtime's (rng 1), seeded with seed (PCL never
 *   calls srand: 1).
 * DLG_ERR_INVALID: nr_samples > n_src, a parameter outside its range, a bad stride, null features,
 * a non-finite guess, a max_correspondence_distance that is NaN or <= 0, fewer than
 * k_correspondences valid target rows, a context of a communicator with world > 1, a count above
 * INT32_MAX. */
typedef struct {
  int32_t max_iterations;      /* setMaximumIterations (1000); >= 0 */
  int32_t nr_samples;          /* setNumberOfSamples (3); 3..8 */
  int32_t k_correspondences;   /* setCorrespondenceRandomness (10); 1..32 */
  int32_t rng;                 /* 0 glibc rand(), 1 MSVC rand() */
  uint32_t seed;               /* srand (1) */
  int32_t compute_fitness;     /* != 0: stats->fitness = getFitnessScore(fitness_max_range) */
  int32_t batch;               /* tests only: hypotheses per scoring launch (0: the library's choice) */
  int32_t max_blocks;          /* tests only: n >= 1 = at most n workgroups per scoring launch */
  float min_sample_distance;   /* setMinSampleDistance (0) */
  double max_correspondence_distance; /* setMaxCorrespondenceDistance (sqrt(DBL_MAX)) */
  double fitness_max_range;    /* getFitnessScore's max_range (DBL_MAX) */
} dlg_sac_ia_params;           /* dlg_abi_struct_size(19) */

typedef struct {
  int32_t sample[8];           /* the source indices drawn (-1: unused slots, the scored guess) */
  int32_t match[8];            /* the target rows picked (-1: unused, invalid) */
  int32_t rank[8];             /* the ranks drawn (-1: unused) */
  int32_t valid;               /* 0: a sample or its row was not finite */
  int32_t relaxations;         /* halvings of min_sample_distance in this iteration */
  int64_t draws;               /* rand() calls of this iteration */
  float T[16];                 /* row-major; zero when invalid */
  uint64_t err_hi, err_lo;     /* E = err_hi 2^24 + err_lo, err_lo < 2^24 */
  int64_t n_far;               /* terms that were 1.0f */
  int64_t n_used;              /* source points that added a term */
} dlg_sac_ia_hypothesis;       /* dlg_abi_struct_size(20) */

typedef struct {
  int32_t iterations;          /* records: the scored guess and the drawn iterations */
  int32_t converged;           /* hasConverged: a hypothesis was adopted */
  int32_t best_iteration;      /* the adopted record (-1: none, final = guess) */
  int32_t n_valid, n_invalid;  /* drawn hypotheses */
  int32_t batches;             /* scoring batches */
  int32_t levels;              /* hierarchy levels a pair of the call reached */
  int32_t reserved;
  int64_t draws, relaxations;  /* over every iteration */
  int64_t n_queries;           /* distinct source descriptors searched */
  int64_t host_syncs;          /* stream synchronisations after the target hierarchy's build */
  double error;                /* RN(E) 2^-48 of the lowest scored hypothesis (0: none) */
  double fitness;              /* compute_fitness != 0, else 0 */
  double build_ms;             /* profiling: the target hierarchy's build (its read-backs included) */
  double knn_ms, score_ms;     /* profiling: HIP events around the descriptor search, the scoring */
  double device_ms;            /* their sum */
} dlg_sac_ia_stats;            /* dlg_abi_struct_size(21) */

void dlg_sac_ia_params_default(dlg_sac_ia_params* p);
/* KdTreeFLANN<FPFHSignature33>::nearestKSearch by the kernel dlg_sac_ia_align runs: per query (33
 * floats first in a record of q_stride_bytes) the k (1..32) nearest rows with 33 finite values, in
 * (d, index) order: idx_out and d_out are n_queries x k.  A query with a non-finite value gets -1
 * and 0.  DLG_ERR_INVALID when fewer than k rows are valid, a stride < 132 or no multiple of 4. */
dlg_status dlg_fpfh_knn(dlg_ctx* ctx, const float* queries, int64_t q_stride_bytes,
                        int64_t n_queries, const float* rows, int64_t row_stride_bytes,
                        int64_t n_rows, int32_t k, int32_t* idx_out, float* d_out);
/* computeErrorMetric of the caller's n_transforms row-major 4x4 transformations by the kernels
 * dlg_sac_ia_align runs; every finite target point is valid.  hyp_out: one record each, of which
 * T, err_hi, err_lo, n_far and n_used are filled (valid = 1, the rest as for a scored guess).
 * batch, max_blocks: as in dlg_sac_ia_params. */
dlg_status dlg_sac_ia_score(dlg_ctx* ctx, const dlg_points* src, const dlg_points* tgt,
                            const float* transforms, int64_t n_transforms,
                            double max_correspondence_distance, int32_t batch, int32_t max_blocks,
                            dlg_sac_ia_hypothesis* hyp_out);
/* src_features / tgt_features: one record of *_feat_stride bytes (>= 132, a multiple of 4) per
 * point, 33 floats first.  guess (nullable), final_out, aligned_out (nullable; final applied to
 * every source point) and out_stride_bytes as in dlg_icp_align.  hyp_out (nullable): the first
 * hyp_cap records; the scored guess is record 0 with draws = 0 and sample = -1. */
dlg_status dlg_sac_ia_align(dlg_ctx* ctx, const dlg_points* src, const float* src_features,
                            int64_t src_feat_stride, const dlg_points* tgt,
                            const float* tgt_features, int64_t tgt_feat_stride,
                            const dlg_sac_ia_params* params, const float* guess, float* final_out,
                            float* aligned_out, int64_t out_stride_bytes,
                            dlg_sac_ia_hypothesis* hyp_out, int64_t hyp_cap,
                            dlg_sac_ia_stats* stats);

/* ---- Gaussian-sphere plane seeds (Dialog/PlaneDetect.h:667-1015) ----------------------------- */
/* The reference's plane detector up to the seed planes: createPS -> voteForPS -> filtPS ->
 * createGradientField -> rectifySinkFields -> segmentPlanes (called from PCLViewer.cpp:887-960 and
 * :1133-1151); growPlaneArea and mergePlanes are not part of it.
 *   parameter space (PS): the lattice cubes of edge num_res in [-1, 1)^3 (floor(2 / num_res + 0.5)
 *   per axis) whose 8 float corner norms straddle 1; the PS index is the enumeration order, x
 *   outer, z inner; a cell's point is its min corner (float)i * num_res - 1.
 *   vote: per point the query floor(n / num_res) * num_res per component; the vote goes to the PS
 *   cell of the smallest (FLANN float d2, index) over all cells.  A point whose normal has a
 *   non-finite component casts no vote (cell -1).
 *   filter: per PS cell, over the cells with d2 < (float)((double)r * r), r = (float)(3.0 *
 *   std_dev_gaussian), in (d2, index) order, G += (float)(C / A) * (float)vote as a sequential
 *   float sum (A, C in double with the reference's float PI and e, d = sqrtf(d2)); the new vote is
 *   (int)floor(G + 0.5f).
 *   gradient field, sinks: on the host over the filtered votes, by the reference's rules; vote_num
 *   sums raw votes; a sink is kept iff vote_num > t_vote_num.  The rectification's sine is the
 *   double sine rounded to float.
 *   seed planes: a point with finite coordinates carries its cell's sink; per sink with at least
 *   t_num_of_single_plane points, the connected components of the radius graph
 *   (search_radius_for_plane_seg) of its points.  The reference's BFS pushes every point of a
 *   component but its seed twice before it tests the size, so a component of m points is kept iff
 *   2 m - 1 >= t_num_of_single_plane.  A plane is returned as its distinct cloud indices.  Order:
 *   sinks as found; within a sink its points listed by (PS cell, point index), the components by
 *   their first point in that list, the indices of a plane in list order.
 * DLG_ERR_INVALID: a num_res that is not finite, not > 0, or gives more than 512 lattice cells per
 * axis; a std_dev_gaussian or a radius that is not finite and > 0; a delta_radius that does not
 * end the rectification within 100000 steps; negative thresholds; n above INT32_MAX / 2; a
 * context of a communicator with world > 1 (one rank's shard lacks the votes and the neighbours
 * of the others). */
typedef struct {
  float num_res;                        /* config.txt: 0.01 */
  float std_dev_gaussian;               /* 0.05 */
  float search_radius_create_gradient;  /* 0.03 */
  int32_t t_vote_num;                   /* 500 */
  float radius_base;                    /* 0.03 */
  float delta_radius;                   /* 0.01 */
  float s_threshold;                    /* 0.9 */
  float dev_threshold;                  /* 15.0 (degrees) */
  float search_radius_for_plane_seg;    /* 0.1 */
  int32_t t_num_of_single_plane;        /* 500 */
} dlg_gs_params;                        /* dlg_abi_struct_size(23) */

typedef struct {
  int64_t n_cells;           /* PS cells */
  int64_t n_occupied;        /* PS cells with a raw vote */
  int64_t n_voters;          /* points that cast a vote */
  int64_t n_fallback_votes;  /* of them, by the search of all cells (the box bound failed) */
  int64_t n_filter_pairs;    /* (PS cell, occupied cell within the radius) pairs of the filter */
  int64_t n_sinks;           /* kept sinks */
  int64_t n_planes;
  int64_t n_plane_points;
  double space_ms;           /* host: the parameter space built and uploaded (0 when kept) */
  double vote_ms, filter_ms, segment_ms;  /* profiling: HIP events around the three device phases */
  double host_ms;            /* host: gradient field and sink rectification */
  double device_ms;          /* vote_ms + filter_ms + segment_ms */
} dlg_gs_stats;              /* dlg_abi_struct_size(24) */

/* caller buffers of dlg_gs_segment and the sizes it found (set on DLG_ERR_CAPACITY too, when
 * nothing is written to the buffer that is too small) */
typedef struct {
  int64_t* plane_offsets;  /* planes_cap + 1: plane k owns plane_ids[offsets[k] .. offsets[k + 1]) */
  int64_t planes_cap;
  int32_t* plane_ids;      /* ids_cap cloud indices */
  int64_t ids_cap;
  int32_t* sink_cells;     /* sinks_cap: the kept sinks' PS index, in order */
  int64_t* sink_votes;     /* sinks_cap: their vote_num */
  int64_t sinks_cap;
  int32_t* cell_of_point;  /* nullable, n: the PS cell each point voted for, -1 none */
  int32_t* raw_vote;       /* nullable, n_cells each: voteForPS's count, */
  int32_t* filtered_vote;  /*   filtPS's vote, */
  int32_t* sink_init;      /*   createGradientField's and */
  int32_t* sink;           /*   rectifySinkFields' sink per cell */
  int64_t cells_cap;       /* entries of each of the four (>= n_cells when any is given) */
  int64_t n_planes, n_ids, n_sinks, n_cells;  /* out */
} dlg_gs_result;           /* dlg_abi_struct_size(25) */

void dlg_gs_params_default(dlg_gs_params* p);  /* the config.txt values above */
/* createPS on the host (no context): *n_cells, and with corners_out (cap rows of 3 floats) every
 * cell's min corner in PS order; DLG_ERR_CAPACITY (with *n_cells) when cap is too small. */
dlg_status dlg_gs_space(const dlg_gs_params* params, float* corners_out, int64_t cap,
                        int64_t* n_cells);
/* voteForPS alone: normals are n records of stride_bytes (>= 12, a multiple of 4; x, y, z first);
 * cell_of_point: n entries; votes (nullable): votes_cap >= n_cells entries.  stats (nullable):
 * n_cells, n_occupied, n_voters, n_fallback_votes, vote_ms. */
dlg_status dlg_gs_vote(dlg_ctx* ctx, const float* normals, int64_t n, int64_t stride_bytes,
                       const dlg_gs_params* params, int32_t* cell_of_point, int32_t* votes,
                       int64_t votes_cap, dlg_gs_stats* stats);
dlg_status dlg_gs_segment(dlg_ctx* ctx, const dlg_points* pts, const float* normals,
                          int64_t normals_stride_bytes, const dlg_gs_params* params,
                          dlg_gs_result* result, dlg_gs_stats* stats);
/* The same over a cloud's own device copy (every uploaded point, upload order) and its attached
 * normals as given (dlg_cloud_set_normals, dlg_cloud_estimate_normals, flipped by
 * dlg_cloud_regulate_normals): normals -> RegulateNormal -> seeds has no host round trip on the
 * input side.  DLG_ERR_INVALID when no normals are attached. */
dlg_status dlg_cloud_gs_segment(dlg_ctx* ctx, dlg_cloud* cloud, const dlg_gs_params* params,
                                dlg_gs_result* result, dlg_gs_stats* stats);

/* ---- postProcessPlanes (Dialog/PlaneDetect.h:1454-1579) ------------------------------------ */
/* The final planes (plane_clouds_final, HeaderFile.h:98; struct Plane HeaderFile.h:81-88) as
 * borrowed host arrays: plane k owns points[point_offsets[k] .. point_offsets[k + 1]) (its
 * points_set) and border vertices [border_offsets[k] .. border_offsets[k + 1]) (its border, the
 * ConcaveHull polygon of polyPlanes, PlaneDetect.h:1358-1436), records of *_stride_bytes (12 or
 * >= 16, multiple of 4).  coeffs: 4 floats per plane (coeff.values; only [0..2], the outward
 * normal, is read). */
typedef struct {
  int32_t n_planes;
  const float* coeffs;
  const float* points;
  int64_t points_stride_bytes;
  const int64_t* point_offsets;  /* n_planes + 1 */
  const float* borders;
  int64_t borders_stride_bytes;
  const int64_t* border_offsets; /* n_planes + 1 */
} dlg_planes;

/* config.ini [PlaneDetect] values and the call's state (PlaneDetect.h:86-90, 1453) */
typedef struct {
  float t_dist_point_plane;  /* T_dist_point_plane: isPointInPoly's plane-distance gate */
  float radius_local;        /* radius_local: clusterFilt neighbourhood radius (>= 0) */
  int32_t t_cluster_num;     /* T_cluster_num: clusters of <= this many points are dropped */
  int32_t plane_start_index; /* planes [plane_start_index, n_planes) may absorb points */
  uint32_t rand_seed;        /* the srand(time(0)) value isPointInPoly reseeds rand() with */
} dlg_postprocess_params;

/* polyPlanes() -> polyPointCloud() (PlaneDetect.h:1358-1440) for one plane, so the four-file
 * polygon hand-off (PCLViewer.cpp:1341-1396) can run from RANSAC output alone: the plane's points
 * (its points_set) projected onto their least-squares plane (pcl::computePointNormal, PCL float
 * arithmetic) as projPoint2Plane does, then pcl::ConcaveHull's alpha shape (alpha = alpha_poly,
 * config.txt:28) restated step by step (PCA frame, Delaunay triangulation, circumradius filter,
 * boundary edges, PCL's polygon walk; dialog_amd/csrc/alpha_shape.hpp): the triangles, the alpha
 * filter and the boundary are qhull's ("QJ") on the committed fixtures.  The reference takes
 * polygons[0]; qhull's facet order, which decides that, is unpinned, so the border is the
 * boundary polygon of largest area.  Orientation as the reference: reversed when
 * normalize(normalize(p1 - p0) x normalize(p2 - p1)) . pn < 0.  border_out: up to cap records of
 * out_stride_bytes (>= 12; xyz first); *n_out = vertices (0: fewer than 3 points or no polygon),
 * also reported with DLG_ERR_CAPACITY.  Host arithmetic; no context.  The C++ shim's
 * dialog::polyPointCloud / dialog::polyPlanes wrap it (include/dialog/sac_segmentation.hpp). */
dlg_status dlg_plane_border(const dlg_points* plane_pts, const float pn[3], float alpha,
                            float* border_out, int64_t out_stride_bytes, int64_t cap,
                            int64_t* n_out);

/* PlaneDetect.h:1477-1498: coeffs_out[4k..4k+3] = pcl::computePointNormal of plane k's points
 * (float sums in list order, eigen33, d = -n.centroid; NaN with < 3 points), negated when its
 * dot with the previous normal coeffs[4k..4k+2] is < 0.  Host arithmetic (sequential float sums
 * are sequential by definition); no context needed. */
dlg_status dlg_refit_planes(const dlg_planes* planes, float* coeffs_out);

/* postProcessPlanes() minus its display/bookkeeping: (1) refit as dlg_refit_planes; (2) every
 * plane point marks its nearest cloud point processed (KdTreeFLANN nearestKSearch k = 1, ties ->
 * lowest index); (3) each unprocessed cloud point joins every plane k >= plane_start_index whose
 * isPointInPoly (PlaneDetect.h:1891-1964, after srand(rand_seed)) accepts it; (4) clusterFilt
 * (PlaneDetect.h:1582-1655) on the points still unprocessed.  Outputs: coeffs_out (4 per plane);
 * absorbed_offsets[n_planes + 1] and absorbed_ids: per plane, the ascending cloud indices it
 * absorbed (the shim appends those points to points_set); remaining_ids: ascending cloud indices
 * that form the new source_cloud.  Sizes are reported (absorbed_offsets[n_planes],
 * *n_remaining) also on DLG_ERR_CAPACITY.  A plane taking part in (3) must have >= 1 border
 * vertex (the reference divides by the border size).  Exact duplicate points are assumed absent
 * (preProcess removes them): clusterFilt's "skip the first neighbour" then skips the point
 * itself, and its BFS clusters are the connected components computed here. */
dlg_status dlg_post_process_planes(dlg_ctx* ctx, const dlg_points* cloud, const dlg_planes* planes,
                                   const dlg_postprocess_params* params, float* coeffs_out,
                                   int64_t* absorbed_offsets, int32_t* absorbed_ids,
                                   int64_t absorbed_cap, int32_t* remaining_ids,
                                   int64_t remaining_cap, int64_t* n_remaining);

/* clusterFilt() alone (PlaneDetect.h:1582-1655): ascending indices of the points whose
 * radius-`radius` connected component has more than t_cluster_num points. */
dlg_status dlg_cluster_filter(dlg_ctx* ctx, const dlg_points* pts, float radius,
                              int32_t t_cluster_num, int32_t* kept_ids, int64_t cap,
                              int64_t* n_kept);

/* ---- host-side RANSAC control (no device) ----------------------------------------------------
 * The sequential half of RandomSampleConsensus::computeModel [PCL-1.8 ext] that dlg_sac_segment
 * runs on the host, exported on its own so that a caller with another scorer -- and the
 * multi-rank CPU tests -- drive exactly the replay the GPU path uses:
 *   dlg_sac_control_next    <- SampleConsensusModel::getSamples/drawIndexSample (the RNG and the
 *                              swaps on the persistent shuffled index copy) for the next batch:
 *                              3 list positions per draw into the N_active-long global list;
 *   dlg_sac_control_consume <- computeModel's loop over the batch's (isSampleGood, count) pairs:
 *                              1000 bad draws in a row end it, strict '>' keeps the first best,
 *                              k = log(1-p)/log(1-w^3), the max_iterations break.
 * A batch must be consumed before the next one is drawn.  Point-sharded ranks each run one
 * controller on the global N and the summed counts and so take identical decisions. */
typedef struct dlg_sac_control dlg_sac_control;
dlg_status dlg_sac_control_create(dlg_sac_control** out, const dlg_sac_params* prm,
                                  int64_t n_active_global, int max_batch /* 0 = 4096 */);
dlg_status dlg_sac_control_destroy(dlg_sac_control* ctl);
/* *n_draws = size of the next batch (0 once the loop has ended); DLG_ERR_CAPACITY if
 * cap < 3 * *n_draws (nothing is drawn) */
dlg_status dlg_sac_control_next(dlg_sac_control* ctl, int32_t* positions_out, int64_t cap,
                                int* n_draws);
/* counts/good of the batch just drawn, in draw order; *best_in_batch = draw index of a new best
 * (-1: unchanged), *finished = 1 once computeModel's loop has ended */
dlg_status dlg_sac_control_consume(dlg_sac_control* ctl, const int32_t* counts,
                                   const int32_t* good, int n_draws, int* best_in_batch,
                                   int* finished);
/* iterations, draws, has_model, n_unrefined (best count), n_active, tests; best_draw = global
 * draw index (over all batches) of the winning hypothesis, -1 without a model */
dlg_status dlg_sac_control_result(const dlg_sac_control* ctl, dlg_sac_stats* st,
                                  int64_t* best_draw);

/* The device half of the pair above: countWithinDistance of the caller's draws.  positions:
 * 3 * n_draws positions into the global active list, exactly what dlg_sac_control_next hands out
 * (1 <= n_draws <= 4096; a position outside the list: DLG_ERR_INVALID).  Runs the gather, the
 * hypothesis build and the scoring of a dlg_sac_segment round for prm->model (any of the four)
 * on the path that round would take for this cloud -- the exhaustive, pruned or pruned
 * NORMAL_PLANE scorer, at several ranks the sample and count allreduces or the hypothesis
 * slices -- and leaves the active list as it is.  Per draw, in draw order:
 *   counts_out  inliers of the draw's plane among the active points (all ranks); 0 for a bad
 *               sample and for a plane the axis-constrained models reject
 *   good_out    isSampleGood
 *   valid_out   (nullable) isModelValid: 0 only for a good sample whose plane
 *               DLG_SACMODEL_PERPENDICULAR_PLANE / DLG_SACMODEL_PARALLEL_PLANE reject
 *   coeffs_out  (nullable) 4 floats: computeModelCoefficients, also of a rejected plane; NaN for
 *               a bad sample
 * counts_out and good_out are what dlg_sac_control_consume takes.  Several ranks: every rank
 * calls it with the same positions. */
dlg_status dlg_score_samples(dlg_ctx* ctx, dlg_cloud* cloud, const dlg_sac_params* prm,
                             const int32_t* positions, int n_draws, int32_t* counts_out,
                             int32_t* good_out, int32_t* valid_out, float* coeffs_out);
/* Tests: the verdicts of the axis-constrained models on n values f of the float dot product
 * their test reduces to (perpendicular: axis.normalized() . Cn, parallel: axis . Cn).
 * by_threshold[i]: from the float thresholds the host derives from eps_angle once per call and
 * the device compares against (perpendicular: valid when f >= thresholds[1] or f <=
 * thresholds[0], found by bisection over float bit patterns; parallel: invalid when |f| >
 * thresholds[1], the largest float <= |sin(eps_angle)|); by_formula[i]: from the acos / sin
 * formula of dlg_ctx_set_axis evaluated directly in double.  The two must agree for every f.
 * model: one of the two constrained models.  Host arithmetic; no context. */
dlg_status dlg_axis_verdicts(int model, double eps_angle, const float* f, int64_t n,
                             int32_t* by_threshold, int32_t* by_formula, float thresholds[2]);

/* ---- profiling ------------------------------------------------------------------------------ */
/* Kernel-level HIP-event timing on the context's stream (bench roofline); off by default.
 * enable 1: the scoring launches, the select phase and the PCL refit walk; 2: without the walk's
 * events (each timing event on a dispatch costs the stream a few microseconds). */
dlg_status dlg_set_profiling(dlg_ctx* ctx, int enable);
dlg_status dlg_synchronize(dlg_ctx* ctx);
/* Scoring-kernel micro-benchmark (kernel A/B on the device): D random plane hypotheses through
 * the same gather/build path, `kernel` (DLG_SCORE_EXACT, DLG_SCORE_BF16 or DLG_SCORE_PRUNED, the
 * last needing the cloud's Morton copy) launched `reps` times on the cloud's active points;
 * returns the mean device time per launch and (optional) the counts of the last launch.
 * The draw is fixed, so that a host can replay the hypotheses and check counts_out against
 * PCL's countWithinDistance (tests/test_score_counts_oracle.py): one Mt19937 seeded with 777,
 * rnd() = next() >> 1 as in dlg_sac_control; position i of the 3 * D is (uint32_t)rnd() %
 * n_active, an index into the cloud's active list in list order, three consecutive positions
 * per hypothesis (repeats are not redrawn).  List entry `pos` is point pos of an unindexed cloud
 * as uploaded, point indices[pos] of a cloud uploaded with indices, and after extraction rounds
 * entry pos of the remaining list, which keeps the uploaded order.  counts_out[d] is the number
 * of active points within `threshold` of hypothesis d's plane, 0 when isSampleGood rejects its
 * sample; needs >= 3 active points and 1 <= D <= 4096. */
dlg_status dlg_score_benchmark(dlg_ctx* ctx, dlg_cloud* cloud, int D, int kernel, int reps,
                               double threshold, double* ms_per_launch, int32_t* counts_out);
/* DLG_REFIT_PCL's device refit (fsum.hip) on caller data, for tests and measurement: the nine
 * sequential float sums of pcl::computeMeanAndCovarianceMatrix's dense branch (accu[0..8] =
 * xx, xy, xz, yy, yz, zz, x, y, z in list order) over n points (xyz: 3 floats each), then
 * optimizeModelCoefficients' float eigen33 refit of cin.  sums_out[9] and coeff_out[4] are the
 * device's bits; *uncertain = 1 when an eigen33 transcendental could not be rounded for certain
 * (the extraction then takes the host's value).  reps >= 1 launches are timed: *ms_per_call.
 * walk_stats (optional, the last call's; 8 int64 per chain, several counters packed):
 *   [0] windows walked record by record;
 *   [1] bits 0-31 speculation passes, bits 32-63 table lookups missed: no table built yet;
 *   [2] bits 0-31 passes needing the full lemma, bits 32-63 table lookups missed: lead out of
 *       the table's range;
 *   [3] bits 0-23 chunks stepped alone, bits 24-63 five 8-bit saturating buckets of the missed
 *       leads (|lead| < 128, < 512, < 4096, larger, not an exact multiple of the quantum);
 *   [4] bits 0-31 reruns, bits 32-63 table lookups missed: entry dropped by the builder;
 *   [5] shader clocks of the walk; [6] shader clocks of its integer stepping;
 *   [7] bits 0-31 windows passed by their summaries, bits 32-63 windows passed by a table. */
dlg_status dlg_float_sums(dlg_ctx* ctx, const float* xyz, int64_t n, const float cin[4], int reps,
                          float sums_out[9], float coeff_out[4], int* uncertain,
                          double* ms_per_call, int64_t* walk_stats /* nullable: [9][8] */);
/* Debugging: the bytes this process holds right now in the library's device buffers (pinned == 0)
 * or pinned host buffers (pinned == 1), over all contexts and clouds.  The library's own count, so a
 * test can see a leak on a device it shares with other processes.  No context. */
int64_t dlg_debug_live_bytes(int pinned);
/* Debugging: the absorption step (isPointInPoly) of dlg_post_process_planes alone, up to its
 * vote, so that a test can compare the device's crossing arithmetic ray by ray.  planes->coeffs are used as given (4 floats per
 * plane: no refit, planes->points and point_offsets are not read) and every cloud point counts as
 * unprocessed.  Per plane k, ids[offsets[k] .. offsets[k + 1]) are its candidates (the points
 * within t_dist of their projection on the plane) in ascending order and masks[] their ray
 * parities: bit i set when ray i of isPointInPoly (after srand(rand_seed)) crosses the border an
 * odd number of times; the point is absorbed when >= 5 of the 10 bits are set.  A plane with a
 * non-finite coefficient has an empty range; a plane without border vertices is refused.
 * offsets: n_planes + 1.  *n_needed = offsets[n_planes], also reported with DLG_ERR_CAPACITY
 * (cap < *n_needed: ids and masks are not written). */
dlg_status dlg_debug_pip_masks(dlg_ctx* ctx, const dlg_points* cloud, const dlg_planes* planes,
                               float t_dist, uint32_t rand_seed, int64_t* offsets, int32_t* ids,
                               uint32_t* masks, int64_t cap, int64_t* n_needed);
/* Execution-path options of a context.  Every setting gives identical results (planes, inliers,
 * counts): they only choose among equivalent device paths, for tests and measurement.  There are
 * no environment switches in the library. */
enum {
  DLG_OPT_PRUNE = 1,        /* Morton copy + pruned countWithinDistance: -1 (default) clouds of
                               >= 131072 points, 0 never, 1 every cloud (applies at upload) */
  DLG_OPT_LEAN_ROUNDS = 2,  /* 1 (default): single-pass selects driven by the Morton copy in
                               SACMODEL_PLANE extraction, in every refit mode and at any rank
                               count (PCL refit on N > 1 ranks: each rank walks its shard's float
                               chains); 0: two-pass */
  DLG_OPT_SPEC_PICK = 3,    /* 1 (default): device-side computeModel decision for probability-1
                               rounds (host replay confirms it); 0: host decision only */
  DLG_OPT_PRUNE_NP = 4,     /* 1 (default): pruned SACMODEL_NORMAL_PLANE scoring; 0: exhaustive */
  DLG_OPT_SCORE_KERNEL = 5, /* exhaustive scorer (no Morton copy): DLG_SCORE_BF16 (default) or
                               DLG_SCORE_EXACT */
  DLG_OPT_PRUNE_STATS = 6,  /* 1: count the pruned kernel's work (dlg_prune_stats); 0 (default) */
  DLG_OPT_SELECT_TILE = 7,  /* points per tile of the lean rounds' single-pass selects: 4096,
                               8192 or 16384 (default) */
  DLG_OPT_PCL_REFIT_DEVICE = 8, /* DLG_REFIT_PCL: 1 (default) the float sums on the
                               device, exact (fsum.hpp); 0 gathered and summed on the host; 2 as 1,
                               the host recomputing every refit's tail from the sums; 3 as 2 and
                               every round's select redone with the host's plane (test) */
  DLG_OPT_PRUNE_TILE_SCORER = 9, /* the pruned plane scorer's (tile, plane) pairs:
                               DLG_TILE_EXACT (default) PCL-order f32 with lanes as planes, or
                               DLG_TILE_BF16 32x32 bf16 matrix-core blocks + band re-decision
                               (NORMAL_PLANE: DLG_TILE_EXACT lanes as planes with the prefilter
                               verdicts as bits, DLG_TILE_BF16 round 4's lanes-as-points scorer).
                               (A/B-only variants of the first, same counts: 11, 14 with 1, 4
                               planes per lane, 12 packed f32 tests, 15..17 item-claim orders;
                               the getter returns the value set) */
  DLG_OPT_NORMALS_FUSED = 10, /* PCL-float radius normals: 1 (default) search, (d2, index) order
                               and sums in one fused pass; 0: the chunked count / fill / sort /
                               sum pipeline */
  DLG_OPT_REGULATE_WAVE = 11, /* RegulateNormal's claim pass: 1 (default) one wave per frontier
                               node over its packed candidate cells; 0: one thread per (node,
                               cell) */
  DLG_OPT_FS_POISON = 12,   /* tests only: 1 fills the PCL float-sum walk's window tables with
                               garbage entries stamped for the next launch whenever its scratch
                               is laid out, before the clear; 0 (default) */
  DLG_OPT_HYP_SHARD = 13,   /* several ranks, small clouds (SURVEY 8(e)'s fallback): 1 = every
                               rank uploads the WHOLE cloud (id_base 0) and dlg_sac_segment /
                               dlg_extract_planes split each batch's hypotheses over the ranks
                               (rank r scores its slice, the counts are allreduced; the rest of
                               the round runs on every rank alike: same results as one rank).
                               0: point sharding (each rank uploads its shard).  -1 (default):
                               hypothesis sharding exactly when every rank holds the same cloud
                               (same ids and extent), decided once per cloud -- the layout
                               dlg_shard_range hands out when point shards would be too small.
                               The decision compares counts, id_base and extents, not the
                               points: ranks that upload different points with equal counts,
                               id_base and extents (index subsets of an axis-aligned scene)
                               must set 0 themselves, and every rank must set the same value */
  DLG_OPT_FS_ONE_WALK = 14, /* several ranks, PCL float refit (same sums every way): 0 (default)
                               = walk, rebase every rank on the guess the walks propagate, walk
                               again, then hand the exact chain ends rank to rank (each repair a
                               few windows long); 1 = no rebase: the repairs start from the
                               double-prefix guesses (the round-4 protocol, A/B only); 2 = 0 with
                               parallel repair iterations and host checks instead of the
                               hand-over (tests and A/B only) */
  DLG_OPT_FS_SEGMENTS = 15, /* one rank, PCL float refit: walkers per float chain, 1..16 (default
                               8): the chain's windows in segments walked at once from the refined
                               guesses, then joined in order (a segment whose guess was not its
                               exact start is walked again until it meets its recorded walk); 1 =
                               one walker per chain.  Same sums every way */
  DLG_OPT_FAULT_INJECT = 16, /* tests only: k > 0 = this rank fails (DLG_ERR_INTERNAL) in the
                               middle of extract round k - 1, after the round's scoring; 0
                               (default).  Exercises the group abort: every peer returns
                               DLG_ERR_COMM naming the failed rank */
  DLG_OPT_SYNC_CHECK = 17,  /* several ranks, debug: 1 = after every extract round the ranks
                               allgather (round, inliers, coefficient bits, collectives issued,
                               the axis bits and eps_angle of dlg_ctx_set_axis) and fail the call
                               (aborting the group) on any mismatch; 0 (default) */
  DLG_OPT_COMM_TIMEOUT_MS = 18, /* several ranks: a host wait on the group (a stream holding an
                               RCCL collective, a round's results) that makes no progress for this
                               long aborts the group (DLG_ERR_COMM on every rank); 0 = no limit;
                               default 600000 */
  DLG_OPT_SEL1_TICKET = 19, /* single-pass select tiles numbered by an atomic ticket taken at
                               dispatch (a tile's predecessors are then always resident, so the
                               look-back completes even beside other contexts' spinning selects on
                               the same device) or by workgroup index (complete in index order
                               while the launch has the device to itself): -1 (default) tickets
                               while another context of this process uses the same device, 1
                               always, 0 never */
  DLG_OPT_BOUNDS_STREAM = 20, /* lean rounds: 1 = the survivors' sphere bounds on a second stream
                               beside the list pass (event-ordered both ways); 0 (default) */
  DLG_OPT_SPATIAL_CURVE = 21, /* the spatial copy's point order (tiles of 32 consecutive points):
                               1 (default) = Hilbert curve, 0 = Morton (Z-order, rounds 1-5).
                               Same results either way; Hilbert tiles are more compact (no Z
                               jumps inside a tile), so fewer (tile, plane) pairs pass the
                               sphere tests.  Applies to clouds built after the change */
  DLG_OPT_FS_JOIN = 22,      /* one rank, PCL float refit, segmented walk: 1 (default) = the last
                               of a chain's segment walkers to finish joins the chain's segments in
                               the walk's own launch; 0 = the joins as a launch of their own
                               (round 5).  Same sums either way */
  DLG_OPT_UNREFINED_LIST = 23, /* lean rounds, PCL float refit: the unrefined plane's inliers in
                               list order by 1 (default) = one pass over the active list (k_ulist:
                               pristine coordinates gathered by index, look-back compaction); 0 =
                               stamps from the Morton copy's near tiles into a bitmap + its
                               compaction (rounds 3-5).  Same inliers either way */
  DLG_OPT_VOXEL_LONG_RUN = 24, /* dlg_voxel_grid: the occupancy from which a voxel's centroid is
                               summed by one wave (64 members loaded at a time, the chains stepped
                               through them) instead of one thread; 1 = every voxel by a wave,
                               INT32_MAX = none.  Default 32 (the measured cross-over).  Same bits for every value */
  DLG_OPT_SOR_LITERAL = 25,    /* tests only, dlg_statistical_outlier_removal: bit 0 = every
                               query's distance sum by the literal sequential loop, bit 1 = the two
                               statistics sums by the literal host loop.  Default 0 (either only
                               where its certificate fails).  Same bits for every value */
  DLG_OPT_ICP_REVERSED = 26,   /* dlg_icp_align / dlg_icp_correspondences: 1 = the correspondence
                               pass visits the working cloud from its last entry to its first.
                               Default 0.  Same bits for every value (the sums are exact) */
  DLG_OPT_ICP_MAX_BLOCKS = 27, /* tests only, dlg_icp_align / dlg_icp_correspondences: n >= 1 = every
                               launch of the registration (gather, apply, level, moments, pack) runs
                               min(its default, n) workgroups, so that a small cloud takes the
                               several-entries-per-thread paths of a huge one; 0..65536.  Default 0
                               (the default launch shapes).  Same bits for every value (the sums
                               are exact) */
  DLG_OPT_CULL = DLG_OPT_ICP_MAX_BLOCKS + 1 /* (28) probability-1 rounds of the plane models on one rank (pruned
                               scoring, DLG_TILE_EXACT): 1 (default) = only the hypotheses whose
                               tile bound -- 32 x the tiles whose sphere test they pass -- can
                               still reach the best exact count are scored exactly, the 64 with the
                               largest bounds first; n in 2..4096 = the n largest first (tests and
                               A/B); 0 = every hypothesis.  A culled hypothesis has a count below
                               the winner's, so computeModel's decision and everything after it are
                               the same for every value; the counts of culled hypotheses are not
                               computed (dlg_score_samples always computes all).  A round that
                               scores more than 1/16 of its batch exactly turns culling off for the rest of
                               the call */
  ,
  DLG_OPT_CULL_FUSE = DLG_OPT_CULL + 1 /* (29) A/B: 1 (default) = a culled round's scoring runs in
                               four launches (prune; tile bound + first candidate set; first exact
                               pass + second set; second exact pass + pick), each selection made by
                               the last workgroup of the launch before it; 0 = the seven-launch
                               sequence (one launch per step).  Same counts, same pick, same
                               dlg_cull_stats for either value */
};
enum { DLG_TILE_EXACT = 0, DLG_TILE_BF16 = 1, DLG_TILE_MFMA = 2 };
enum { DLG_SCORE_EXACT = 0, DLG_SCORE_BF16 = 1, DLG_SCORE_PRUNED = 2,
       /* dlg_score_benchmark only, the culled rounds' launches (DLG_OPT_CULL's K; 0 or 1: 64):
        * DLG_SCORE_BOUND: counts_out[h] = the tile bound of hypothesis h (>= its count);
        * DLG_SCORE_CULLED: counts_out[h] = the exact count of a scored hypothesis, -1 for a culled
        * one (bad draws are never scored) */
       DLG_SCORE_BOUND = 3, DLG_SCORE_CULLED = 4 };
dlg_status dlg_ctx_set_option(dlg_ctx* ctx, int option, int64_t value);
dlg_status dlg_ctx_get_option(const dlg_ctx* ctx, int option, int64_t* value);
/* the pruned scoring kernel's counters since DLG_OPT_PRUNE_STATS was set (or the last reset):
 * [0] workgroups (DLG_TILE_EXACT), [1] super-tile list entries tested against tile spheres, [2] tiles visited,
 * [3] 32x32 blocks (DLG_TILE_EXACT: 64-lane passes) scored, [4] (tile, plane) pairs scored,
 * [5] blocks with a band re-decision (DLG_TILE_BF16 only), [6] / [7] (DLG_TILE_EXACT) the sum
 * and the maximum of the workgroups' spans in 100 MHz clock ticks (load balance).  A culled round
 * (DLG_OPT_CULL) adds its exact passes: [1] planes tested against super-tile spheres, [2] tiles
 * of the super-tiles visited, [4] (tile, plane) pairs evaluated, [3] those in passes of 128 */
dlg_status dlg_prune_stats(dlg_ctx* ctx, uint64_t out[8], int reset);
/* the culled rounds' counters since the context was created (or the last reset), kept on the
 * device and read here: [0] rounds scored culled, [1] hypotheses scored in the first exact pass,
 * [2] in the second, [3] good hypotheses culled, [4] rounds with a non-empty second pass,
 * [5] rounds that scored more than 1/16 of their batch (culling then stops for the call); [6], [7] 0.
 * dlg_score_benchmark's ids do not count */
dlg_status dlg_cull_stats(dlg_ctx* ctx, uint64_t out[8], int reset);

/* Which levels of the grid hierarchy the context's most recent k-NN normals call used
 * (dlg_estimate_normals[_ex] or dlg_cloud_estimate_normals with k_nn > 0).  Host bookkeeping of
 * the call's level loop: no device counters, nothing is read from the device.  A radius call
 * (k_nn == 0) leaves the record alone; a k-NN call clears `valid` when it starts and sets it when
 * its last level is launched, so a call that fails before that leaves valid == 0.  A call refused
 * for its arguments and an empty cloud (n == 0) run no search and leave the record alone. */
typedef struct {
  int32_t valid;           /* 0 until the context has finished a k-NN normals call */
  int32_t k;               /* the call's k_nn */
  int64_t n;               /* points of the call (non-finite rows included) */
  int32_t levels_planned;  /* levels of the hierarchy's plan (1..12); 1: the plain per-thread
                              search, no deferral */
  int32_t reserved;        /* 0 */
  int64_t queries[12];     /* queries launched at level l ([0] == n); 0 beyond levels_planned */
  int32_t built[12];       /* 1: level l's grid was built ([0] always; a coarser level only once
                              some query was deferred to it) */
} dlg_knn_record;          /* dlg_abi_struct_size(26) */
dlg_status dlg_knn_stats(dlg_ctx* ctx, dlg_knn_record* out);

/* The shard of an n_global-point cloud rank `rank` of `world` should upload:
 * the contiguous range [*lo, *hi) of the global order, or -- when a shard would fall below the
 * 131072-point Morton-copy cut-off (the pruned scorer's minimum) and world > 1 -- the whole cloud
 * [0, n_global) on every rank, which DLG_OPT_HYP_SHARD's default (-1) then runs hypothesis-
 * sharded.  *replicated = 1 in that case.  Host arithmetic; no context. */
dlg_status dlg_shard_range(int64_t n_global, int rank, int world, int64_t* lo, int64_t* hi,
                           int* replicated);

/* max over ranks of a host double (bench timing) and a barrier; no-ops for world == 1 */
dlg_status dlg_allreduce_max_f64(dlg_ctx* ctx, double* value);
dlg_status dlg_barrier(dlg_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* DIALOG_RANSAC_H */
