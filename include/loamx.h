/* loamx — C-ABI of the MI355X-native LOAM registration hot path.
 *
 * One opaque handle per reference class on the path; every entry point below is what a binding of that class
 * would call.  The reference interfaces replaced (all under /root/reference):
 *
 *   loamx_scanreg_*  <->  loam::BasicScanRegistration   include/loam_velodyne/BasicScanRegistration.h:135-163
 *                                                        (processScanlines src/lib/BasicScanRegistration.cpp:28-46,
 *                                                         extractFeatures :155-254, RegistrationParams .h:34-72)
 *   loamx_odom_*     <->  loam::BasicLaserOdometry      include/loam_velodyne/BasicLaserOdometry.h:16-48
 *                                                        (process src/lib/BasicLaserOdometry.cpp:196-666,
 *                                                         transformToEnd :57-87, updateIMU :181-194)
 *   loamx_map_*      <->  loam::BasicLaserMapping       include/loam_velodyne/BasicLaserMapping.h:80-111
 *                                                        (process src/lib/BasicLaserMapping.cpp:266-599,
 *                                                         optimizeTransformTobeMapped :626-926,
 *                                                         updateOdometry :607-621)
 *   loamx_tm_*       <->  loam::BasicTransformMaintenance include/loam_velodyne/BasicTransformMaintenance.h:44-66
 *   loamx_batch_*    new: the batched-sweep mode of BASELINE.json's north_star (independent sweeps against a frozen
 *                    shared map) — the unit that is sharded across GPUs.
 *
 * Conventions
 *  - Point clouds are caller-owned arrays of records with x,y,z float32 at byte offsets 0/4/8 and intensity float32
 *    at byte offset `intensity_offset` of each record, `stride` bytes apart.  pcl::PointXYZI is {stride 32,
 *    intensity_offset 16}; a packed float4 is {16, 12}.  Outputs are written with the same description.
 *  - Poses are float[6] = rot_x (pitch), rot_y (yaw), rot_z (roll), x, y, z in the LOAM camera frame, rotation order
 *    R = Ry*Rx*Rz (reference src/lib/math_utils.h:212-238).
 *  - Point coordinates handed to loamx_scanreg_process, loamx_odom_*, loamx_map_* and staged into a pipeline must be finite.  The
 *    reference's own pipeline guarantees that (MultiScanRegistration.cpp:187-191 drops non-finite returns — and so does
 *    loamx_scanreg_process_raw / loamx_pipeline_stage_step_raw); its pcl::removeNaNFromPointCloud calls in the odometry
 *    (BasicLaserOdometry.cpp:230, :252) are safeguards that never fire there.  Here a violation is an ERROR, not a silent drop: the
 *    call (for a pipeline: the step that first uses the sweep) returns LOAMX_E_INVALID — binned rings are checked on the device while
 *    the curvature pass reads them, feature clouds on the host while they are packed; full-resolution clouds that are only
 *    transformed (loamx_map_process full_res) are not checked.
 *  - Return value: 0 = processed, 1 = skipped (mirrors the reference's `false` / silent guards), < 0 = error;
 *    loamx_last_error() gives the text for the calling thread's last failing call.  No exception or abort crosses
 *    the ABI.
 *  - A handle is single-threaded (externally synchronised), owns its device memory and one HIP stream; calls are
 *    synchronous unless named *_async.  No pointer returned by the library outlives the next call on that handle.
 *  - The library needs a gfx950 GPU: creating a handle without one fails with LOAMX_E_NOGPU.  There is no CPU
 *    fallback anywhere in the library.
 */
#ifndef LOAMX_H
#define LOAMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LOAMX_OK 0
#define LOAMX_SKIPPED 1
#define LOAMX_E_INVALID (-1)
#define LOAMX_E_CAPACITY (-2)
#define LOAMX_E_HIP (-3)
#define LOAMX_E_NOGPU (-4)
#define LOAMX_E_UNSUPPORTED (-5) /* an optional dependency was left out of this build (the multi-GPU exchanges without RCCL) */
#define LOAMX_E_INTERNAL (-6)    /* a bound that the library's own invariants exclude was reached (the route's round cap) */

/* caller-owned cloud description (input or output) */
typedef struct loamx_cloud {
  void* data;                /* first record */
  uint32_t count;            /* in: number of points (input) / capacity (output); out: points written */
  uint32_t stride;           /* bytes between records, >= 16 */
  uint32_t intensity_offset; /* byte offset of the float32 intensity inside a record (12 or 16) */
  uint32_t reserved;
} loamx_cloud;

const char* loamx_last_error(void);
/* number of visible HIP devices (0 if none / HIP unavailable); never fails */
int loamx_device_count(void);
/* ABI version of this header */
#define LOAMX_ABI_VERSION 6
int loamx_abi_version(void);
/* How this library was built, as "key=value;..." (static storage): abi=<n>; diag=0|1 (1: made with EXTRA=-DLOAMX_DIAG — the only kind of
 * build that reads the diagnostic LOAMX_* environment switches, some of which change results; a product library ignores them);
 * rccl=0|1; roctx=0|1.  A harness records it next to its measurements. */
const char* loamx_build_info(void);
/* Host memory pinned by the HIP runtime this library runs on (hipHostMalloc / hipHostFree; NULL when there is no device or no
 * memory): sweeps of packed {stride 16, intensity at 12} records handed over from such memory, and landing areas of that kind for
 * registered clouds, are copied by DMA from / to where they lie instead of through the handles' staging blocks.  Memory pinned by other
 * means through the same runtime (hipHostRegister, a framework's pinned allocator) is recognised as well; anything else works as before. */
void* loamx_host_alloc(size_t bytes);
void loamx_host_free(void* p);

/* ------------------------------------------------------------------------------------------------------------
 * Feature extraction  (BasicScanRegistration, IMU-less path)
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct loamx_scanreg loamx_scanreg;

/* mirrors loam::RegistrationParams (BasicScanRegistration.h:34-72, defaults .h:37-44) */
typedef struct loamx_scanreg_config {
  float scan_period;                 /* 0.1 */
  int n_feature_regions;             /* 6 */
  int curvature_region;              /* 5 */
  int max_corner_sharp;              /* 2 */
  int max_surface_flat;              /* 4 */
  float less_flat_filter_size;       /* 0.2 */
  float surface_curvature_threshold; /* 0.1 */
  int device;                        /* HIP device ordinal */
  /* (ABI version 2) */
  int max_corner_less_sharp;         /* 20; must be >= max_corner_sharp (ScanRegistration.cpp:100-109).  0 = 10 x max_corner_sharp,
                                        what the RegistrationParams constructor derives (BasicScanRegistration.cpp:22) */
  int imu_history_size;              /* 200; >= 1 (ScanRegistration.cpp:59-66).  The reference's history buffer is created with 200
                                        entries and ensureCapacity only grows it (CircularBuffer.h:53-70), so values below 200
                                        behave as 200; at most 4096 here */
} loamx_scanreg_config;

/* Ring-length limit.  The feature extraction holds a whole scan ring in one workgroup's LDS, so the longest ring of a sweep (of any
 * sweep of a pipeline step) has a limit that depends on n_feature_regions (R) and the pick limits.  With L the ring length,
 *   F = 16 * ceil(L / 16),   N = 16 * ceil((floor(L / R) + 8) / 16),   S = the smallest power of two >= max(N, 64),
 *   W = min(R, 6),           C = 4 * R * (max_corner_sharp + max_corner_less_sharp + max_surface_flat),
 *   bytes = 16 * ceil((8 * F + C) / 16) + 9 * W * N + (S > 512 ? 8 * W * S : 0) + 16,
 * a ring is accepted when bytes <= 162816 (160 KB less 1 KB).  The longest ring accepted at the default pick limits (2, 20, 4):
 *   R        1     2     3     4     5     6     7     8     12    13    16    32     64
 *   L_max  5704  5681  6122  5667  5084  6101  7118  7616  8939  9168  9776  16159  17568
 * curvature_region does not enter.  A longer ring is refused with LOAMX_E_INVALID before anything is enqueued; the handle stays
 * usable.  With raw input (process_raw, process_sensor, the pipeline's raw steps) the ring sizes are known only after binning,
 * so the refusal comes after the binning and before the extraction. */

void loamx_scanreg_default_config(loamx_scanreg_config* cfg);
loamx_scanreg* loamx_scanreg_create(const loamx_scanreg_config* cfg);
void loamx_scanreg_destroy(loamx_scanreg* h);
/* BasicScanRegistration::configure (BasicScanRegistration.cpp:49-53): new parameters for an existing handle; the IMU history,
 * the scan time and the sweep state are kept, as in the reference (cfg->device must be the handle's device) */
int loamx_scanreg_configure(loamx_scanreg* h, const loamx_scanreg_config* cfg);
/* processScanlines: `cloud` holds the rings concatenated in ring order, ring r occupying ring_size[r] points.
 * Outputs (any may be NULL): sharp, less_sharp, flat, less_flat; count fields return the sizes. */
int loamx_scanreg_process(loamx_scanreg* h, const loamx_cloud* cloud, const uint32_t* ring_size, uint32_t n_rings,
                          loamx_cloud* sharp, loamx_cloud* less_sharp, loamx_cloud* flat, loamx_cloud* less_flat);

/* Raw-sweep ingestion + feature extraction: loam::MultiScanRegistration::process(laserCloudIn, scanTime)
 * (src/lib/MultiScanRegistration.cpp:160-238) followed by processScanlines.  `mapper` mirrors loam::MultiScanMapper
 * (include/loam_velodyne/MultiScanRegistration.h:47-89; presets .h:60-75; validation .cpp:107-127).
 * raw_xyz: `count` records with x, y, z float32 at byte offsets 0/4/8 (sensor axes: x forward, y left, z up — the
 * /velodyne_points payload), `stride` bytes apart, in firing order.
 * Outputs (any may be NULL): `full` = the binned cloud in the LOAM frame, rings concatenated, intensity = ring + relTime
 * (laserCloud()); ring_size[n_scan_rings] = points per ring; then the four feature clouds as in loamx_scanreg_process. */
typedef struct loamx_multiscan_mapper {
  float lower_bound_deg;  /* vertical angle of the first ring */
  float upper_bound_deg;  /* vertical angle of the last ring */
  uint32_t n_scan_rings;
} loamx_multiscan_mapper;
int loamx_multiscan_mapper_preset(const char* sensor /* "VLP-16" | "HDL-32" | "HDL-64E" */, loamx_multiscan_mapper* out);
int loamx_scanreg_process_raw(loamx_scanreg* h, const loamx_multiscan_mapper* mapper, const void* raw_xyz, uint32_t count,
                              uint32_t stride, loamx_cloud* full, uint32_t* ring_size, loamx_cloud* sharp, loamx_cloud* less_sharp,
                              loamx_cloud* flat, loamx_cloud* less_flat);

/* Sensor model: raw-sweep ingestion for any lidar.  It generalises loamx_multiscan_mapper: it says where the ring of a record
 * comes from (linear bounds as the mapper, a table of laser elevations, or a ring field of the record) and where its time within
 * the sweep comes from (the azimuth, as the reference computes it, or a time field of the record).  Records keep x, y, z float32 at
 * byte offsets 0 / 4 / 8; field offsets are byte offsets inside a record of `stride` bytes (a PointCloud2 field list).
 * A record is kept when its x, y, z are finite and not near zero (MultiScanRegistration.cpp:187-196), its ring is valid, and — in
 * time-field mode — its time is finite.  Then:
 *   RING_FROM_BOUNDS   ring = getRingForAngle of the vertical angle, as loamx_scanreg_process_raw computes it, bit for bit.
 *   RING_FROM_TABLE    with angle and deg = (double)(angle * 180) / PI taken as for BOUNDS: ring = the k that minimises
 *                      |deg - ring_angles_deg[k]| in double (a tie goes to the smaller k); dropped when that minimum is above
 *                      max_angle_error_deg.  The table has n_scan_rings finite entries, strictly increasing (ring 0 = lowest).
 *   RING_FROM_FIELD    ring = the unsigned integer at ring_offset (U8 / U16 / U32); dropped when >= n_scan_rings.
 *   TIME_FROM_AZIMUTH  relTime as loamx_scanreg_process_raw computes it, halfPassed included, over the records kept by THIS model
 *                      in record order; startOri / endOri from records 0 and count - 1 (MultiScanRegistration.cpp:165-173).  It
 *                      assumes firing order.
 *   TIME_FROM_FIELD    t_i = the field at time_offset (U32 / F32 / F64) as a double; t_ref = the smallest t_i of the kept records;
 *                      relTime = (float)((t_i - t_ref) * time_scale), clamped to scan_period when above it.  No azimuth is used,
 *                      so any record order works: RING-MAJOR CLOUDS (Ouster) REQUIRE THIS MODE.
 * The kept records are split by ring in record order (stable), intensity = (float)ring + relTime, and IMU de-skew uses that relTime
 * (the IMU index is the running maximum over the kept records in record order), as for loamx_scanreg_process_raw. */
enum { LOAMX_RING_FROM_BOUNDS = 0, LOAMX_RING_FROM_TABLE = 1, LOAMX_RING_FROM_FIELD = 2 };
enum { LOAMX_TIME_FROM_AZIMUTH = 0, LOAMX_TIME_FROM_FIELD = 1 };
enum { LOAMX_FIELD_U8 = 1, LOAMX_FIELD_U16 = 2, LOAMX_FIELD_U32 = 3, LOAMX_FIELD_F32 = 4, LOAMX_FIELD_F64 = 5 };
typedef struct loamx_sensor_model {
  uint32_t n_scan_rings;                  /* 1..256 (BOUNDS: >= 2, as loamx_scanreg_process_raw) */
  uint32_t ring_source, time_source;      /* LOAMX_RING_FROM_*, LOAMX_TIME_FROM_* */
  float lower_bound_deg, upper_bound_deg; /* BOUNDS: exactly loamx_multiscan_mapper (upper > lower) */
  const float* ring_angles_deg;           /* TABLE: n_scan_rings entries, strictly increasing; read during the call only */
  float max_angle_error_deg;              /* TABLE: > 0; a record farther than this from every entry is dropped */
  uint32_t ring_offset, ring_type;        /* FIELD ring: byte offset in the record, LOAMX_FIELD_U8 / U16 / U32 */
  uint32_t time_offset, time_type;        /* FIELD time: byte offset in the record, LOAMX_FIELD_U32 / F32 / F64 */
  double time_scale;                      /* FIELD time: seconds per unit of the field (1 for seconds, 1e-9 for nanoseconds) */
} loamx_sensor_model;
/* BOUNDS + AZIMUTH model of a mapper (zeroes the other fields); host only */
int loamx_sensor_model_from_mapper(const loamx_multiscan_mapper* m, loamx_sensor_model* out);
/* LOAMX_OK, or LOAMX_E_INVALID with a message: unknown source or type; table NULL, not strictly increasing or not finite;
 * max_angle_error_deg <= 0; a field that does not fit inside `stride` or is not naturally aligned; time_scale <= 0 or not finite;
 * a ring count out of range; a stride below 12 or not a multiple of 4.  Host only: needs no device. */
int loamx_sensor_model_check(const loamx_sensor_model* m, uint32_t stride);
/* loamx_scanreg_process_raw with a sensor model: same outputs (ring_size has m->n_scan_rings entries), IMU handling and errors */
int loamx_scanreg_process_sensor(loamx_scanreg* h, const loamx_sensor_model* m, const void* records, uint32_t count, uint32_t stride,
                                 loamx_cloud* full, uint32_t* ring_size, loamx_cloud* sharp, loamx_cloud* less_sharp,
                                 loamx_cloud* flat, loamx_cloud* less_flat);

/* IMU data for the scan registration: updateIMUData (BasicScanRegistration.cpp:82-98) feeds the
 * handle's IMU history (capacity max(200, imu_history_size): the reference's buffer is created with 200 entries and
 * ensureCapacity only grows it, include/loam_velodyne/CircularBuffer.h); loamx_scanreg_set_time gives the scanTime of the
 * next process call (times in seconds on one clock); with a non-empty history loamx_scanreg_process_raw de-skews every
 * kept point (projectPointToStartOfSweep :101-147) and loamx_scanreg_get_imu_trans returns imuTransform() (:258-281):
 * start angles, current angles, position shift, velocity change — what loamx_odom_update_imu consumes.
 * acc_xyz: local acceleration with gravity removed and axes remapped as ScanRegistration.cpp:171-174 does. */
int loamx_scanreg_update_imu(loamx_scanreg* h, double stamp_sec, float roll, float pitch, float yaw, const float acc_xyz[3]);
int loamx_scanreg_set_time(loamx_scanreg* h, double scan_time_sec);
int loamx_scanreg_get_imu_trans(loamx_scanreg* h, float imu_trans[12]);

/* ------------------------------------------------------------------------------------------------------------
 * Sweep-to-sweep odometry  (BasicLaserOdometry)
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct loamx_odom loamx_odom;

typedef struct loamx_odom_config {
  float scan_period;  /* 0.1  */
  int max_iterations; /* 25; 1 .. 255 */
  float delta_t_abort; /* 0.1 */
  float delta_r_abort; /* 0.1 */
  int device;
} loamx_odom_config;

void loamx_odom_default_config(loamx_odom_config* cfg);
loamx_odom* loamx_odom_create(const loamx_odom_config* cfg);
void loamx_odom_destroy(loamx_odom* h);
/* updateIMU: 4 x (x,y,z) = pitch/yaw/roll start, pitch/yaw/roll end, shift from start, velocity from start */
int loamx_odom_update_imu(loamx_odom* h, const float imu_trans[12]);
/* process(): the four feature clouds of the current sweep.  The first call only initialises (reference
 * BasicLaserOdometry.cpp:198-211). */
int loamx_odom_process(loamx_odom* h, const loamx_cloud* sharp, const loamx_cloud* less_sharp, const loamx_cloud* flat,
                       const loamx_cloud* less_flat);
int loamx_odom_get_transform(loamx_odom* h, float transform[6]);
int loamx_odom_get_transform_sum(loamx_odom* h, float transform_sum[6]);
int loamx_odom_set_transform(loamx_odom* h, const float transform[6]);
int loamx_odom_set_transform_sum(loamx_odom* h, const float transform_sum[6]);
/* lastCornerCloud()/lastSurfaceCloud(): the re-projected feature clouds handed on to mapping */
int loamx_odom_get_last_clouds(loamx_odom* h, loamx_cloud* last_corner, loamx_cloud* last_surf);
/* transformToEnd(cloud): in place on a caller cloud, with the current transform */
int loamx_odom_transform_to_end(loamx_odom* h, loamx_cloud* cloud);
/* diagnostics: iterations entered / rows selected in the last iteration of the last process() */
int loamx_odom_get_stats(loamx_odom* h, int stats[4]);

/* ------------------------------------------------------------------------------------------------------------
 * Linked nodes (ABI version 6): the reference's three nodes exchange a sweep's clouds as ROS messages — host memory
 * (ScanRegistration.cpp:186-208 -> LaserOdometry.cpp:141-233 -> LaserMapping.cpp:155-230).  A process that hosts the three
 * handles on ONE device can hand the clouds from node to node in HBM instead: same data flow, same results bit for bit
 * (tests/test_gpu_linked.py), without the five round trips over PCIe per sweep.
 *   loamx_scanreg_process_linked   the sweep goes up and the extraction is enqueued; returns without waiting.  The feature
 *                                  clouds and the sweep stay in the handle's device buffers.  A sweep of packed {stride 16,
 *                                  intensity at 12} records in memory the HIP runtime has pinned (hipHostMalloc / hipHostRegister)
 *                                  is copied by DMA from where it lies and must stay unchanged until loamx_odom_process_linked
 *                                  has returned; any other cloud has been copied out when this call returns.
 *   loamx_odom_process_linked      waits for `sr`'s extraction (and reports what loamx_scanreg_process would: LOAMX_E_INVALID
 *                                  for non-finite input, ...) — in two steps: the iterations start on the sharp / less-sharp / flat
 *                                  clouds, the less-flat cloud (its voxel grid still running) is taken when the sweep's tail
 *                                  needs it — runs process() on its clouds and re-projects the sweep's
 *                                  full-resolution cloud to the sweep end (transformToEnd of LaserOdometry.cpp:326) into a
 *                                  device buffer of `od`.  Returns with the pose (LOAMX_SKIPPED for the initialising sweep); the
 *                                  tail goes on behind it.  `sr`'s buffers are read until loamx_odom_link_wait(od) or
 *                                  loamx_map_process_linked has returned: start `sr`'s next sweep only then.
 *   loamx_map_process_linked       updateOdometry(od's transformSum) + process() on od's last corner / surface clouds and the
 *                                  re-projected full-resolution cloud, ordered behind od's tail on the device.
 *                                  full_res_registered (may be NULL): receives the registered full-resolution cloud
 *                                  (count = capacity in, points out; packed records in pinned memory receive it by DMA directly —
 *                                  loamx_map_process's full_res likewise).  `od` may start its next sweep when this has returned.
 * The host-cloud getters (loamx_odom_get_last_clouds, ...) keep working after the linked calls. */
int loamx_scanreg_process_linked(loamx_scanreg* h, const loamx_cloud* cloud, const uint32_t* ring_size, uint32_t n_rings);
int loamx_odom_process_linked(loamx_odom* h, loamx_scanreg* sr);
int loamx_odom_link_wait(loamx_odom* h);

/* ------------------------------------------------------------------------------------------------------------
 * Scan-to-map registration  (BasicLaserMapping)
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct loamx_map loamx_map;

typedef struct loamx_map_config {
  float scan_period;     /* 0.1  */
  int max_iterations;    /* 10   */
  float delta_t_abort;   /* 0.05 */
  float delta_r_abort;   /* 0.05 */
  float corner_filter_size; /* 0.2 */
  float surf_filter_size;   /* 0.4 */
  float map_filter_size;    /* kept for API parity; unused by the reference as well (BasicLaserMapping.cpp:261) */
  int device;
} loamx_map_config;

void loamx_map_default_config(loamx_map_config* cfg);
loamx_map* loamx_map_create(const loamx_map_config* cfg);
void loamx_map_destroy(loamx_map* h);
int loamx_map_update_odometry(loamx_map* h, const float transform_sum[6]);
/* process(): corner_last / surf_last in, full_res registered in place (transformFullResToMap).
 * Returns with the sweep's results — the transforms, the statistics, the registered cloud.  The map update that ends the reference's
 * process() (insertion into the cubes and their re-filtering, BasicLaserMapping.cpp:535-593) is enqueued behind the registration on
 * the device and may still be running then: every later call that reads or changes the map (the next process / insert, get_cubes,
 * save_snapshot, ...) waits for it first, so the map any call sees is the reference's.  A failure inside the deferred update is
 * reported by that later call.  Every fifth processed frame (the surround cloud is cut from the updated map, :242-264) waits itself. */
int loamx_map_process(loamx_map* h, const loamx_cloud* corner_last, const loamx_cloud* surf_last, loamx_cloud* full_res);
/* see "Linked nodes" above */
int loamx_map_process_linked(loamx_map* h, loamx_odom* od, loamx_cloud* full_res_registered);
/* Behind a sweep's map update the handle prepares the NEXT sweep's map partition and sub-map index for the pose it predicts (constant
 * odometry velocity); the next process() adopts that work when the plan of the true pose — cube window, valid cubes, their order and
 * sizes — equals the predicted one entry by entry, and partitions afresh otherwise: results never depend on it.  counts[0] = sweeps
 * that adopted a prepared partition, counts[1] = sweeps whose prediction missed.  LOAMX_MAP_NO_SPECULATION=1 switches it off. */
int loamx_map_get_speculation(loamx_map* h, uint64_t counts[2]);
/* The map side of process() alone — the merge step of a map epoch (collective 3): a sweep that was registered elsewhere
 * (the batched pipeline, against a frozen copy of this map) is stacked, down-sized, inserted into the cubes with the GIVEN pose
 * (rx, ry, rz, tx, ty, tz = its transformAftMapped) and the touched cubes are re-filtered, exactly as process() does after its
 * optimisation (BasicLaserMapping.cpp:512-593); no optimisation runs, and the pose is inserted AS GIVEN — no IMU blend is applied to it even
 * when the handle holds IMU history (a pipeline pose has had its blend), and the handle's own transforms (Tobe / Bef / AftMapped), frame
 * counter and iteration limit are as before the call, also after an error.  loamx_map_get_cubes() afterwards is the next epoch's map
 * (loamx_pipeline_stage_frozen_* / loamx_dist_broadcast_map). */
int loamx_map_insert(loamx_map* h, const loamx_cloud* corner_last, const loamx_cloud* surf_last, const float pose6[6]);
/* which: 0 transformAftMapped, 1 transformBefMapped, 2 transformTobeMapped, 3 transformSum */
int loamx_map_get_transform(loamx_map* h, int which, float transform[6]);
int loamx_map_set_transform(loamx_map* h, int which, const float transform[6]);
/* updateIMU(IMUState2) (BasicLaserMapping.cpp:602-605, .h:47-75) and the laserOdometryTime argument of process()
 * (:266): with a non-empty IMU history transformUpdate blends 0.2 % of the interpolated IMU roll / pitch into the pose
 * (:173-200).  Times in seconds on a common clock. */
int loamx_map_update_imu(loamx_map* h, double stamp_sec, float roll, float pitch);
int loamx_map_set_time(loamx_map* h, double laser_odometry_time_sec);
int loamx_map_has_fresh_map(loamx_map* h);
/* laserCloudSurroundDS() */
int loamx_map_get_surround(loamx_map* h, loamx_cloud* out);
/* test / warm-start hook: insert map-frame points straight into the rolling cube grid (by coordinate) */
int loamx_map_load_cubes(loamx_map* h, const loamx_cloud* corner, const loamx_cloud* surf);
/* dump the whole map: which 0 = corner cubes, 1 = surf cubes */
int loamx_map_get_cubes(loamx_map* h, int which, loamx_cloud* out);
/* Map snapshot on disk (checkpointing a map, e.g. as the frozen map of the batched mode): the rolling map
 * of both feature types in storage order, the cube window, the frame counters and the five transforms.  A handle restored with
 * load continues bit for bit like the one that saved (same map filter sizes required).  File layout: mapping.hip, SnapshotHeader. */
int loamx_map_save_snapshot(loamx_map* h, const char* path);
int loamx_map_load_snapshot(loamx_map* h, const char* path);
/* diagnostics of the last process(): iterations, rows selected, corner queries, surf queries, corner sub-map size,
 * surf sub-map size, degenerate flag, optimised flag */
/* HIP-event timing of the registration inside the last process() (as loamx_batch_set_timing / loamx_batch_get_timing: ms[0] = the
 * registration's device time, ms[1] = sum of the Gauss-Newton launches, counts[0] = launches, counts[1] = query-iterations) */
int loamx_map_set_timing(loamx_map* h, int on);
int loamx_map_get_timing(loamx_map* h, float ms[4], uint64_t counts[4]);
int loamx_map_get_stats(loamx_map* h, int stats[8]);

/* ------------------------------------------------------------------------------------------------------------
 * Pose fusion after the path  (BasicTransformMaintenance, include/loam_velodyne/BasicTransformMaintenance.h:44-66,
 * src/lib/BasicTransformMaintenance.cpp:46-178) and the orientation convention of the nodes' nav_msgs/Odometry
 * messages (src/lib/LaserOdometry.cpp:300-308, src/lib/LaserMapping.cpp:205-213, src/lib/TransformMaintenance.cpp:
 * 66-115).  Host arithmetic only: these entry points need no device.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct loamx_tm loamx_tm;
loamx_tm* loamx_tm_create(void);
void loamx_tm_destroy(loamx_tm* h);
int loamx_tm_update_odometry(loamx_tm* h, const float transform_sum[6]);                                  /* updateOdometry */
int loamx_tm_update_mapping_transform(loamx_tm* h, const float aft_mapped[6], const float bef_mapped[6]); /* updateMappingTransform */
int loamx_tm_associate_to_map(loamx_tm* h);                                                                /* transformAssociateToMap */
int loamx_tm_get_mapped(loamx_tm* h, float transform_mapped[6]);                                           /* transformMapped() */
/* (rot_x, rot_y, rot_z) -> message orientation (x, y, z, w), and back */
int loamx_wire_pose_to_quat(const float rot_xyz[3], double quat_xyzw[4]);
int loamx_wire_quat_to_pose(const double quat_xyzw[4], float rot_xyz[3]);

/* ------------------------------------------------------------------------------------------------------------
 * Batched-sweep mode: B independent sweeps registered against one frozen sub-map.
 *   set_frozen[_device]  -> upload (or adopt) the sub-map and build its spatial index once per map epoch
 *   upload               -> stage the B sweeps' corner_last / surf_last (+ optional full-resolution) clouds in HBM
 *   run                  -> device only: stack round trip, voxel down-sampling, <= max_iterations Gauss-Newton
 *                           iterations per sweep, registration of the full-resolution clouds
 *   download             -> poses + per-sweep stats (+ optionally the registered clouds)
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct loamx_batch loamx_batch;

loamx_batch* loamx_batch_create(const loamx_map_config* cfg, uint32_t max_sweeps);
void loamx_batch_destroy(loamx_batch* h);
int loamx_batch_set_frozen(loamx_batch* h, const loamx_cloud* corner_map, const loamx_cloud* surf_map);
/* device-resident packed float4 (x,y,z,intensity) arrays, e.g. the buffers an RCCL broadcast just filled */
int loamx_batch_set_frozen_device(loamx_batch* h, const void* d_corner_xyzi, uint32_t n_corner, const void* d_surf_xyzi,
                                  uint32_t n_surf);
/* sweep s uses corner_last[s], surf_last[s], full_res[s] (full_res may be NULL) and guess[s][6] =
 * initial transformTobeMapped */
/* Double-buffered map epochs (BASELINE configs[4]): index the NEXT epoch's sub-map on a stream of its own
 * while sweeps are still registered against the current one, then make it current at a batch boundary.  The device
 * buffers are only read until the staged build has finished (hipDeviceSynchronize / the next swap), the index keeps a
 * cell-sorted copy.  wait_event (may be NULL): a hipEvent_t recorded behind whatever fills the buffers (a copy, an RCCL
 * broadcast) — the build is ordered behind it on the device, the host does not wait.  swap returns LOAMX_SKIPPED when nothing is staged. */
int loamx_batch_stage_frozen_device(loamx_batch* h, const void* d_corner_xyzi, uint32_t n_corner, const void* d_surf_xyzi,
                                    uint32_t n_surf, void* wait_event /* hipEvent_t of the buffers' producer, or NULL */);
int loamx_batch_stage_frozen(loamx_batch* h, const loamx_cloud* corner_map, const loamx_cloud* surf_map);   /* host clouds */
int loamx_batch_swap_frozen(loamx_batch* h);
int loamx_batch_upload(loamx_batch* h, uint32_t n_sweeps, const loamx_cloud* corner_last, const loamx_cloud* surf_last,
                       const loamx_cloud* full_res, const float* guess6);
int loamx_batch_run(loamx_batch* h);
int loamx_batch_run_async(loamx_batch* h);
int loamx_batch_sync(loamx_batch* h);
/* poses6: n_sweeps x 6; stats: n_sweeps x 4 ints (iterations, rows selected, corner queries, surf queries);
 * either may be NULL */
int loamx_batch_download(loamx_batch* h, float* poses6, int* stats4);
int loamx_batch_download_full_res(loamx_batch* h, uint32_t sweep, loamx_cloud* out);
/* kernel-level timing of the last run(): ms[0] = whole run, ms[1] = sum of residual-kernel launches,
 * counts[0] = residual launches, counts[1] = total query-iterations executed, counts[2] = total DS queries */
/* record HIP events around every residual launch of the next run()s (off by default) */
int loamx_batch_set_timing(loamx_batch* h, int on);
int loamx_batch_get_timing(loamx_batch* h, float ms[4], uint64_t counts[4]);
/* raw HIP stream of the handle (hipStream_t) so a harness can bracket it with its own events */
void* loamx_batch_stream(loamx_batch* h);
/* Parity hook for the kNN contract (nanoflann_pcl.h:140-152, nanoflann.hpp:115-139, :372-379): runs the library's own
 * neighbour search (the device routine the Gauss-Newton kernel calls) for n query points given in the MAP frame against
 * the frozen corner (which = 0) or surf (which = 1) sub-map.  idx5[5 q + k] = index, in the cloud handed to set_frozen, of
 * the k-th nearest point of query q, d2_5 = its squared distance in float, (dx*dx + dy*dy) + dz*dz; ascending by
 * (distance, index).  Only neighbours closer than 1.05 m are searched for (the reference rejects a query whose fifth
 * neighbour is 1 m away or more, BasicLaserMapping.cpp:671, :760): missing entries are 0xffffffff / FLT_MAX. */
int loamx_batch_knn_probe(loamx_batch* h, int which, const float* queries_xyz, uint32_t n, uint32_t* idx5, float* d2_5);
/* Parity hook for the 6x6 solve of the update steps (colPivHouseholderQr().solve: BasicLaserMapping.cpp:867, BasicLaserOdometry.cpp:559):
 * n systems ata[36 i .. ) x = atb[6 i .. ) through the wave-cooperative routine the kernels call (x_coop) and through the scalar
 * routine it must equal bit for bit (x_scalar, one thread, the reference's order of operations). */
int loamx_batch_qr6_probe(loamx_batch* h, const float* ata, const float* atb, uint32_t n, float* x_coop, float* x_scalar);
/* Stress probe of the exchange between the workgroups of one odometry stream (tagged 16-byte records written by one agent-scope store,
 * accepted by the reader when both tags match): `pairs` producer / consumer workgroup pairs on different XCDs, `rounds` versions per
 * record.  out4 = {accepted reads, torn reads (tags differ: the reader polls again), INCONSISTENT accepted reads (must be 0: the
 * property the exchange rests on), consumer threads that gave up waiting (must be 0)}. */
int loamx_batch_xrec_stress(loamx_batch* h, uint32_t pairs, uint32_t rounds, uint64_t out4[4]);
/* Parity hook for the voxel-grid stage: the down-sampled stack clouds of one sweep of the last run (laserCloudCornerStackDS /
 * laserCloudSurfStackDS, BasicLaserMapping.cpp:512-527 — the query points of the Gauss-Newton iterations, sensor frame, in
 * pcl::VoxelGrid's output order).  count fields: capacity in, size out; LOAMX_E_CAPACITY when a cloud does not fit. */
int loamx_batch_download_ds(loamx_batch* h, uint32_t sweep, loamx_cloud* corner_ds, loamx_cloud* surf_ds);

/* Parity hook for the segmented voxel grid on its own (pcl::VoxelGrid per segment; test use): n packed x y z intensity points in nseg
 * segments, given EITHER as contiguous ranges seg_off[nseg + 1] (seg_off[0] = 0, seg_off[nseg] = n) OR as one segment id per point
 * seg_ids[n] (the other pointer is NULL); valid (optional): one byte per point, 0 = the point is ignored.  Even segments are filtered
 * with leaf_even, odd ones with leaf_odd.  out_xyzi (room for n points) receives the voxel means of segment 0, 1, ... back to back in
 * PCL's output order, out_off[nseg + 1] the running count: segment s owns out_xyzi[out_off[s] .. out_off[s + 1]).  The stage runs
 * as the library's own callers run it (index computation, then the sort and reduction, the kernel chosen by the same dispatch) on
 * one pipeline and stream per process, whose buffers live on from call to call.  LOAMX_E_HIP when a wait inside the kernels timed out. */
int loamx_voxel_probe(const float* pts_xyzi, uint32_t n, const uint32_t* seg_off, const uint32_t* seg_ids, const uint8_t* valid, uint32_t nseg,
                      float leaf_even, float leaf_odd, float* out_xyzi, uint32_t* out_off);
/* Parity hook for the device-wide exclusive scan of uint32 (test use), on one state buffer per process that is cleared once and
 * never again.  len = max(n, max_n).  in[len] is uploaded whole; out[len + 1] (and out2[len + 1] when given: a second copy of the
 * result) are uploaded too, scanned into and read back whole, so the caller sees exactly which words were written: out[0 .. n) = the
 * exclusive prefix sums of in[0 .. n) mod 2^32, out[n] = *total = their sum.  flags: */
#define LOAMX_SCAN_COUNT_ON_DEVICE 1u /* the kernel reads n from device memory and the launch covers max_n elements; an n beyond max_n
                                       * is cut to the launch and answered with LOAMX_E_HIP (the buffers are still read back).
                                       * Without it n travels as a kernel argument and max_n only sizes the buffers */
#define LOAMX_SCAN_IN_PLACE 2u        /* the input is scanned inside the result buffer */
#define LOAMX_SCAN_ZERO_IN 4u         /* the scan clears the input it has read; in[len] receives the input buffer as the scan left it */
int loamx_scan_probe(uint32_t* in, uint32_t n, uint32_t max_n, uint32_t flags, uint32_t* out, uint32_t* total, uint32_t* out2);
/* Parity hook for the counting-sorted grid index on its own (test use): n packed points (x y z w) in K clouds, cloud c =
 * [off[c], off[c + 1]) with off[0] = 0, off[K] = n, K <= 4096, empty clouds allowed; cell_edge: the initial cell edge, 0.25 .. 16 (it
 * grows by 1.25x while a cloud's cell table exceeds its budget: 16 M - 2048 cells over K).  One single index and one batch index per
 * process live on the probes' stream from call to call, with the state every build leaves behind.  flags: */
#define LOAMX_INDEX_SINGLE 1u      /* the single-cloud index of the registration: K = 1, n >= 1, cell_edge 1.05f, no ring packing */
#define LOAMX_INDEX_PACK_RING 2u   /* .w of a sorted point = (ring << 24) | index, ring = (int) of the input's .w; 255 = does not fit */
#define LOAMX_INDEX_FOLD_BOUNDS 4u /* a kernel copies the points and folds them into the index's bounds accumulators as the library's
                                    * producers do; the build then skips its own bounding-box pass */
typedef struct loamx_index_desc {
  float ox, oy, oz, inv_h; /* origin (the cloud's minimum) and 1 / cell edge */
  int32_t nx, ny, nz;
  uint32_t ncell;          /* nx * ny * nz (an empty cloud: one cell) */
  uint32_t cell_base;      /* the cloud's first entry in the cell table */
  uint32_t pt_base;        /* off[c] */
} loamx_index_desc;
/* desc[K]; table[table_cap] receives *table_len = total cells + 1 entries (LOAMX_E_CAPACITY, with *table_len set, when it does not
 * fit): cell j of cloud c holds sorted points [table[cell_base + j], table[cell_base + j + 1]); sorted_xyzw: room for n points, .w =
 * the point's index inside its cloud (bit pattern), with the ring byte under LOAMX_INDEX_PACK_RING. */
int loamx_index_probe(const float* pts_xyzw, uint32_t n, const uint32_t* off, uint32_t K, float cell_edge, uint32_t flags, loamx_index_desc* desc,
                      uint32_t* table, uint32_t table_cap, uint32_t* table_len, float* sorted_xyzw);
/* Parity hook for the bucketed voxel grid of the registration's stack clouds on its own (test use): n >= 1 packed x y z intensity
 * points (n < 2^24) in nseg <= 4096 contiguous segments seg_off[nseg + 1] (seg_off[0] = 0, seg_off[nseg] = n, empty ones allowed);
 * segment k belongs to sweep k / 2 and is filtered with leaf_even / leaf_odd by its parity.  poses12: 12 words per sweep,
 * (nseg + 1) / 2 sweeps — rx ry rz tx ty tz sin(rx) cos(rx) sin(ry) cos(ry) sin(rz) cos(rz), the sine / cosine words used as given.
 * Non-finite and far coordinates are NOT refused: they are the stage's own give-up case.  The stage runs as the registration runs it
 * (plan, round trip + bucket search, reduction; one object and stream per process, whose buffers, counters and epoch live on from
 * call to call), then the stream is waited for.  There is no fallback: after a give-up the arrays hold what the kernels left.
 * stack_xyzi[n]: every point after the map -> sensor round trip; out_xyzi[n] / out_off[nseg + 1]: the voxel means of segment 0, 1, ...
 * back to back in PCL's output order and the running count; segs[nseg], lo[bucket_cap], cnt[bucket_cap]: the plan — per segment its
 * first bucket, bucket count and position bits, per bucket the smallest voxel key it takes ((iz + 2^20) << 42 | (iy + 2^20) << 21 |
 * (ix + 2^20)) and the number of points that arrived.  A segment of m points owns max(1, ceil(m / 2048)) buckets; LOAMX_E_CAPACITY
 * (status->buckets set, nothing run) when bucket_cap is smaller than their sum.  LOAMX_E_HIP when a wait inside the kernels timed out. */
#define LOAMX_VOXBUCKET_SRC_POINTERS 1u /* the kernels read segment k through a device table of one pointer per segment (the
                                         * registration's device-resident inputs) instead of the concatenated array */
typedef struct loamx_voxbucket_seg {
  uint32_t bucket0, nbuckets, pos_bits, pad; /* nbuckets = 0: the plan gave the segment up */
} loamx_voxbucket_seg;
typedef struct loamx_voxbucket_status {
  uint32_t gave_up; /* 1: the run raised its fail word (the registration would repeat it through the general kernel) */
  uint32_t why;     /* bit r: reason r — 0 coordinate beyond +-2^20 voxels or not finite, 1 more than 512 buckets in a segment,
                     * 2 segment box beyond INT_MAX voxels, 3 bucket box beyond 63 sort bits, 5 bucket over its 4096 slots */
  uint32_t buckets; /* buckets of the run */
  uint32_t pad;
} loamx_voxbucket_status;
int loamx_voxbucket_probe(const float* pts_xyzi, uint32_t n, const uint32_t* seg_off, uint32_t nseg, const float* poses12, float leaf_even,
                          float leaf_odd, uint32_t flags, float* stack_xyzi, float* out_xyzi, uint32_t* out_off,
                          loamx_voxbucket_status* status, loamx_voxbucket_seg* segs, uint64_t* lo, uint32_t* cnt, uint32_t bucket_cap);
/* Parity hook for the sweep re-projection on its own (transformToEnd, BasicLaserOdometry.cpp:57-87, and its de-skew twin
 * transformToStart, :40-53; test use): n packed points (x y z w, w = ring + time fraction, 0 <= w < 1024, finite coordinates) in K
 * clouds, cloud c = [off[c], off[c + 1]) with off[0] = 0, off[K] = n, 1 <= K <= 4096, empty clouds allowed; cloud c belongs to
 * stream c % ns, 1 <= ns <= K.  params[ns]: the re-projection parameters of every stream, word for word what the kernels read — the
 * sine / cosine words are used as given, never recomputed from angles.  The library's own kernels run unmodified, on one object and
 * stream per process whose buffers live on from call to call.  out_xyzw[n] receives the points.  The variant is flags & 7: */
#define LOAMX_REPROJECT_BATCH 0u     /* the batch kernel in place: it also writes the ring-first table and folds the bounds */
#define LOAMX_REPROJECT_FUSED 1u     /* the batch kernel reading points [0, n_corner_all) and [n_corner_all, n) from two source arrays
                                      * (the fused staging copy); the array it writes starts as all-ones words */
#define LOAMX_REPROJECT_SINGLE 2u    /* the single-cloud kernel, in place, one launch per cloud */
#define LOAMX_REPROJECT_COPY 3u      /* the copying single-cloud kernel, one launch per cloud */
#define LOAMX_REPROJECT_GATHER 4u    /* the gather kernel: every cloud in a buffer of its own, handed over last cloud first, with an
                                      * explicit stream id per cloud */
#define LOAMX_REPROJECT_TO_START 5u  /* transformToStart of every point with T and scan_period of its stream; w is handed through */
#define LOAMX_REPROJECT_NO_RING_TABLE 8u /* the batch kernel gets no ring-first table */
#define LOAMX_REPROJECT_NO_BOUNDS 16u    /* the batch kernel gets no bounds accumulators */
/* Variants 2 - 4 have no pass-through of their own: clouds of a stream with enabled == 0 are copied as they are.
 * ring_first[K * 320] and bounds[6 * K] (variants 0 and 1, unless switched off; NULL otherwise allowed) are uploaded, worked on and
 * read back, so the caller sees which words were written.  ring_first: per cloud, word r < 319 = (epoch << 24) | index inside the
 * cloud of the first point of a run of ring r; word 319 = epoch when the cloud is NOT ring-ordered with every ring below 255.
 * epoch: 1 .. 255.  bounds: per cloud min x y z, max x y z of the points written, as order-preserving words (a float's bits with the
 * sign bit set when positive, all bits flipped when negative). */
typedef struct loamx_reproject_params {
  float T[6];                   /* the sweep's transform: rx ry rz tx ty tz */
  float sT[3], cT[3];           /* sine / cosine of rx ry rz */
  float shift[3];               /* imuShiftFromStart */
  float s_start[3], c_start[3]; /* IMU pitch, yaw, roll at the sweep's start */
  float s_end[3], c_end[3];     /* ... and at its end */
  float scan_period;
  int32_t enabled;              /* 0: the batch kernel leaves the stream's clouds as they are (a first sweep) */
} loamx_reproject_params;
int loamx_reproject_probe(const float* pts_xyzw, uint32_t n, const uint32_t* off, uint32_t K, const loamx_reproject_params* params, uint32_t ns,
                          uint32_t epoch, uint32_t n_corner_all, uint32_t flags, float* out_xyzw, uint32_t* ring_first, uint32_t* bounds);

/* ------------------------------------------------------------------------------------------------------------
 * Streaming pipeline: n independent streams, each advancing one sweep per step through feature extraction ->
 * odometry -> registration against the frozen sub-map.  A stream keeps the reference's sequential state (odometry
 * transform / transformSum / last clouds, mapping transformBefMapped / transformAftMapped); only the map is frozen.
 * Sweeps are staged in HBM ahead of time, so step() is device work plus a few offset / pose read-backs.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct loamx_pipeline loamx_pipeline;

loamx_pipeline* loamx_pipeline_create(const loamx_scanreg_config* fcfg, const loamx_odom_config* ocfg,
                                      const loamx_map_config* mcfg, uint32_t n_streams);
void loamx_pipeline_destroy(loamx_pipeline* h);
int loamx_pipeline_set_frozen(loamx_pipeline* h, const loamx_cloud* corner_map, const loamx_cloud* surf_map);
int loamx_pipeline_set_frozen_device(loamx_pipeline* h, const void* d_corner_xyzi, uint32_t n_corner, const void* d_surf_xyzi,
                                     uint32_t n_surf);
/* double-buffered map epochs, as loamx_batch_stage_frozen_device / loamx_batch_swap_frozen; swap between two steps */
int loamx_pipeline_stage_frozen_device(loamx_pipeline* h, const void* d_corner_xyzi, uint32_t n_corner, const void* d_surf_xyzi,
                                       uint32_t n_surf, void* wait_event);
int loamx_pipeline_stage_frozen(loamx_pipeline* h, const loamx_cloud* corner_map, const loamx_cloud* surf_map);
int loamx_pipeline_swap_frozen(loamx_pipeline* h);
/* seed a stream's state; any pointer may be NULL (left unchanged) */
int loamx_pipeline_set_state(loamx_pipeline* h, uint32_t stream, const float* transform, const float* transform_sum,
                             const float* bef_mapped, const float* aft_mapped);
/* stage n_steps sweeps per stream: sweep (t, s) = clouds[t * n_streams + s] (rings concatenated) */
int loamx_pipeline_upload(loamx_pipeline* h, uint32_t n_steps, const loamx_cloud* clouds, const uint32_t* const* ring_size,
                          const uint32_t* n_rings);
/* Streaming input (the PCIe-inclusive mode, SURVEY.md §8d "GPU timing"): instead of staging a whole run with
 * loamx_pipeline_upload, hand over ONE step at a time, in order, without blocking — the copies go to a stream of their own
 * (packed float4 clouds {stride 16, intensity at 12} straight from the caller's memory: pin it, e.g. hipHostRegister, and the
 * transfer is a DMA that overlaps the kernels of the steps in flight; other layouts are repacked through pinned staging on
 * the calling thread).  Up to eight steps are in flight: stage_step(t) may be called once step(t - 8) has returned; the
 * buffers of step t are read until step(t) has returned. */
int loamx_pipeline_stage_step(loamx_pipeline* h, uint32_t step, const loamx_cloud* clouds, const uint32_t* const* ring_size,
                              const uint32_t* n_rings);
/* Raw input for the batched pipeline: step `step` as the sensors delivered it — raw_xyz[s] = one
 * revolution of stream s, counts[s] records with x, y, z float32 at byte offsets 0 / 4 / 8, `stride` bytes apart, sensor axes,
 * firing order (the /velodyne_points payload; MultiScanRegistration.cpp:160-238).  The payloads cross PCIe as they are (pin them
 * for a DMA) and are re-strided, binned into rings and — for a stream with IMU data — de-skewed on the device; same ordering
 * rules as loamx_pipeline_stage_step.  scan_time_sec[s] (may be NULL without IMU data) is the sweep's time stamp on the clock of
 * loamx_pipeline_update_imu, which feeds stream s's IMU history exactly as loamx_scanreg_update_imu does (updateIMUData,
 * BasicScanRegistration.cpp:82-98); the resulting imuTransform() of every sweep is plugged into that stream's odometry
 * (BasicLaserOdometry::updateIMU).  The same messages feed the stream's mapping-side history (LaserMapping's own subscription, 200
 * deep): a sweep staged with a time stamp gets transformUpdate's roll / pitch blend (BasicLaserMapping.cpp:171-200) from the messages
 * that had arrived when it was staged, before its full-resolution cloud is registered. */
int loamx_pipeline_stage_step_raw(loamx_pipeline* h, uint32_t step, const void* const* raw_xyz, const uint32_t* counts, uint32_t stride,
                                  const loamx_multiscan_mapper* mapper, const double* scan_time_sec);
/* loamx_pipeline_stage_step_raw with a sensor model (loamx_sensor_model above): records[s] = counts[s] records of `stride` bytes */
int loamx_pipeline_stage_step_sensor(loamx_pipeline* h, uint32_t step, const void* const* records, const uint32_t* counts,
                                     uint32_t stride, const loamx_sensor_model* m, const double* scan_time_sec);
int loamx_pipeline_update_imu(loamx_pipeline* h, uint32_t stream, double stamp_sec, float roll, float pitch, float yaw, const float acc_xyz[3]);
/* Asynchronous output: after enable (before the first step), download_step_async — called after loamx_pipeline_step(t) —
 * starts copying the registered full-resolution clouds of step t (out[k] = k-th stream that was registered; packed float4
 * records; count in = capacity, out = points) on a copy stream and returns; the registration alternates between two device
 * buffers so the next step does not wait for the copy.  wait_downloads blocks until every started copy has landed.
 * When the destination is pinned memory of the ROCm runtime's own (hipHostMalloc, torch's pinned tensors) the copy is handed to
 * the GPU's SDMA engine directly; other host memory goes through hipMemcpyAsync on a copy stream (whose choice of engine may
 * disturb kernels that write to host memory, see csrc/hostlink.hpp).  download_counts: [0] downloads issued the first way,
 * [1] the second. */
int loamx_pipeline_enable_async_downloads(loamx_pipeline* h);
int loamx_pipeline_download_step_async(loamx_pipeline* h, loamx_cloud* out, uint32_t n_out);
int loamx_pipeline_wait_downloads(loamx_pipeline* h);
int loamx_pipeline_download_counts(loamx_pipeline* h, uint64_t counts[2]);
/* run staged step t for every stream.  LOAMX_SKIPPED when no stream reached the registration stage (first sweeps) */
int loamx_pipeline_step(loamx_pipeline* h, uint32_t step);
/* stats8: odometry iterations, odometry rows, mapping iterations, mapping rows, corner queries, surf queries,
 * degenerate, mapped */
int loamx_pipeline_get(loamx_pipeline* h, uint32_t stream, float* transform, float* transform_sum, float* aft_mapped,
                       int* stats8);
/* registered full-resolution cloud of the k-th stream that was registered in the last step */
int loamx_pipeline_download_full_res(loamx_pipeline* h, uint32_t slot, loamx_cloud* out);
/* The re-projected less-sharp / less-flat clouds of one stream's sweep of the LAST step (laserCloudCornerLast / laserCloudSurfLast as the
 * odometry hands them to the mapping, LaserOdometry.cpp:296-326): with the stream's transformAftMapped (loamx_pipeline_get) they are what
 * loamx_map_insert needs to merge the sweep into the next epoch's map.  count fields: capacity in, size out. */
int loamx_pipeline_download_last_clouds(loamx_pipeline* h, uint32_t stream, loamx_cloud* last_corner, loamx_cloud* last_surf);
/* Look-ahead (default on): while step t's registration runs, the odometry and the feature extraction of the following staged
 * steps already execute on their own HIP streams (they are independent ROS nodes in the reference) — up to
 * loamx_pipeline_lookahead_depth() steps ahead.  Results are identical; loamx_pipeline_get() always reports the sweep that was
 * registered last.  Turn it off when per-stream state is changed with loamx_pipeline_set_state() between steps. */
int loamx_pipeline_set_lookahead(loamx_pipeline* h, int on);
/* How many steps beyond the one being registered the odometry may run: 0 with the look-ahead off, 6 for batches staged with
 * loamx_pipeline_upload (a stream whose sweeps need every odometry iteration needs them for several sweeps in a row; the lead absorbs
 * such a run) and for the streaming ring (loamx_pipeline_stage_step*: eight slots, i.e. six steps beyond the one being registered
 * and one more being staged). */
int loamx_pipeline_lookahead_depth(loamx_pipeline* h);
/* Blocks until the look-ahead has finished every step it is currently allowed to run ahead (odometry of up to
 * loamx_pipeline_lookahead_depth() steps beyond the last loamx_pipeline_step, their feature extraction) and everything of it is enqueued on the device; *last_odometry_step (may be NULL)
 * receives the last step whose odometry is complete.  For a caller that wants a quiescent pipeline — a benchmark window that must
 * contain the look-ahead work it profits from, a clean shutdown point — without switching the look-ahead off. */
int loamx_pipeline_drain_lookahead(loamx_pipeline* h, int* last_odometry_step);
/* HIP-event timing of the stages: 0 off, 1 stage events + an event pair around every Gauss-Newton launch, 2 stage events only
 * (the pairs cost ~3 % of a step: a caller that wants both the rate and the launch durations samples them, as bench.py does). */
int loamx_pipeline_set_timing(loamx_pipeline* h, int on);
/* stage_ms: features, odometry, registration, whole step (HIP events on the pipeline's stream);
 * reg_ms / counts as loamx_batch_get_timing */
int loamx_pipeline_get_timing(loamx_pipeline* h, float stage_ms[4], float reg_ms[4], uint64_t counts[4]);
/* The odometry chains' launch pairs (k_odom_corr_grid + k_odom_lm, BasicLaserOdometry.cpp:246-622 in groups of five iterations), timed
 * with HIP events on the chains' own streams while loamx_pipeline_set_timing(h, 1) is on; running totals over all chains since the handle
 * was created (never waits: a call whose events have not completed is counted later).
 * ms4 = {k_odom_lm launches that iterated, k_odom_lm launches over converged streams, k_odom_corr_grid likewise x 2};
 * counts7 = {lm launches that iterated, lm no-op launches, iterations (slowest stream of each launch, summed), corr launches that
 * searched, corr no-op launches, algorithmic bytes of the iterating lm launches (48 B x features of the streams still iterating),
 * features searched by the corr launches}. */
int loamx_pipeline_get_odom_launch_timing(loamx_pipeline* h, double ms4[4], uint64_t counts7[7]);
void* loamx_pipeline_stream(loamx_pipeline* h);

/* ------------------------------------------------------------------------------------------------------------
 * Multi-GPU: one process per GPU, RCCL over xGMI.  The batched mode shards by independent sweeps — rank r of G
 * registers sweeps [r*B/G, (r+1)*B/G) against a replica of the frozen map — so the data path has no collective.  The two
 * exchanges are (1) the map epoch: ncclBroadcast of the two sub-map buffers, asynchronous, returning an event that
 * loamx_{batch,pipeline}_stage_frozen_device takes as wait_event (the index build of epoch k+1 is ordered behind the broadcast
 * on the device while epoch k's registrations run: double buffering), and (2) the results: ncclAllGather of
 * n_local x (6 pose floats + iterations + flags) per rank.  The 128-byte id from loamx_dist_get_unique_id (rank 0) reaches the
 * other processes by the host's own means (loam_velodyne_amd/launch.py uses a file).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct loamx_dist loamx_dist;
#define LOAMX_DIST_ID_BYTES 128
int loamx_dist_get_unique_id(unsigned char id[LOAMX_DIST_ID_BYTES]);
loamx_dist* loamx_dist_create(const unsigned char id[LOAMX_DIST_ID_BYTES], int rank, int world_size, int device);
void loamx_dist_destroy(loamx_dist* h);
int loamx_dist_rank(const loamx_dist* h);
int loamx_dist_world_size(const loamx_dist* h);
/* this rank's contiguous share [begin, end) of a batch of `batch` sweeps */
int loamx_dist_shard(const loamx_dist* h, uint32_t batch, uint32_t* begin, uint32_t* end);
/* device buffers of packed float4 (x,y,z,intensity), the same sizes on every rank; in place (root's content reaches all).
 * wait_event (may be NULL): hipEvent_t behind whatever fills the root's buffers; *done_event (may be NULL) receives a hipEvent_t
 * owned by the handle, recorded behind the broadcast — valid until the next broadcast on this handle. */
int loamx_dist_broadcast_map(loamx_dist* h, void* d_corner_xyzi, uint32_t n_corner, void* d_surf_xyzi, uint32_t n_surf, int root,
                             void* wait_event, void** done_event);
/* every rank contributes ITS n_local records (poses6[n_local][6], iters_flags2[n_local][2], the latter may be NULL; n_local may
 * differ between ranks and may be 0 — the shards of loamx_dist_shard are unequal whenever the batch does not divide by the world
 * size) and receives the records of all ranks concatenated in rank order (sum of the counts = the batch); counts_all (may be NULL)
 * receives the world_size record counts.  Every rank must call it; blocking. */
int loamx_dist_allgather_results(loamx_dist* h, const float* poses6, const int* iters_flags2, uint32_t n_local, float* poses6_all,
                                 int* iters_flags2_all, uint32_t* counts_all);
/* the same with the capacity of the receive arrays stated (in records): LOAMX_E_CAPACITY — after both collectives, so that no rank
 * is left waiting, and with counts_all filled — when the ranks' records do not fit; nothing is written beyond the capacity */
int loamx_dist_allgather_results_cap(loamx_dist* h, const float* poses6, const int* iters_flags2, uint32_t n_local, float* poses6_all,
                                     int* iters_flags2_all, uint32_t capacity_records, uint32_t* counts_all);
/* only the first half: every rank's record count (for a caller that sizes its receive arrays by them).  Every rank must call it. */
int loamx_dist_allgather_counts(loamx_dist* h, uint32_t n_local, uint32_t* counts_all);
/* ranks the RCCL communicator itself reports (ncclCommCount); -1 on error */
int loamx_dist_comm_count(loamx_dist* h);
/* The host side of the two rules above without a device or a communicator (for a host that brings its own transport; the
 * library's own all-gather uses exactly these): the shard of a rank; the padded send block of a rank (n_pad records of
 * LOAMX_DIST_RECORD_FLOATS floats = 6 pose floats + iterations + flags as raw ints, zero beyond n_local); and the inverse for the
 * gathered blocks recv8[world_size][n_pad][...] given every rank's record count. */
#define LOAMX_DIST_RECORD_FLOATS 8
int loamx_dist_shard_of(int rank, int world_size, uint32_t batch, uint32_t* begin, uint32_t* end);
int loamx_dist_pack_results(const float* poses6, const int* iters_flags2, uint32_t n_local, uint32_t n_pad, float* send8);
int loamx_dist_unpack_results(const float* recv8, const uint32_t* counts, int world_size, uint32_t n_pad, float* poses6_all,
                              int* iters_flags2_all);
/* The merge step of a map epoch (BasicLaserMapping.cpp:536-593 is what loamx_map_insert restates): the sweeps a rank has registered —
 * per stream the re-projected corner / surf clouds of its last step (loamx_pipeline_download_last_clouds) and its transformAftMapped —
 * travel to the rank that owns the map accumulator as ONE message of 32-bit words per rank:
 *   'LXCL', n_streams, (n_corner, n_surf) x n_streams | 6 pose floats x n_streams | the points (x y z intensity), corner(0) surf(0) ...
 * pack / unpack are host-side layout rules (no device, any transport); words == NULL asks for the size only.
 * loamx_dist_gatherv: variable-size gather to `root` over RCCL — every rank's word count first (all-gather), then the words point to
 * point inside one group; recv_words (root only) receives the ranks' messages back to back in rank order, counts_all (may be NULL)
 * every rank's word count.  Every rank calls it, also with n_words = 0. */
int loamx_dist_pack_clouds(uint32_t n_streams, const loamx_cloud* corner, const loamx_cloud* surf, const float* poses6, uint32_t* words,
                           uint64_t capacity_words, uint64_t* n_words);
int loamx_dist_unpack_clouds_header(const uint32_t* words, uint64_t n_words, uint32_t* n_streams, uint32_t* n_corner, uint32_t* n_surf,
                                    uint32_t capacity_streams);
int loamx_dist_unpack_clouds_stream(const uint32_t* words, uint64_t n_words, uint32_t stream, float pose6[6], loamx_cloud* corner,
                                    loamx_cloud* surf);
int loamx_dist_gatherv(loamx_dist* h, const uint32_t* send_words, uint32_t n_words, int root, uint32_t* recv_words, uint64_t capacity_words,
                       uint32_t* counts_all);
int loamx_dist_barrier(loamx_dist* h);
void* loamx_dist_stream(loamx_dist* h);   /* hipStream_t of the collectives */

/* ------------------------------------------------------------------------------------------------------------
 * Dense global map (not in the reference): a sparse voxel map of the whole run in device memory, fed with registered sweeps where
 * they lie (the mapper's and the pipeline's registered full-resolution clouds) or with map-frame points from the host.
 *
 * Per point, in f32 (inv = 1.0f / leaf): d = p - origin, d2 = (dx*dx + dy*dy) + dz*dz; the point is kept when d2 >= min_range^2 and,
 * with max_range > 0, d2 <= max_range^2.  Per axis t = p*inv, i = floor(t), f = t - (float)i, q = min((uint32)(f * 2^20), 2^20 - 1);
 * a point with any |i| >= 2^20 is dropped.  The voxel key packs (iz + 2^20, iy + 2^20, ix + 2^20) in 21 bits each (ascending key =
 * ascending (iz, iy, ix), the order of csrc/voxel.hpp).  Each voxel keeps n and the 64-bit integer sums Sx, Sy, Sz of q: the map, and
 * every byte exported from it, does not depend on the thread schedule or on the order of the points.
 * Export: one record per voxel in ascending key order, x = (float)(((double)ix + (double)Sx / ((double)n * 2^20)) * (double)leaf)
 * (y, z alike), intensity = (float)n; axes 1 writes the sensor axes ingestion started from (x_s = z, y_s = x, z_s = y), axes 0 the LOAM
 * frame.
 * Capacity: with max_voxels > 0 an add is refused (LOAMX_E_CAPACITY, map unchanged) when voxels_now + points_in_call > max_voxels
 * (the cloud's point count before filtering).  Without a cap the table doubles on its own, on the device, before its load would pass
 * one half; the adds from a mapper / a pipeline do not block the calling thread.
 * Ordering: an add from a mapper or a pipeline is enqueued on that handle's own stream, behind the kernel that wrote the registered
 * cloud; download, get_stats and save_pcd wait for every add first.  A source on another device than the map: LOAMX_E_INVALID.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct loamx_densemap loamx_densemap;
typedef struct loamx_densemap_config {
  float leaf;             /* voxel edge in metres, > 0 (default 0.1) */
  float min_range;        /* points closer than this to the sweep's origin are dropped (default 0: none) */
  float max_range;        /* points farther than this are dropped (default 0: no limit) */
  uint64_t max_voxels;    /* cap on stored voxels; 0 = bounded by device memory only */
  uint32_t initial_slots; /* hash-table slots at creation, power of two >= 1024 (default 1 << 20) */
  int device;
} loamx_densemap_config;

void loamx_densemap_default_config(loamx_densemap_config* cfg);      /* host only, no device needed */
loamx_densemap* loamx_densemap_create(const loamx_densemap_config* cfg);
void loamx_densemap_destroy(loamx_densemap* h);
int loamx_densemap_reset(loamx_densemap* h);
/* map-frame points from the host; origin[3] = the sensor position used by the range filter */
int loamx_densemap_add(loamx_densemap* h, const loamx_cloud* points, const float origin[3]);
/* the registered full-resolution cloud of m's last process() / process_linked(), origin = that sweep's transformAftMapped translation;
 * LOAMX_SKIPPED when that call produced no registered cloud */
int loamx_densemap_add_from_map(loamx_densemap* h, loamx_map* m);
/* the registered cloud of the slot-th stream registered in p's last step (the slot of loamx_pipeline_download_full_res), origin = that
 * stream's transformAftMapped translation; LOAMX_SKIPPED when the last step registered nothing */
int loamx_densemap_add_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot);
/* stats: voxels, slots, points offered, points added, dropped by range, dropped outside the key range */
int loamx_densemap_get_stats(loamx_densemap* h, uint64_t stats[6]);
/* count in = capacity, out = voxels (LOAMX_E_CAPACITY, nothing written, when they do not fit); records as described above */
int loamx_densemap_download(loamx_densemap* h, loamx_cloud* out, int axes /* 0 LOAM frame, 1 sensor axes */);
int loamx_densemap_save_pcd(loamx_densemap* h, const char* path, int axes);
/* host only: any cloud as a binary PCD v0.7 file, fields x y z intensity (F 4); axes as above */
int loamx_write_pcd(const char* path, const loamx_cloud* c, int axes);

/* Free-space carving (optional, off by default: a handle that never enables it behaves, allocates and exports as described above).
 * A sweep ray that reaches a far surface proves the voxels it crossed empty; counting those crossings per voxel is what lets an
 * export drop the returns of cars and pedestrians, which otherwise stay in the map as smears along their paths.
 *
 * loamx_densemap_enable_carving is allowed only on an empty map (a fresh handle, or right after reset; otherwise LOAMX_E_INVALID
 * and the handle is unchanged).  It allocates two uint32_t words per slot beside the table: miss, the number of rays that crossed
 * the voxel, and stamp, the sequence number of the last add call that put a point into it.  Carving stays on until the handle is
 * destroyed; reset clears both words of every slot.
 * Per add call (add, add_from_map, add_from_pipeline alike, on the same stream as the insert): the call takes the next sequence
 * number seq (1, 2, ...), inserts as above while storing stamp = seq into every voxel it adds a point to, and then traces rays.
 * The ray of point i of the call (i its index in the call's cloud) is traced iff all of these hold, tested in this order, each failed
 * test counting in a statistic of its own:  the point was added (range and key filters above; no statistic);  i % ray_stride == 0;
 * max_range == 0 or d2 <= max_range^2 (d2 as above, the square in f32);  the origin's cell passes |i| < 2^20 on every axis and
 * n_steps <= max_steps (one statistic for the two).
 * The traversal, in voxel units, f32, no fused multiply-add, / correctly rounded.  Per axis a:  so = o_a*inv, sp = p_a*inv;
 * c0 = (int)floorf(so), c1 = (int)floorf(sp);  rem_a = |c1 - c0|, s_a = sign(c1 - c0);  d = sp - so;  and, where rem_a > 0,
 * b = (float)(c0 + (s_a > 0 ? 1 : 0)), tmax_a = (b - so)/d, tdelta_a = 1.0f/fabsf(d).  n_steps = rem_x + rem_y + rem_z.
 * One step: among the axes with rem_a > 0 the one with the smallest tmax_a (ties: x before y before z) moves its cell index by s_a,
 * rem_a -= 1, tmax_a = tmax_a + tdelta_a.  After exactly n_steps steps the walk stands in the point's cell whatever the rounding
 * did: the step count ends the walk, not a float comparison.
 * Cell k is the cell after k steps (cell 0 the origin's).  The cells k = 0 .. n_steps - 1 - end_margin are visited (none when that
 * is negative; the end cell never is).  A visited cell is looked up in the table, read-only; if it is there and its stamp != seq, its
 * miss goes up by one.  A voxel hit by the same call is not carved by that call ("occupied wins": this keeps ground seen at a
 * grazing angle); cells that are not in the table are free space already.
 * Determinism: n, Sx, Sy, Sz keep their property (they depend on neither order nor call boundaries).  miss depends on neither the
 * thread schedule nor the order of the points within a call (the stride picks by index: with ray_stride > 1 the order decides
 * WHICH rays are traced).  miss does depend on how the points are split into calls and on the order of the calls, by definition: a
 * call carves what the earlier calls left, plus its own inserts through the stamp.
 * Rule: a voxel is dynamic iff miss >= min_misses and (uint64)miss * den > n * num (n the voxel's 64-bit point count); den == 0 is
 * LOAMX_E_INVALID, a NULL rule is the default rule.  download_static / save_pcd_static export as download / save_pcd minus the
 * dynamic voxels.  prune removes them from the table on the device (survivors keep n, S*, miss and stamp; adds go on as before).
 * With carving off every function below except enable_carving and the three host-only helpers answers LOAMX_E_INVALID. */
typedef struct loamx_densemap_carve_config {
  float max_range;      /* rays longer than this are not traced; 0 = no limit (default 0) */
  uint32_t ray_stride;  /* trace the points whose index in the call's cloud is a multiple of it, >= 1 (default 1): the cost knob */
  uint32_t end_margin;  /* cells before the end cell that are left alone (default 1) */
  uint32_t max_steps;   /* rays with more steps are not traced, 1..65536 (default 4096) */
} loamx_densemap_carve_config;
typedef struct loamx_densemap_static_rule {
  uint32_t min_misses;  /* default 3 */
  uint32_t num, den;    /* default 1, 1: more crossings than points */
} loamx_densemap_static_rule;
void loamx_densemap_carve_default_config(loamx_densemap_carve_config* cfg);   /* host only */
void loamx_densemap_static_rule_default(loamx_densemap_static_rule* rule);    /* host only */
/* host only: the rule on one voxel's n and miss, 1 dynamic / 0 static (LOAMX_E_INVALID: NULL or den == 0) */
int loamx_densemap_rule_is_dynamic(const loamx_densemap_static_rule* rule, uint64_t n, uint32_t miss);
int loamx_densemap_enable_carving(loamx_densemap* h, const loamx_densemap_carve_config* cfg /* NULL: the defaults */);
/* waits for the adds as get_stats does.  stats: rays traced, not traced by stride, by range, by step count or origin key; cells
 * visited; misses recorded */
int loamx_densemap_get_carve_stats(loamx_densemap* h, uint64_t stats[6]);
/* the miss word per voxel in the record order of loamx_densemap_download; *n = voxels (LOAMX_E_CAPACITY, nothing written, when
 * capacity < *n) */
int loamx_densemap_download_misses(loamx_densemap* h, uint32_t* out, uint64_t capacity, uint64_t* n);
int loamx_densemap_download_static(loamx_densemap* h, loamx_cloud* out, int axes, const loamx_densemap_static_rule* rule);
int loamx_densemap_save_pcd_static(loamx_densemap* h, const char* path, int axes, const loamx_densemap_static_rule* rule);
/* removed (may be NULL): the number of voxels that left */
int loamx_densemap_prune(loamx_densemap* h, const loamx_densemap_static_rule* rule, uint64_t* removed);

/* Second moments and surfels (optional, off by default: a handle that never enables it behaves, allocates and exports as described
 * above).  With the sums of the products of the offsets beside the sums of the offsets, a voxel holds a mean, a covariance and a
 * normal: the map becomes a surfel / normal-distribution map, from the points it held on the device when they were inserted.
 *
 * loamx_densemap_enable_moments is allowed only on an empty map (a fresh handle, or right after reset; otherwise LOAMX_E_INVALID
 * and the handle is unchanged).  It allocates nine uint64_t words per slot beside the table (72 bytes per slot) and stays on until
 * the handle is destroyed; reset clears the words.  It is independent of carving: either, both or neither, enabled in either order.
 * Per point that an add inserts (add, add_from_map, add_from_pipeline alike; the same filters and the same q_x, q_y, q_z as above),
 * nine integers are added to the words of its voxel, in this order:
 *   Mxx += q_x*q_x, Myy, Mzz, Mxy += q_x*q_y, Mxz, Myz:  each product is an exact integer below 2^40; the sums are unsigned, modulo
 *     2^64, and exact while the voxel holds fewer than 2^24 points.
 *   Vx, Vy, Vz:  with d = p - origin per component in f32 (the d of the range filter),
 *     w_a = (int32_t)fminf(fmaxf(d_a * 1024.0f, -2^30), 2^30) (the conversion truncates toward zero), V_a += w_a as a signed 64-bit
 *     sum (two's complement in the word).  V points from the sensor positions to the voxel's points.
 * All nine are integer sums: like n, Sx, Sy, Sz they depend neither on the thread schedule, nor on the order of the points, nor on
 * how the points are split into calls.  prune and the table's growth carry them.
 * The surfel of a voxel is computed on the host, in double, when it is exported:
 *   N_ab = n*M_ab - S_a*S_b as an exact (128-bit) integer, converted to double once;  C_ab = N_ab / ((double)n * (double)n), the
 *   covariance of the offsets in units of (leaf / 2^20)^2;  l0 <= l1 <= l2 the eigenvalues of the symmetric 3x3 C (cyclic Jacobi).
 *   normal = the unit eigenvector of l0, with the sign that makes normal . V <= 0 (it faces the sensors; the dot product in double);
 *   when that dot product is exactly 0, the sign that makes its first non-zero component positive.
 *   curvature = l0 / (l0 + l1 + l2).
 *   A voxel has a surfel iff n >= min_points, the exact integer Nxx + Nyy + Nzz > 0, and l1 >= min_planar_ratio * l2 (the ratio
 *   widened to double).  Otherwise its normal is (0, 0, 0) and its curvature 0.
 *   x, y, z, intensity are the bytes loamx_densemap_download gives; with axes 1 the normal is permuted like the position.
 * With moments off every function below except enable_moments and the two host-only helpers answers LOAMX_E_INVALID. */
typedef struct loamx_surfel {
  float x, y, z, intensity, normal_x, normal_y, normal_z, curvature;   /* the order of pcl::PointXYZINormal's fields */
} loamx_surfel;
typedef struct loamx_densemap_surfel_config {
  uint32_t min_points;     /* voxels with fewer points have no surfel, >= 3 (default 5) */
  float min_planar_ratio;  /* >= 0 (default 0.01): below l1 / l2 of it the points form a line */
} loamx_densemap_surfel_config;
void loamx_densemap_surfel_default_config(loamx_densemap_surfel_config* cfg);   /* host only */
/* host only, no device: the surfel of one voxel from its integer words.  idx = the voxel indices ix, iy, iz; vals = n, Sx, Sy, Sz;
 * mom = the nine words in the order above; cfg NULL: the defaults.  LOAMX_E_INVALID: a NULL argument, leaf <= 0, n == 0,
 * min_points < 3, a negative (or NaN) ratio, axes not 0 / 1 */
int loamx_densemap_surfel_of(float leaf, const int32_t idx[3], const uint64_t vals[4], const uint64_t mom[9],
                             const loamx_densemap_surfel_config* cfg, int axes, loamx_surfel* out);
int loamx_densemap_enable_moments(loamx_densemap* h);
/* nine words per voxel in the record order of loamx_densemap_download; *n = voxels (LOAMX_E_CAPACITY, nothing written, when
 * capacity < *n; capacity counts voxels) */
int loamx_densemap_download_moments(loamx_densemap* h, uint64_t* out, uint64_t capacity, uint64_t* n);
/* one surfel per voxel in the record order; capacity / *n as above.  rule NULL: every voxel; a rule requires carving and leaves
 * out the voxels it calls dynamic, as download_static does.  cfg NULL: the defaults */
int loamx_densemap_download_surfels(loamx_densemap* h, loamx_surfel* out, uint64_t capacity, uint64_t* n, int axes,
                                    const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule);
/* binary PCD v0.7, fields x y z intensity normal_x normal_y normal_z curvature (F 4) */
int loamx_densemap_save_pcd_surfels(loamx_densemap* h, const char* path, int axes, const loamx_densemap_surfel_config* cfg,
                                    const loamx_densemap_static_rule* rule);

/* Frozen snapshot and alignment (optional: a handle that never freezes behaves, allocates and exports as described above).  The
 * surfels are what a point-to-plane registration needs; a frozen copy of them on the device turns the map into something a cloud
 * can be aligned to: a loop-closure candidate verified as a 6-DOF constraint, or a sweep with a rough pose re-localised.
 *
 * loamx_densemap_freeze needs moments (a non-NULL rule also carving; otherwise LOAMX_E_INVALID).  It waits for the adds as
 * download_surfels does and computes the surfels on the host exactly as download_surfels does in axes 0 with the same cfg / rule
 * (seconds on a map of millions of voxels: freeze every N sweeps, not every sweep).  The voxels that have a surfel (a non-zero normal)
 * and that the rule does not call dynamic go into a second open-addressing table on the device, independent of the map's: the key is
 * the voxel's key in the map's table, the payload the six f32 mean x, y, z, normal x, y, z with the bytes download_surfels gives.
 * One entry is 32 bytes; the table has the smallest power of two of slots that is >= 2 * count and >= 1024.  A second freeze replaces
 * the first; reset and destroy drop the snapshot; adds, growth, prune and enable_* never touch it: the snapshot is what the map looked
 * like when it was frozen (a loop closure must not match against the drifted recent sweeps).  *n_surfels (may be NULL) = entries.
 *
 * loamx_densemap_align_step: one linearisation of the point-to-plane problem about the pose (R, t) with centre c, rtc = R row-major,
 * t, c.  Per point p, independently, in f32, no fused multiply-add, in this order:
 *   d = p - c per component;  a_k = (R_k0*d_x + R_k1*d_y) + R_k2*d_z;  p' = a + t.  (With c = t_in, a is the lever arm about the sensor.)
 *   If not (|a_k| < 1024 for every k): the point counts as FAR (NaN too) and is done.
 *   i_k = floorf(p'_k * inv), inv = 1.0f / leaf as in the insert.  If not (|i_k| < 2^20 for every k): OUTSIDE, done.
 *   Candidate cells: neighbourhood 0: the cell (i_x, i_y, i_z); 1: the 27 cells (i_x+dx, i_y+dy, i_z+dz), dz the outer loop, then
 *   dy, then dx, each running -1, 0, 1; a cell with an index outside the key range is skipped.  Any other value: LOAMX_E_INVALID.
 *   For each candidate found in the snapshot: e = p' - mean, d2 = (e_x*e_x + e_y*e_y) + e_z*e_z.  The smallest d2 wins, a tie goes
 *   to the earlier candidate (strict <).  No candidate found: UNMATCHED, done.
 *   r = (n_x*e_x + n_y*e_y) + n_z*e_z.  If not (fabsf(r) <= max_residual): REJECTED, done.  Otherwise MATCHED.
 *   (max_residual outside (0, 16]: LOAMX_E_INVALID.)
 *   J = (a_y*n_z - a_z*n_y, a_z*n_x - a_x*n_z, a_x*n_y - a_y*n_x, n_x, n_y, n_z): d r / d (w, v) for R <- exp([w]) R, t <- t + v.
 *   A matched point adds 28 integers to sums: the 21 products J_k*J_l, k <= l, row-major upper triangle, each as
 *   (int64)rintf(prod * 65536.0f);  the six J_k*r as (int64)rintf(prod * 16777216.0f);  r*r as (int64)rintf(prod * 16777216.0f).
 *   Every product is one f32 multiply and the scaling by a power of two is exact.  Bounds: |a_k| < 2^10 and |n| = 1 give
 *   |J_k| < 2^11, |r| <= 2^4, so a term is at most 2^38 (J J), 2^39 (J r), 2^32 (r r): the 64-bit sums are exact for clouds below
 *   2^20 points (and far beyond).
 * counts = FAR, OUTSIDE, UNMATCHED, REJECTED, MATCHED; they add up to the cloud's count.  sums and counts are integer sums: they
 * depend on neither the thread schedule nor the order of the points.  The call blocks until the 33 words are back.
 *
 * loamx_densemap_align_solve (host only): in double, H = sums[0..21) / 2^16 (symmetric 6x6), g = sums[21..27) / 2^24; the
 * eigen-decomposition of H (cyclic Jacobi); directions with l <= degenerate_ratio * l_max (or l <= 0) are dropped from the update
 * and counted in *dropped (LOAM's degeneracy handling);  x = - sum over the kept directions of v (v . g) / l.  degenerate_ratio
 * outside [0, 1): LOAMX_E_INVALID.
 *
 * loamx_densemap_align: Gauss-Newton over align_step and align_solve from pose_in (row-major 3x4, map <- cloud: x -> R x + t').  The
 * host keeps R, t in double, t = R c + t'_in with c = centre (NULL: 0), rounds them to f32 for each step, updates
 * R <- exp([x_0..2]) R (Rodrigues), t <- t + x_3..5, and ends as converged (status 0) when |x_0..2| < eps_rot and |x_3..5| < eps_trans.
 * A step with fewer than min_matched matches ends the loop with status 2 and the pose of the last good iteration (the input pose
 * when it is the first).  pose reports t' = t - R c.  The loop BLOCKS the caller: one launch and one small readback per iteration.
 * The from_* forms read the registered cloud of a mapper / a pipeline slot where it lies (as add_from_map / add_from_pipeline do),
 * behind an event on its stream, with its origin as the centre; pose_in NULL: identity.  LOAMX_SKIPPED when there is no cloud,
 * LOAMX_E_INVALID on another device.  Without a snapshot align_step and the three align forms answer LOAMX_E_INVALID. */
int loamx_densemap_freeze(loamx_densemap* h, const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule,
                          uint64_t* n_surfels);
int loamx_densemap_frozen_size(loamx_densemap* h, uint64_t* n_surfels);   /* 0 when nothing is frozen */
int loamx_densemap_align_step(loamx_densemap* h, const loamx_cloud* points, const float rtc[15], uint32_t neighbourhood,
                              float max_residual, int64_t sums[28], uint64_t counts[5]);
typedef struct loamx_densemap_align_config {
  uint32_t max_iterations;   /* 1..1000 (default 20) */
  uint32_t neighbourhood;    /* 0 or 1 (default 1) */
  float max_residual;        /* metres, (0, 16]; 0 = the leaf (default 0) */
  uint32_t min_matched;      /* default 50 */
  float eps_rot, eps_trans;  /* default 1e-5 rad, 1e-5 m */
  float degenerate_ratio;    /* [0, 1) (default 1e-4) */
} loamx_densemap_align_config;
typedef struct loamx_densemap_align_result {
  double pose[12];           /* row-major 3x4, map <- cloud: x -> R x + t' */
  uint32_t iterations, degenerate_dims;   /* steps run; directions dropped by the last solve */
  int status;                /* 0 converged, 1 max_iterations reached, 2 fewer than min_matched matches */
  double rms;                /* sqrt(sum r^2 / matched) of the last step (0 without a match) */
  uint64_t counts[5];        /* of the last step */
} loamx_densemap_align_result;
void loamx_densemap_align_default_config(loamx_densemap_align_config* cfg);   /* host only */
int loamx_densemap_align_solve(const int64_t sums[28], float degenerate_ratio, double x[6], uint32_t* dropped);   /* host only */
int loamx_densemap_align(loamx_densemap* h, const loamx_cloud* points, const double pose_in[12], const float centre[3] /* NULL: 0 */,
                         const loamx_densemap_align_config* cfg /* NULL: the defaults */, loamx_densemap_align_result* out);
int loamx_densemap_align_from_map(loamx_densemap* h, loamx_map* m, const double pose_in[12] /* NULL: identity */,
                                  const loamx_densemap_align_config* cfg, loamx_densemap_align_result* out);
int loamx_densemap_align_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot, const double pose_in[12],
                                       const loamx_densemap_align_config* cfg, loamx_densemap_align_result* out);

/* Many start poses at once (optional: a handle that never calls these runs the kernels it ran and allocates what it allocated).  The
 * basin of loamx_densemap_align is a few leaves wide; a loop candidate of loamx_place (a yaw hint quantised to 2 pi / n_sectors, no
 * translation) or a sweep to be re-localised in a loaded map needs many starts tried and the best kept.  Every hypothesis is
 * independent and every word of a step is an integer sum, so the batched forms are defined by the single ones, to the bit.
 *
 * loamx_densemap_align_step_many: the linearisation of align_step about n_poses poses, rtc[15 k ..] = R row-major, t, c of pose k
 * (1 <= n_poses <= LOAMX_ALIGN_MAX_POSES).  The cloud is staged once; one memset, ONE launch (kernel k_dm_align_step_many: the poses
 * lie in a table in device memory, a second grid dimension runs over them) and one readback through pinned memory cover all poses.
 * sums[28 k ..] and counts[5 k ..] are exactly the words loamx_densemap_align_step gives for rtc[15 k ..]: the same f32 expressions in
 * the same order, the same candidate order and tie rule, the same fixed-point scaling.  The order of the poses changes nothing but the
 * order of the outputs.  An empty cloud gives zeros and no launch.
 *
 * loamx_densemap_align_many: the Gauss-Newton loop of loamx_densemap_align for the n_poses start poses poses_in[12 k ..] in lockstep.
 * In iteration it = 0, 1, ... the hypotheses that have not ended — a hypothesis ends when it converged, when a step gave it fewer than
 * min_matched matches, or after max_iterations steps — are compacted in ascending index; the f32 roundings of their R, t, c go up in
 * one copy, one launch linearises them, one readback of 33 * n_active words returns, and the host solves and updates each one in double
 * with the functions of the single loop.  out[k] is byte for byte what loamx_densemap_align returns for poses_in[12 k ..] with the same
 * cloud, centre and cfg: pose, iterations, degenerate_dims, status, rms and counts.  A call whose longest hypothesis runs I iterations
 * costs I launches and I blocking readbacks, whatever n_poses.
 * The from_* forms read the registered cloud where it lies, behind an event, as align_from_* do, with its origin as the centre;
 * poses_in NULL is allowed only with n_poses == 1 and means the identity.  LOAMX_SKIPPED without a cloud, LOAMX_E_INVALID on another
 * device.
 *
 * loamx_densemap_align_best (host only): the candidates are the results with status != 2; the best is the one with the largest
 * counts[4] (matched), then the smallest rms, then the smallest index.  *best = UINT32_MAX when there is no candidate (n == 0
 * included), which is still LOAMX_OK.  align_many and its from_* forms write the same value to *best (may be NULL).
 * A CONVERGED STATUS IS NOT EVIDENCE OF A CORRECT POSE: a start in the wrong basin converges too (a box's half-turn look-alike
 * converges with every point matched).  The inlier count and the rms are the evidence; which threshold on them accepts a loop is the
 * host's decision.
 *
 * loamx_densemap_get_align_stats: three counters that run from the handle's creation (reset does not clear them), counted by the
 * single-pose functions too: stats[0] launches of either step kernel, stats[1] readbacks of accumulator words, stats[2] pose-steps
 * (the sum of n_active over the launches; a single step counts 1).
 *
 * Refused with LOAMX_E_INVALID, a message that names the argument, and nothing written: a NULL argument (centre, cfg, best and the
 * from_* forms' poses_in as stated above excepted); n_poses == 0 or > LOAMX_ALIGN_MAX_POSES; neighbourhood, max_residual and cfg as for
 * the single forms; a start pose that is not finite (the whole call); no snapshot.
 *
 * Start poses for a place-recognition match (Python: loamx.pose_grid): with the stored entry's sweep registered at P_e = (R_e, t_e),
 * sensor origin o_e, and a query whose loamx_place match reports yaw_hint, the query's pose is near R = Ry(+yaw_hint) R_e, Ry = rot_y
 * of the pose convention (about +y, turning +z towards +x), with the sensor origin at o_e: shift k of a match corresponds to the
 * query cloud being the stored cloud rotated by -k * 2 pi / S about +y, that is to the query sensor having turned by +k * 2 pi / S.
 * The hint is used as it is, with its sign (a cloud rotated by +k steps gets shift S - k).  Exact for a levelled stored pose (R_e a
 * rotation about +y), to first order in its pitch and roll otherwise. */
#define LOAMX_ALIGN_MAX_POSES 4096
int loamx_densemap_align_step_many(loamx_densemap* h, const loamx_cloud* points, const float* rtc /* 15 * n_poses */, uint32_t n_poses,
                                   uint32_t neighbourhood, float max_residual, int64_t* sums /* 28 * n_poses */, uint64_t* counts /* 5 * n_poses */);
int loamx_densemap_align_many(loamx_densemap* h, const loamx_cloud* points, const double* poses_in /* 12 * n_poses */, uint32_t n_poses,
                              const float centre[3] /* NULL: 0 */, const loamx_densemap_align_config* cfg,
                              loamx_densemap_align_result* out /* n_poses */, uint32_t* best /* may be NULL */);
int loamx_densemap_align_many_from_map(loamx_densemap* h, loamx_map* m, const double* poses_in, uint32_t n_poses,
                                       const loamx_densemap_align_config* cfg, loamx_densemap_align_result* out, uint32_t* best);
int loamx_densemap_align_many_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot, const double* poses_in, uint32_t n_poses,
                                            const loamx_densemap_align_config* cfg, loamx_densemap_align_result* out, uint32_t* best);
int loamx_densemap_align_best(const loamx_densemap_align_result* results, uint32_t n, uint32_t* best);   /* host only, no device */
int loamx_densemap_get_align_stats(loamx_densemap* h, uint64_t stats[3]);

/* Coarser levels and coarse-to-fine alignment (optional: a handle that never calls these runs the kernels it ran and allocates what
 * it allocated).  loamx_densemap_align finds its correspondences in the point's own cell or its 27 neighbours, at the map's one leaf:
 * a start more than about a leaf and a half off matches nothing, or the wrong wall.  A coarser copy of the map has a wider basin and
 * a blunter minimum; aligning against the coarse copy first and handing the pose down level by level has both the reach of the coarse
 * level and the accuracy of the fine one.
 *
 * Levels.  A level-l voxel (l >= 1) has the leaf leaf * 2^l (one f32 multiply by a power of two) and the indices I = i >> 1 of its
 * level-(l-1) children (level 0 is the map; the shift is arithmetic: floor for negative indices).  Its thirteen words are the sums,
 * over the children it has, of these per-child integers, with b_a = i_a & 1 and n, S, M, V the child's words:
 *     n'    += n
 *     S'_a  += (S_a >> 1) + n * b_a * 2^19
 *     M'_ab += (M_ab >> 2) + b_a * 2^18 * S_b + b_b * 2^18 * S_a + n * b_a * b_b * 2^38     (mod 2^64, as M)
 *     V'_a  += V_a                                                                          (signed, as V)
 * This is the child's sum of q and of q_a q_b re-expressed in the parent's own 20-bit units, q' = q/2 + b * 2^19, with one floor per
 * child and word.  So a level-l voxel has exactly the format of a level-0 voxel whose leaf is leaf * 2^l; its offsets stay below 2^20;
 * its sums are exact while it holds fewer than 2^24 points; loamx_densemap_surfel_of(leaf * 2^l, I, vals, mom, ...) gives its surfel;
 * and every word is an integer sum that depends on no order.  For points whose offsets are even at every level (coordinates that are
 * multiples of leaf / 2^(20 - l)) every floor is a no-op and level l is, word for word, the map a handle of leaf * 2^l builds.
 * Level 1 is taken from the map's table and leaves out the voxels the rule calls dynamic (rule NULL: every voxel; a rule needs
 * carving); level l + 1 is taken from level l.  One kernel, k_dm_coarsen, serves every level: one thread per source slot; an occupied,
 * selected slot finds or claims its parent's key in a fresh table and adds its thirteen integers with 64-bit atomics.  The fresh table
 * has the smallest power of two of slots that is >= 2 * the source's occupancy and >= 1024, so it never grows; a probe bound reached
 * is LOAMX_E_INTERNAL.  The live table is only read.
 *
 * loamx_densemap_coarsen: waits for the adds as download does, runs the cascade up to `level` (1 .. LOAMX_PYRAMID_MAX_LEVELS - 1) and
 * returns that level's voxels in ascending key order: keys[i], vals[4 i ..] = n, Sx, Sy, Sz, mom[9 i ..] in the order of
 * download_moments.  *n = voxels; LOAMX_E_CAPACITY, nothing written, when capacity < *n (keys, vals, mom may be NULL with capacity 0).
 * Needs moments.  With loamx_densemap_surfel_of it is a coarser surfel export.
 *
 * loamx_densemap_freeze_pyramid: `levels` snapshots (1 .. LOAMX_PYRAMID_MAX_LEVELS, default 3).  Level 0 is built by the code of
 * loamx_densemap_freeze with the same cfg / rule and is byte for byte that snapshot; with levels == 1 the call is loamx_densemap_freeze
 * (no further launch, no further copy).  Level l >= 1 is a snapshot of its own with the same entry format and slot rule: the voxels
 * of level l that have a surfel under cfg at the leaf leaf * 2^l, under the level's own keys; with max_curvature > 0 a voxel whose
 * surfel has a larger curvature gets no entry (a coarse voxel that spans a corner is no plane; 0 = no limit; level 0 is not
 * filtered).  n_surfels (may be NULL) receives `levels` entry counts.  loamx_densemap_freeze, loamx_densemap_reset and destroy drop the
 * coarse levels.  loamx_densemap_frozen_levels: how many levels stand, 0 = nothing frozen, 1 after a plain freeze.
 *
 * loamx_densemap_align_select_level: every alignment form above (align_step, align_step_many, align, align_many and their from_*
 * forms) reads the table of the selected level, with inv = 1.0f / (leaf * 2^level) and max_residual 0 meaning that level's leaf; the
 * kernels are the same.  The selection is 0 after every freeze of either kind and after reset; a level that does not stand is
 * LOAMX_E_INVALID.  With the selection at 0 every word of every call above is what it was.  loamx_densemap_get_align_stats sums
 * over the levels.
 *
 * loamx_densemap_align_pyramid: for level = first_level down to 0 the loop of loamx_densemap_align against that level; the start is
 * pose_in for the first level and after that the pose the level before reported (after status 2 that is its last good pose, so a level
 * that matched too little hands its input on).  out[k] is the result at level first_level - k (first_level + 1 results), byte for
 * byte what loamx_densemap_align_select_level(level) + loamx_densemap_align returns from the same start: that is the definition.  cfg
 * is applied at every level (max_residual 0: each level's leaf).  The cloud is staged once.  The selected level is neither read nor
 * changed.  The from_* forms as align_from_*: pose_in NULL is the identity, LOAMX_SKIPPED without a cloud.
 * A pyramid over many start poses composes from align_select_level and align_many.
 *
 * LOAMX_E_INVALID, with a message, nothing written and the handle unchanged: a NULL argument (rule, cfg, pyramid, centre, n_surfels
 * and the from_* forms' pose_in excepted); level 0 or >= LOAMX_PYRAMID_MAX_LEVELS for coarsen; levels outside 1 ..
 * LOAMX_PYRAMID_MAX_LEVELS; a negative (or NaN) max_curvature; moments off; a rule without carving; a level or first_level that does
 * not stand; cfg as for loamx_densemap_align at any of the levels; a pose that is not finite. */
#define LOAMX_PYRAMID_MAX_LEVELS 6
typedef struct loamx_densemap_pyramid_config {
  uint32_t levels;        /* snapshots to build, 1 .. LOAMX_PYRAMID_MAX_LEVELS (default 3) */
  float max_curvature;    /* levels >= 1: no entry for a surfel with a larger curvature; >= 0, 0 = no limit (default 0) */
} loamx_densemap_pyramid_config;
void loamx_densemap_pyramid_default_config(loamx_densemap_pyramid_config* cfg);   /* host only */
int loamx_densemap_coarsen(loamx_densemap* h, uint32_t level, const loamx_densemap_static_rule* rule /* NULL: every voxel */,
                           uint64_t* keys, uint64_t* vals /* 4 per voxel */, uint64_t* mom /* 9 per voxel */, uint64_t capacity,
                           uint64_t* n);
int loamx_densemap_freeze_pyramid(loamx_densemap* h, const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule,
                                  const loamx_densemap_pyramid_config* pyramid /* NULL: the defaults */, uint64_t* n_surfels /* levels */);
int loamx_densemap_frozen_levels(loamx_densemap* h, uint32_t* levels);
int loamx_densemap_align_select_level(loamx_densemap* h, uint32_t level);
int loamx_densemap_align_pyramid(loamx_densemap* h, const loamx_cloud* points, const double pose_in[12], const float centre[3] /* NULL: 0 */,
                                 const loamx_densemap_align_config* cfg, uint32_t first_level,
                                 loamx_densemap_align_result* out /* first_level + 1 */);
int loamx_densemap_align_pyramid_from_map(loamx_densemap* h, loamx_map* m, const double pose_in[12] /* NULL: identity */,
                                          const loamx_densemap_align_config* cfg, uint32_t first_level, loamx_densemap_align_result* out);
int loamx_densemap_align_pyramid_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot, const double pose_in[12],
                                               const loamx_densemap_align_config* cfg, uint32_t first_level,
                                               loamx_densemap_align_result* out);

/* A prior map: native save / load, and the exact merge of two maps (optional: a handle that never calls them runs the kernels it
 * ran).  Every word of a voxel is an integer sum, so the map can be written out and read back without loss, and two maps of the same
 * leaf can be combined by adding words per key.
 *
 * File ('LXDM', version 1), little-endian, of exactly this size (no trailing bytes).  Header, 128 bytes:
 *     0 "LXDM"            4 u32 version = 1        8 u32 flags (1 carving, 2 moments)        12 f32 leaf
 *    16 u64 count        24 u64 points offered    32 u64 dropped by range                    40 u64 dropped outside the key range
 *    48 u64 carve_stats[6] in the order of get_carve_stats       96 f32 carve max_range, u32 ray_stride, end_margin, max_steps
 *   112 16 reserved bytes, zero.        Without carving the bytes 48 .. 111 are zero.
 * Body, every array in ascending key order (the record order of loamx_densemap_download):  u64 keys[count];  u64 vals[4 * count]
 * (n, Sx, Sy, Sz per voxel);  with carving u32 miss[count], zero-padded to a multiple of 8 bytes;  with moments u64 mom[9 * count],
 * the words loamx_densemap_download_moments gives.  Stamps and the sequence number of the calls are not stored: a stamp only matters
 * while it equals the sequence number of the call in progress, so a loaded or merged-in voxel gets stamp 0, which is equivalent for
 * every add that follows.
 * Determinism: the file has the same bytes whatever the thread schedule, the order of the points, the split into calls (for
 * everything but miss, as above), the size of the table and the number of rehashes behind the map.
 *
 * loamx_densemap_save waits for the adds as download does, writes to a temporary name beside `path` and renames it: a save that
 * fails leaves nothing under `path`.  Pruned voxels are not in the file.  The frozen snapshot is not saved: the surfels are a function
 * of the words, so a freeze after a load reproduces it bit for bit.
 *
 * loamx_densemap_file_info (host only, no device): the header of a file.  deep == 0 checks the header and the exact size of the
 * file: magic, version, flags within {1, 2}, leaf finite and > 0, reserved bytes zero, with carving a configuration that
 * enable_carving accepts (without: zero bytes), count <= 2^30.  deep != 0 also reads every record: keys strictly ascending, each
 * < 2^63 with each of its three 21-bit fields in [1, 2^21 - 1], every n >= 1.  Any failure: LOAMX_E_INVALID with a message that names
 * the field.  load and merge_file run the deep check before anything touches the device.
 *
 * loamx_densemap_load: h must be empty (fresh, or right after reset) and its leaf must have the bits of the file's.  load enables on h
 * whichever of carving and moments the file has and h has not, and h carves with the file's configuration from then on; a handle
 * that has a feature the file lacks: LOAMX_E_INVALID.  count > max_voxels (with a cap): LOAMX_E_CAPACITY.  A refused load leaves the
 * handle unchanged.  The table gets the smallest power of two of slots that is >= initial_slots and >= 2 * count.  Afterwards
 * get_stats (but for slots), get_carve_stats and every export (download*, save_pcd*, download_moments, download_misses,
 * download_surfels, save) give what the saving handle gave, and later adds behave as they would have on the saving handle.
 *
 * loamx_densemap_merge(dst, src): per key of src the voxel of dst (created when absent) receives n += n, S* += S* and the nine moment
 * words modulo 2^64 and miss += miss modulo 2^32; it keeps its stamp (0 for a new voxel).  dst's three point statistics and six
 * carve statistics grow by src's.  src is only read; the frozen snapshots of both stay as they are.  n, S* and the moment words of
 * the result are those of one map fed with every add of both maps, in any order.  The miss words are the SUMS of the two maps' miss
 * words, which is not what carving the joint sequence of calls would have counted: neither map's rays saw the other's voxels.
 * LOAMX_E_INVALID, dst unchanged: dst and src are the same handle, live on different devices, differ in a bit of the leaf, or do not
 * have the same features enabled (carving on in both or off in both; moments alike).  LOAMX_E_CAPACITY, dst unchanged: with a cap,
 * voxels(dst) + voxels(src) > max_voxels (the bound before common keys are known, as an add counts its points before filtering).
 * The call waits for the adds of both handles and returns when dst holds the result.  Growth follows the add's rule: the table
 * doubles on the device, before the merge, until voxels(dst) + voxels(src) is at most one half of the slots.
 * loamx_densemap_merge_file(dst, path): the same with the records of a file as the source (its flags must equal dst's features); the
 * records go up through pinned memory.  load is merge_file into an empty handle plus the enabling. */
struct loamx_densemap_file_info {   /* (a struct tag only: the name is the function's) */
  uint32_t version, flags;          /* flags: 1 carving, 2 moments */
  float leaf;
  uint64_t voxels;
  uint64_t offered, dropped_range, dropped_key;
  uint64_t carve_stats[6];
  loamx_densemap_carve_config carve;
};
int loamx_densemap_save(loamx_densemap* h, const char* path);
int loamx_densemap_load(loamx_densemap* h, const char* path);
int loamx_densemap_merge(loamx_densemap* dst, loamx_densemap* src);
int loamx_densemap_merge_file(loamx_densemap* dst, const char* path);
int loamx_densemap_file_info(const char* path, struct loamx_densemap_file_info* info, int deep);   /* host only, no device */

/* Ray casts (optional: a handle that never casts a ray runs the kernels it ran, allocates what it allocated and exports the same
 * bytes).  "From here, in this direction, what is the first surface of the map, and how far?" answered on the device, without a
 * download: a live sweep checked against a prior map (a return that stops in front of the mapped surface is a new object, one that
 * goes through it a removed one), a line of sight between two poses, the range image a lidar would see from a pose.
 *
 * Ray i runs from origin to ends[i], both in the map frame: a sweep and its sensor position, exactly as loamx_densemap_add takes
 * them.  Per ray, independently, in f32, no fused multiply-add, / and sqrtf correctly rounded, inv = 1.0f / leaf, in this order:
 *   If a component of the end is not finite, or the end's cell fails |floorf(p_a * inv)| < 2^20 on some axis: NOT_TRACED, done.
 *   The walk of the carving section above runs, unchanged: the same so, sp, c0, c1, rem, s, tmax, tdelta, the same tie rule, and
 *   exactly n_steps integer steps.  If the origin's cell fails the key rule, or n_steps > max_steps: NOT_TRACED, done.
 *   Cell k is the cell after k steps.  The cells k = skip_steps .. n_steps are looked up in the live table, read-only: unlike
 *   carving, the end cell is included.  No cell is looked up when skip_steps > n_steps.
 *   The first cell k that is in the table, holds n >= min_points points and, with a rule, is not dynamic under it (the rule of the
 *   carving section, on the voxel's n and miss) ends the ray: HIT when k < n_steps, HIT_END when k == n_steps.
 *   No such cell: MISS.
 * The record of a hit: key = the voxel's key;  x, y, z = its exported position, computed on the device in double exactly as the
 * export does, x = (float)(((double)ix + (double)Sx / ((double)n * 2^20)) * (double)leaf) (y, z alike): the bytes
 * loamx_densemap_download gives in axes 0;  with d = p - o and e = (x, y, z) - o per component, L2 = (d_x*d_x + d_y*d_y) + d_z*d_z,
 * range = L2 == 0 ? 0 : ((d_x*e_x + d_y*e_y) + d_z*e_z) / sqrtf(L2): the metres along the ray to the foot of that position (it may
 * be negative for a hit in the origin's own cell);  n = the voxel's point count, saturated at 2^32 - 1;  miss = its miss word (0 with
 * carving off);  steps = k.  The position is the MEAN of the voxel's points, not a surface: range is good to about half a leaf.
 * Without a hit key, x, y, z, range, n and miss are 0, and steps is the number of cells looked up (0 when NOT_TRACED).
 * counts = NOT_TRACED, MISS, HIT, HIT_END, cells looked up (over all rays, those of a hit up to and including its cell).  The
 * first four add up to the cloud's count.  All five are integer sums: they depend on neither the thread schedule nor the order of the
 * rays.  Records and counts depend on the map's words only, not on the table's size, the number of rehashes or the order of the adds
 * (miss depends on the call history, as documented above).  An empty map is valid: every traced ray is a MISS.
 * Ordering: the call waits for the adds as download does, runs on the map's own stream and blocks until the five words and, with
 * out != NULL, the records are back (through pinned memory): out[i] belongs to ray i.  out may be NULL: counts only.  An empty
 * cloud: LOAMX_OK, zero counts, no launch.  The from_* forms read the registered cloud of a mapper / a pipeline slot where it lies,
 * with its origin, behind an event on its stream (as add_from_map / add_from_pipeline pick it); LOAMX_SKIPPED when there is no cloud,
 * LOAMX_E_INVALID on another device.
 * LOAMX_E_INVALID, with a message that names the argument: NULL h, ends (m, p), origin or counts;  max_steps outside 1..65536;
 * min_points == 0;  a rule with den == 0;  a rule on a handle without carving.  LOAMX_E_CAPACITY, nothing written: out != NULL and
 * capacity < the cloud's count.  A refused call leaves the map as it was. */
#define LOAMX_RAY_NOT_TRACED 0
#define LOAMX_RAY_MISS 1
#define LOAMX_RAY_HIT 2
#define LOAMX_RAY_HIT_END 3
typedef struct loamx_ray_hit {      /* 40 bytes */
  uint64_t key;                     /* the hit voxel's key; 0 without a hit */
  float x, y, z;                    /* its position: the bytes loamx_densemap_download gives in axes 0; 0 without a hit */
  float range;                      /* metres along the ray to the foot of that position; 0 without a hit */
  uint32_t n;                       /* its point count, saturated at 2^32 - 1 */
  uint32_t miss;                    /* its miss word (0 with carving off) */
  uint32_t steps;                   /* k of the hit cell; without a hit: cells looked up */
  uint32_t status;                  /* 0 NOT_TRACED, 1 MISS, 2 HIT (before the end cell), 3 HIT_END (in the end cell) */
} loamx_ray_hit;
typedef struct loamx_densemap_raycast_config {
  uint32_t max_steps;    /* rays with more steps are not traced, 1..65536 (default 4096) */
  uint32_t skip_steps;   /* cells k < skip_steps are not looked up (the sensor's own voxels) (default 0) */
  uint32_t min_points;   /* a voxel with fewer points is transparent, >= 1 (default 1) */
} loamx_densemap_raycast_config;
void loamx_densemap_raycast_default_config(loamx_densemap_raycast_config* cfg);   /* host only */
int loamx_densemap_raycast(loamx_densemap* h, const loamx_cloud* ends, const float origin[3],
                           const loamx_densemap_raycast_config* cfg /* NULL: the defaults */,
                           const loamx_densemap_static_rule* rule /* NULL: every voxel; else needs carving */,
                           loamx_ray_hit* out /* may be NULL: counts only */, uint64_t capacity, uint64_t counts[5]);
int loamx_densemap_raycast_from_map(loamx_densemap* h, loamx_map* m, const loamx_densemap_raycast_config* cfg,
                                    const loamx_densemap_static_rule* rule, loamx_ray_hit* out, uint64_t capacity, uint64_t counts[5]);
int loamx_densemap_raycast_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot,
                                         const loamx_densemap_raycast_config* cfg, const loamx_densemap_static_rule* rule,
                                         loamx_ray_hit* out, uint64_t capacity, uint64_t counts[5]);

/* Sweep log and rebuild (optional: a handle that never calls loamx_densemap_enable_history runs the kernels it ran, allocates what
 * it allocated and exports the same bytes).  The map keeps sums per voxel, not sweeps; with history on it also keeps every added
 * cloud in device memory, and loamx_densemap_rebuild replays that log under one rigid correction per logged call into a fresh
 * table: after a loop closure (loamx_place -> loamx_densemap_align_many -> loamx_posegraph_optimize) the map is made consistent with
 * the corrected poses without a point crossing PCIe.
 *
 * The log.  loamx_densemap_enable_history is allowed only on an empty map (a fresh handle, or right after reset; otherwise
 * LOAMX_E_INVALID and the handle is unchanged), in any order with enable_carving / enable_moments, and stays on until destroy; reset
 * empties the log and keeps history on.  Every add call that reaches the insert is logged (add, add_from_map, add_from_pipeline):
 * its whole cloud as offered, x, y, z, w byte for byte, including the points the range and key filters drop and non-finite ones.
 * Empty clouds, LOAMX_SKIPPED and refused calls are not logged.  The append is a device-to-device copy on the stream of the insert,
 * behind whatever wrote the cloud; the caller is not blocked.  Per logged call the host keeps the first point, the count and the
 * origin; the call index is the running count of logged calls (the carving sequence number minus one).  The log is never rewritten:
 * it holds the points as they were added.  It grows by doubling from initial_points (a new block, a device-to-device copy on the
 * add's stream, the old block freed where the host next waits), never beyond max_bytes: with max_bytes an add whose cloud would take
 * the log past max_bytes / 16 points is refused with LOAMX_E_CAPACITY before anything is enqueued, map and log unchanged.  Point
 * indices are 64-bit.  A map that has no sweeps behind it cannot be rebuilt: loamx_densemap_load and loamx_densemap_merge_file
 * into a handle with history, and loamx_densemap_merge with such a handle as dst, answer LOAMX_E_INVALID (handle unchanged); such a
 * handle as src is fine.  The 'LXDM' file stays at version 1 and does not carry the log.
 * loamx_densemap_history_size: logged calls and logged points.  loamx_densemap_history_download waits for the adds as download
 * does and returns, through pinned memory, the logged bytes of that call (out->count in = capacity, out = the call's count) and its
 * origin; LOAMX_E_CAPACITY when the cloud does not fit (out->count = the call's count, nothing else written), LOAMX_E_INVALID for a
 * call beyond the log or a handle without history.
 *
 * The correction.  A correction is a row-major 3x4 matrix R | t from the map frame to the map frame, x -> R x + t; for logged call k
 * the host computes it in double as P_k(now) * P_k(when added)^-1 (loamx_posegraph_corrections).  Its 12 doubles must be finite; nothing else is checked (the host
 * answers for R being a rotation).  It is rounded to f32 once, entry by entry, and applied per point in f32, no fused multiply-add,
 * in this order:  p'_a = ((R_a0*x + R_a1*y) + R_a2*z) + t_a;  w is untouched.  The call's origin goes through the same expression.
 * A correction whose 12 rounded entries compare equal (==) to the identity's is the identity: that call is replayed from its logged
 * bytes without any arithmetic (non-finite points, signed zeros and payloads stay as they were).  loamx_densemap_correct (host
 * only, no device) is this definition for n packed x, y, z triples (xyz_out may be xyz_in); LOAMX_E_INVALID, nothing written, for a
 * non-finite entry.
 *
 * loamx_densemap_rebuild(h, corrections, n_calls): afterwards the handle holds the map, the three point statistics, the six carve
 * statistics and the sequence number that a fresh handle of the same configuration and features would hold after
 * add(correct(C_k, points_k), correct(C_k, origin_k)) for k = 0, 1, ... in order (corrections NULL: every C_k the identity).  The
 * replay always starts from the logged originals: a second rebuild does not compose with the first, and the log itself is
 * unchanged.  Adds after a rebuild go on as on that fresh handle and are logged as given.  The frozen snapshot is not touched (it
 * still shows the map as it was frozen: freeze again); voxels removed by prune come back (they are in the log: prune again).
 * With carving off every word is independent of the order, and the whole log is replayed in one launch whatever the number of
 * calls: a thread finds its call from its 64-bit point index in a per-call table in device memory (first point, f32 correction,
 * identity flag, corrected origin), transforms in registers and inserts with the range filter about that call's corrected origin.
 * With carving on the calls are replayed in order, one insert launch (stamp k + 1) and one carve launch per call, enqueued back to
 * back.  No transformed copy of the log is made.  The replay goes into a fresh table with its own counter words, of the smallest
 * size, by doubling from initial_slots, that holds the voxels the map has now at a load of one half.  Before probing, a kernel reads
 * the running occupancy; once it exceeds half the slots it sets a "too small" word and returns without inserting, so a table that is
 * too small costs bounded work.  The host waits and reads the words: the attempt has failed iff the occupancy exceeds half the
 * slots or the "too small" or the overflow word is set (all three mean: more voxels than half the slots), and is repeated with
 * twice the slots, up to 2^31.  On success the table has the smallest power of two of slots that is >= initial_slots, >= 2 x the
 * voxels before and >= 2 x the voxels after; peak memory is the old table plus the new one.
 * The call waits for the adds as download does, runs on the map's own stream and blocks until the new map stands.
 * LOAMX_E_INVALID, with a message that names the argument: no history; n_calls different from the log's count (with corrections
 * NULL too); a non-finite entry.  LOAMX_E_CAPACITY: with max_voxels, the rebuilt map holds more voxels than the cap.  Any refusal
 * or failure, a failed allocation of the second table included, leaves the handle with its old map, statistics and log.
 * loamx_densemap_get_rebuild_stats: rebuilds that succeeded, tables tried, replay launches, points replayed (the last three over
 * every attempt); they run from the handle's creation and are never cleared. */
typedef struct loamx_densemap_history_config {
  uint64_t max_bytes;       /* cap on the log's device memory; 0 = bounded by device memory only (default 0) */
  uint64_t initial_points;  /* capacity at enabling, >= 1 (default 1 << 20) */
} loamx_densemap_history_config;
void loamx_densemap_history_default_config(loamx_densemap_history_config* cfg);   /* host only */
int loamx_densemap_enable_history(loamx_densemap* h, const loamx_densemap_history_config* cfg /* NULL: the defaults */);
int loamx_densemap_history_size(loamx_densemap* h, uint64_t* calls, uint64_t* points);
int loamx_densemap_history_download(loamx_densemap* h, uint64_t call, loamx_cloud* out /* count in = capacity */, float origin[3]);
int loamx_densemap_correct(const double correction[12], const float* xyz_in, float* xyz_out, uint64_t n);   /* host only, no device */
int loamx_densemap_rebuild(loamx_densemap* h, const double* corrections /* 12 * n_calls; NULL: every call the identity */,
                           uint64_t n_calls);
int loamx_densemap_get_rebuild_stats(loamx_densemap* h, uint64_t stats[4]);

/* Snapshots built on the device, and snapshots of a window of the sweep log (optional: a handle that never calls these runs the
 * kernels it ran, allocates what it allocated and exports the same bytes).  loamx_densemap_freeze brings every voxel's thirteen words
 * to the host, computes the surfels there and sends them back, and what it freezes is always the whole map.  Here the surfels are
 * computed where the words lie, and a snapshot can be made of the sweeps j - w .. j + w of the log alone: a loamx_place match (i, j)
 * becomes freeze_history of the window around j, align_many_from_history of sweep i, and one edge j -> i of the pose graph, without a
 * point crossing to the host.
 *
 * The surfel on the device.  Kernel k_dm_surfels, one thread per slot of a table of the map's format: an occupied slot that the rule
 * does not call dynamic computes its surfel by the definition of "Second moments and surfels" with the host's own operations in the
 * host's order — f64 + - * / sqrt, comparisons, integer -> double conversions (the 128-bit one written out: nearest, ties to even)
 * and one f64 -> f32 rounding per output, no fused multiply-add — each of which is correctly rounded on either side, so the six f32 of
 * an entry are the bytes loamx_densemap_download_surfels gives.  The voxels that have a surfel take consecutive places of two device
 * arrays (key; six f32) through one counter, one atomic per wave; the host reads the count (8 bytes), sizes the snapshot's table by
 * the rule of loamx_densemap_freeze and fills it from the arrays.  The order of the arrays, and with it the slot an entry lands in
 * among the slots of its probe sequence, depends on the schedule; the SET of entries does not, and no alignment word depends on
 * the placement.
 *
 * loamx_densemap_freeze_device: loamx_densemap_freeze with the surfels computed on the device — the same preconditions, waits,
 * refusals and side effects (level 0 is replaced, the coarse levels go, the selection returns to level 0) and the same set of
 * (key, six f32) entries, byte for byte.  loamx_densemap_freeze_pyramid_device: the same for loamx_densemap_freeze_pyramid; the
 * cascade's level tables are read where they stand instead of being downloaded.
 *
 * loamx_densemap_freeze_history(h, first_call, n_calls, corrections, cfg, n_surfels): needs history and moments.  The logged calls
 * [first_call, first_call + n_calls) are replayed by the kernel of loamx_densemap_rebuild, call k OF THE WINDOW under
 * corrections[12 k ..] (NULL: every correction the identity; the checks and the f32 rounding are rebuild's), into a scratch table of
 * the map's format with moment words, no carve words and counters of its own, sized as a rebuild sizes its attempts (doubled on the
 * "too small" word); k_dm_surfels runs on it without a rule, level 0 is built from the result and the scratch table is freed.
 * Afterwards level 0 is the snapshot that a fresh handle of the same loamx_densemap_config with moments on would hold after
 * add(correct(C_k, points_k), correct(C_k, origin_k)) for the window's calls followed by loamx_densemap_freeze(cfg, NULL); the coarse
 * levels go and the selection returns to level 0 as after any freeze.  The live map, its statistics (rebuild's included), its log and
 * its carve words are not touched.  LOAMX_E_INVALID with a message that names the argument: no history, no moments, n_calls == 0, a
 * window that reaches beyond the log, a non-finite correction entry.  LOAMX_E_CAPACITY: with max_voxels, the window holds more voxels
 * than the cap.  After any refusal or failure, a failed allocation included, the old snapshot stands.
 *
 * loamx_densemap_download_frozen: the entries of snapshot level `level` in ascending key order, keys[i] and rec[6 i ..] = mean x, y,
 * z, normal x, y, z.  *n = entries; LOAMX_E_CAPACITY, nothing written, when capacity < *n (keys, rec may be NULL with capacity 0);
 * LOAMX_E_INVALID for a level that does not stand.
 *
 * loamx_densemap_align_from_history, _many_from_history, _pyramid_from_history: the from_* forms of loamx_densemap_align,
 * loamx_densemap_align_many and loamx_densemap_align_pyramid on the points of logged call `call` where they lie in the log, behind
 * the adds, with the call's logged origin as the centre.  Every result is byte for byte what the host-fed form returns for the cloud
 * and origin of loamx_densemap_history_download(call) with centre = that origin (pose_in NULL: the identity, as for the other from_*
 * forms).  LOAMX_E_INVALID: no history, a call beyond the log, no snapshot, and whatever the host-fed form refuses. */
int loamx_densemap_freeze_device(loamx_densemap* h, const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule,
                                 uint64_t* n_surfels);
int loamx_densemap_freeze_pyramid_device(loamx_densemap* h, const loamx_densemap_surfel_config* cfg, const loamx_densemap_static_rule* rule,
                                         const loamx_densemap_pyramid_config* pyramid /* NULL: the defaults */, uint64_t* n_surfels /* levels */);
int loamx_densemap_freeze_history(loamx_densemap* h, uint64_t first_call, uint64_t n_calls,
                                  const double* corrections /* 12 * n_calls; NULL: every call the identity */,
                                  const loamx_densemap_surfel_config* cfg, uint64_t* n_surfels);
int loamx_densemap_download_frozen(loamx_densemap* h, uint32_t level, uint64_t* keys, float* rec /* 6 per entry */, uint64_t capacity,
                                   uint64_t* n);
int loamx_densemap_align_from_history(loamx_densemap* h, uint64_t call, const double pose_in[12] /* NULL: identity */,
                                      const loamx_densemap_align_config* cfg, loamx_densemap_align_result* out);
int loamx_densemap_align_many_from_history(loamx_densemap* h, uint64_t call, const double* poses_in, uint32_t n_poses,
                                           const loamx_densemap_align_config* cfg, loamx_densemap_align_result* out, uint32_t* best);
int loamx_densemap_align_pyramid_from_history(loamx_densemap* h, uint64_t call, const double pose_in[12],
                                              const loamx_densemap_align_config* cfg, uint32_t first_level,
                                              loamx_densemap_align_result* out /* first_level + 1 */);

/* Navigation grid (optional: a handle that never calls loamx_densemap_grid runs the kernels it ran, allocates what it allocated and
 * exports the same bytes).  "Where can I drive?": a window of the map projected along the up axis to a 2-D grid of ground height,
 * obstacle count, overhead clearance, class and squared distance to the nearest obstacle, computed on the device from the table
 * where it lies; only nx * nz records of 24 bytes come back.
 *
 * Up is +y of the LOAM frame (z_s of the sensor axes).  A cell is a square of k = cell_leaves voxels on a side in x and z: voxel
 * (ix, iy, iz) lies in cell (cx, cz) = (floor(ix / k), floor(iz / k)) — floor, not truncation: ix = -1, k = 3 gives cx = -1.  The
 * window is the nx * nz cells cx in [x0, x0 + nx), cz in [z0, z0 + nz); cell (cx, cz) is record (cz - z0) * nx + (cx - x0).
 * A voxel qualifies when it lies in the window, holds n >= min_points points, has y_min <= iy <= y_max and, with a rule, is not
 * dynamic under it (the rule of the carving section, on the voxel's n and miss: loamx_densemap_rule_is_dynamic).
 * Per cell, over its qualifying voxels:
 *   ground    = the smallest iy (INT32_MAX: the cell has none).  The ground is the LOWEST voxel, not a fitted surface: one
 *               qualifying voxel under the road lowers it (min_points, y_min and the rule are the guards against that).
 *   elevation = (float)(((double)ground + (double)SSy / ((double)SSn * 2^20)) * (double)leaf), SSn and SSy the 64-bit sums of n and
 *               Sy over the qualifying voxels with iy == ground: the export expression of loamx_densemap_download on the pooled
 *               ground layer.  0.0f without a ground.
 *   obstacles = the number of qualifying voxels with band_lo <= iy - ground <= band_hi (the leaves above the ground that the
 *               vehicle's body occupies).
 *   overhead  = the smallest iy of a qualifying voxel with iy - ground > band_hi (INT32_MAX: none): what the vehicle passes under.
 *   cls       = UNKNOWN when the cell has no qualifying voxel;  otherwise OBSTACLE when obstacles >= min_obstacle_voxels;  otherwise
 *               STEP when some 4-neighbour (cx +- 1, cz), (cx, cz +- 1) inside the window is not UNKNOWN and
 *               |ground - ground_nb| > max_step;  otherwise FREE.  Both sides of a step are marked.  A step beyond the window's edge
 *               is not seen: the cells of the outermost ring are compared with their neighbours inside the window only.
 *   clear2    = with R = clear_max and D = the smallest dx*dx + dz*dz (in cells) to a cell of the window with cls >= 2:  D when
 *               D <= R*R, else (R+1)*(R+1).  An OBSTACLE or STEP cell has 0.  Cells outside the window are not obstacles.  With
 *               R = 0 this is 0 on obstacles and 1 elsewhere, with no special case.
 * Every field is an integer, or one f32 rounding of an expression over integers: the grid depends on neither the thread schedule,
 * the order of the points, the split into add calls (without a rule: the miss words depend on the call history, as documented
 * above) nor the table's size or the number of rehashes.
 * Ordering: the call waits for the adds as download does, runs four kernels on the map's own stream (ground: atomic minimum per
 * cell; fill: the sums, counts and overhead against the final ground; classify; clear) behind one memset, and blocks until the
 * records are back through pinned memory.  Integer atomics only.  It changes nothing in the map.  The device planes live in the
 * handle, grow to the largest window asked for and are freed on destroy.  An empty map is valid: every cell is UNKNOWN.
 * LOAMX_E_INVALID, with a message that names the argument, nothing written to out: NULL h or out;  a configuration that fails
 * loamx_densemap_grid_check;  a rule with den == 0;  a rule on a handle without carving.
 *
 * loamx_densemap_grid_check (host only): LOAMX_OK, or LOAMX_E_INVALID with a message that names the first field out of its bounds.
 * loamx_densemap_grid_window (host only): x0, nx, z0, nz of the window about a centre with a half extent, both in metres, for
 * cfg->cell_leaves; in double, e = (double)leaf * k, lo = floor(((double)c - (double)h) / e), hi = floor(((double)c + (double)h) / e),
 * x0 = lo, nx = hi - lo + 1 (z alike).  LOAMX_E_INVALID, cfg unchanged, when an argument is not finite, leaf <= 0, half_extent < 0
 * or the result breaks a bound of loamx_densemap_grid_check.
 * loamx_grid_occupancy (host only): the classes as nav_msgs/OccupancyGrid values, -1 UNKNOWN, 0 FREE, 100 OBSTACLE or STEP
 * (LOAMX_E_INVALID, nothing written, for a cls above 3).
 * loamx_write_grid_pgm (host only): stem.pgm and stem.yaml as ROS map_server reads them, in the sensor axes (x_s = LOAM z,
 * y_s = LOAM x).  stem.pgm is binary P5, maxval 255, width nz, height nx; file row r, column u is cell (cx, cz) =
 * (x0 + nx - 1 - r, z0 + u); 0 for OBSTACLE or STEP, 254 for FREE, 205 for UNKNOWN.  stem.yaml holds image (the file name of
 * stem.pgm without its directory), resolution = (double)leaf * k, origin: [z0 * resolution, x0 * resolution, 0], negate: 0,
 * occupied_thresh: 0.65, free_thresh: 0.196; numbers are printed with %.9g. */
#define LOAMX_GRID_UNKNOWN 0
#define LOAMX_GRID_FREE 1
#define LOAMX_GRID_OBSTACLE 2
#define LOAMX_GRID_STEP 3
typedef struct loamx_densemap_grid_config {
  uint32_t cell_leaves;          /* k, 1..64 (default 2) */
  int32_t  x0, z0;               /* first cell of the window, |x0|, |z0| <= 2^21 (default 0, 0) */
  uint32_t nx, nz;               /* 1..8192 each, nx * nz <= 2^26 (default 256, 256) */
  uint32_t min_points;           /* a voxel qualifies when n >= min_points, >= 1 (default 2) */
  int32_t  y_min, y_max;         /* and y_min <= iy <= y_max (default -2^20, 2^20): one storey, or a cut under the road */
  uint32_t band_lo, band_hi;     /* leaves above the ground that the vehicle's body occupies, 1 <= band_lo <= band_hi (default 3, 20) */
  uint32_t min_obstacle_voxels;  /* >= 1 (default 1) */
  uint32_t max_step;             /* leaves (default 2) */
  uint32_t clear_max;            /* R, cells, 0..64 (default 10) */
} loamx_densemap_grid_config;
typedef struct loamx_grid_cell {   /* 24 bytes */
  int32_t  ground;      /* iy of the lowest qualifying voxel of the cell; INT32_MAX: none */
  float    elevation;   /* metres; 0.0f when ground is INT32_MAX */
  uint32_t obstacles;   /* qualifying voxels with band_lo <= iy - ground <= band_hi */
  int32_t  overhead;    /* lowest iy of a qualifying voxel with iy - ground > band_hi; INT32_MAX: none */
  uint32_t clear2;      /* squared distance in cells to the nearest OBSTACLE or STEP cell of the window, capped: see above */
  uint32_t cls;         /* 0 UNKNOWN, 1 FREE, 2 OBSTACLE, 3 STEP */
} loamx_grid_cell;
void loamx_densemap_grid_default_config(loamx_densemap_grid_config* cfg);   /* host only */
int loamx_densemap_grid_check(const loamx_densemap_grid_config* cfg);        /* host only */
int loamx_densemap_grid_window(float leaf, float centre_x, float centre_z, float half_extent, loamx_densemap_grid_config* cfg);   /* host only */
int loamx_densemap_grid(loamx_densemap* h, const loamx_densemap_grid_config* cfg /* NULL: the defaults */,
                        const loamx_densemap_static_rule* rule /* NULL: every voxel; else needs carving */,
                        loamx_grid_cell* out /* nx * nz */);
int loamx_grid_occupancy(const loamx_grid_cell* cells, uint64_t n, int8_t* out);   /* host only */
int loamx_write_grid_pgm(const char* stem, const loamx_grid_cell* cells, const loamx_densemap_grid_config* cfg, float leaf);   /* host only */

/* Routing on the navigation grid (optional: a handle that never routes runs the kernels it ran and allocates what it allocated;
 * loamx_densemap_grid returns the bytes it returned).  "How do I get there?": the cost-to-go of every cell of a window towards a set
 * of goal cells, the next step per cell, and routes traced from many starts, computed on the device from the grid where it lies;
 * only what is asked for comes back.  The input is integer (cls, clear2) and so is the answer: shortest-path costs over integer
 * move costs are a unique fixed point that depends on neither the thread schedule nor the number of relaxation rounds.
 *
 * Cell coordinates are window-relative: rx = cx - x0 in [0, nx), rz = cz - z0 in [0, nz), record rz * nx + rx.
 * Weight of a cell, w(c), 0 = blocked, otherwise 1..32: 0 unless clear2 >= min_clear2 and either cls == FREE, or cls == UNKNOWN
 * with unknown_weight > 0; otherwise w = 1 + p + u, p = floor(soft_weight * (soft_clear2 - clear2) / soft_clear2) when
 * clear2 < soft_clear2, else 0; u = unknown_weight for an UNKNOWN cell, else 0.  loamx_grid_route_weight (host only) is this
 * expression: 0..32, or a negative error for NULL or a configuration that fails its check.
 * Moves: direction d = 0..7 is (dx, dz) = (1,0), (1,1), (0,1), (-1,1), (-1,0), (-1,-1), (0,-1), (1,-1); even d is axial, odd d is
 * diagonal and exists only with connectivity == 8.  A move a -> b is legal when b lies in the window, w(a) > 0 and w(b) > 0 and,
 * for a diagonal, both cells (ax + dx, az) and (ax, az + dz) have w > 0 (no corner cutting).  Its cost is s * (w(a) + w(b)),
 * s = 5 axial, 7 diagonal: 10 / 14 on unit weights, and symmetric, so the cost to the goal is also the cost from it.
 * Goals: n_goals pairs (rx, rz), 1 <= n_goals <= 4096.  A pair outside the window or on a blocked cell is ignored and not counted
 * in stats[2]; a cell named twice counts twice.  With no goal left every cell is unreachable and the call is still LOAMX_OK.
 * Field: one loamx_route_cell per cell.  cost = the smallest sum of move costs to any used goal, LOAMX_ROUTE_UNREACHABLE for a
 * blocked cell or one with no path.  next = LOAMX_ROUTE_GOAL when cost == 0, LOAMX_ROUTE_NONE when unreachable, otherwise the
 * smallest d whose move c -> nb is legal and has cost[nb] + move == cost[c]; it is derived from the final costs in a pass of its
 * own and does not depend on the schedule either.
 * Routing needs nx * nz <= 2^22: a path visits each cell at most once and a move costs at most 7 * 64 = 448, so
 * cost < 2^22 * 448 < 2^31.  A larger window is LOAMX_E_INVALID.
 * stats[6]: traversable cells (w > 0);  reachable cells;  goals used;  the largest finite cost (0: none);  relaxation rounds
 * launched;  tile runs that did work.  The first four are part of the definition and exact, the last two describe the schedule.
 *
 * loamx_densemap_route: runs the grid of grid_cfg / rule exactly as loamx_densemap_grid does, then routes on it, in one call and
 * with nothing stale; the 24-byte records only come back when out_cells is given.
 * loamx_densemap_route_cells: the same on a grid of the caller's (edited, painted with keep-out zones, or hand-made), uploaded to
 * a buffer of the route's own; nothing that loamx_densemap_grid keeps is replaced or disturbed.
 * loamx_densemap_route_trace: routes over the field of this handle's last successful route call, traced on the device; only the
 * routes come back.  A route is the list of cells from the start, following next, up to and including the goal cell.  lengths[i]
 * is the full number of cells of route i, 0 when the start is outside the window or unreachable.  Of a route longer than capacity
 * only the first capacity pairs are written; lengths[i] still holds the full length, so the caller can ask again.  Start i's
 * slice of out_xz begins at 2 * capacity * i; the words beyond its route are left untouched.
 * loamx_grid_route_trace (host only): the same walk over a field the caller holds, the same bytes.  It stops with
 * LOAMX_E_INVALID, nothing written, on a field that is not one of ours: a next above 9, a step that leaves the window, a step to
 * a cell whose cost is not strictly smaller (which also bounds the walk by nx * nz steps).
 * loamx_grid_route_points (host only): metres for a route, LOAM frame: x = (float)(((double)x0 + rx + 0.5) * (double)leaf * k),
 * z alike, y = the cell's elevation (0 for an UNKNOWN cell or when cells is NULL).
 * loamx_densemap_grid_cell_of (host only): the cell of a position: in double, rx = floor((double)x / ((double)leaf * k)) - x0,
 * z alike; *inside = 0, rx and rz untouched, when the cell is outside the window.
 * Ordering: the route calls wait for the adds as loamx_densemap_grid does, run on the map's own stream, change nothing in the map
 * and block until what was asked for is back through pinned memory.  Integer atomics only.  The planes live in the handle, are
 * allocated by the first route call, grow to the largest window asked for and are freed on destroy.
 * LOAMX_E_INVALID, with a message that names the argument, nothing written to any output: NULL h, goals_xz, starts_xz, lengths, or
 * out_xz with capacity > 0;  n_goals or n_starts outside 1..4096;  a configuration that fails loamx_grid_route_check;  everything
 * loamx_densemap_grid refuses (but for its out);  nx * nz > 2^22;  cells NULL in route_cells;  a cls above 3 in uploaded cells;
 * route_trace on a handle that has no field yet.  LOAMX_E_INTERNAL: the relaxation did not settle within nx * nz + 2 rounds, which
 * the kernel's invariant excludes. */
#define LOAMX_ROUTE_UNREACHABLE 0xffffffffu
#define LOAMX_ROUTE_GOAL 8u
#define LOAMX_ROUTE_NONE 9u
typedef struct loamx_grid_route_config {
  uint32_t connectivity;     /* neighbours used for moves, 4 or 8 (default 8) */
  uint32_t min_clear2;       /* smallest clear2 of a traversable cell, >= 1: OBSTACLE and STEP cells (clear2 0) never qualify (default 1) */
  uint32_t soft_clear2;      /* clear2 below which a cell pays a penalty, 0..4225 (default 0) */
  uint32_t soft_weight;      /* largest penalty, 0..15 (default 0) */
  uint32_t unknown_weight;   /* 0: UNKNOWN cells are blocked; 1..16: they can be driven at that extra weight (default 0) */
} loamx_grid_route_config;
typedef struct loamx_route_cell {   /* 8 bytes */
  uint32_t cost;   /* LOAMX_ROUTE_UNREACHABLE: blocked, or no path */
  uint32_t next;   /* 0..7: the direction of the next step; LOAMX_ROUTE_GOAL; LOAMX_ROUTE_NONE */
} loamx_route_cell;
void loamx_grid_route_default_config(loamx_grid_route_config* cfg);   /* host only */
int loamx_grid_route_check(const loamx_grid_route_config* cfg);        /* host only */
int loamx_grid_route_weight(const loamx_grid_cell* cell, const loamx_grid_route_config* cfg);   /* host only */
int loamx_densemap_route(loamx_densemap* h, const loamx_densemap_grid_config* grid_cfg /* NULL: the defaults */,
                         const loamx_densemap_static_rule* rule /* NULL: every voxel; else needs carving */,
                         const loamx_grid_route_config* cfg /* NULL: the defaults */, const uint32_t* goals_xz, uint32_t n_goals,
                         loamx_grid_cell* out_cells /* nx * nz; NULL: not wanted */, loamx_route_cell* out_field /* nx * nz; NULL: not wanted */,
                         uint64_t stats[6] /* NULL: not wanted */);
int loamx_densemap_route_cells(loamx_densemap* h, const loamx_grid_cell* cells, uint32_t nx, uint32_t nz,
                               const loamx_grid_route_config* cfg /* NULL: the defaults */, const uint32_t* goals_xz, uint32_t n_goals,
                               loamx_route_cell* out_field /* NULL: not wanted */, uint64_t stats[6] /* NULL: not wanted */);
int loamx_densemap_route_trace(loamx_densemap* h, const uint32_t* starts_xz, uint32_t n_starts /* 1..4096 */,
                               uint32_t* out_xz /* n_starts * capacity pairs */, uint32_t capacity, uint32_t* lengths /* n_starts */);
int loamx_grid_route_trace(const loamx_route_cell* field, uint32_t nx, uint32_t nz, uint32_t start_x, uint32_t start_z,
                           uint32_t* out_xz /* capacity pairs */, uint32_t capacity, uint32_t* length);   /* host only */
int loamx_grid_route_points(const loamx_densemap_grid_config* grid_cfg, float leaf, const loamx_grid_cell* cells /* NULL: y = 0 */,
                            const uint32_t* route_xz, uint32_t n, float* out_xyz /* 3 * n */);   /* host only */
int loamx_densemap_grid_cell_of(const loamx_densemap_grid_config* grid_cfg, float leaf, float x, float z, uint32_t* rx, uint32_t* rz,
                                int* inside);   /* host only */

/* Frontiers of the navigation grid (optional: a handle that never asks for them runs the kernels it ran and allocates what it
 * allocated; loamx_densemap_grid and the route calls return the bytes they returned).  "Where do I go when nobody names a cell?":
 * where known free ground meets ground the map has not seen (Yamauchi's frontier-based exploration).  The frontier cells of a window,
 * grouped into connected frontiers, each with its size, box, centroid sums, the width of its opening and the cheapest of its cells to
 * reach, computed on the device from the grid and the field where they lie; a few records of 64 bytes come back.  Every word is an
 * exact function of the grid's integers (cls, clear2) and of the field.
 *
 * Cells, the window and record indices are those of the routing section: a cell is (rx, rz), window-relative, record c = rz * nx + rx.
 * Frontier cell: a cell with cls == LOAMX_GRID_FREE and clear2 >= min_clear2 of whose eight neighbours (rx + dx, rz + dz),
 * |dx|, |dz| <= 1, not both 0, that lie inside the window at least min_unknown have cls == LOAMX_GRID_UNKNOWN.  Cells outside the
 * window are not unknown: a FREE cell on the outermost ring is a frontier cell only on account of neighbours inside the window, the
 * rule STEP follows at the edge.  unknown8(c) is the count of those unknown neighbours, 0..8.
 * Adjacency: two frontier cells are adjacent iff they differ by (dx, dz) with |dx|, |dz| <= 1, not both 0, and |dx| + |dz| <= 1
 * under connectivity == 4, <= 2 under 8.  A cell that is no frontier cell connects nothing.
 * Frontiers: the classes of the transitive closure of adjacency.  A frontier is kept iff it has at least min_cells cells; the kept
 * ones are numbered 0 .. F-1 in ascending min_cell, the smallest record index in them, and out[f] is frontier f.
 * Labels (optional): one uint32_t per cell in record order: the number of the cell's frontier, LOAMX_FRONTIER_NONE for a cell that
 * is no frontier cell or whose frontier was dropped.
 * stats[6]: frontier cells;  frontiers before min_cells;  frontiers kept;  cells in kept frontiers;  kept frontiers with
 * reachable > 0;  hook attempts that lost to another thread.  The first five are part of the definition and exact, the last
 * describes the schedule.
 * The field: move costs are symmetric (the routing section), so the cost from the vehicle to a cell is the cost-to-go of a field whose
 * only goal is the vehicle's cell.  With start_xz given the call routes towards that one goal under route_cfg exactly as
 * loamx_densemap_route_cells would; the field stays in the handle as that call's would and replaces the last one, so
 * loamx_densemap_route_trace from a frontier's best_cell yields the route from the frontier to the vehicle: reversed, the way there.
 * A start outside the window or on a blocked cell is ignored, as a goal is: every frontier then has reachable == 0 and the call is
 * still LOAMX_OK.  With start_xz == NULL nothing is routed, the handle's field is left alone, and reachable, best_cost and
 * best_cell hold 0, LOAMX_ROUTE_UNREACHABLE and LOAMX_FRONTIER_NONE.
 *
 * loamx_densemap_frontiers: runs the grid of grid_cfg / rule exactly as loamx_densemap_grid does, routes when a start is given, and
 * finds the frontiers on the records where they lie on the device; only the kept records cross, and the labels when wanted.
 * loamx_densemap_frontiers_cells: the same on a grid of the caller's, uploaded as loamx_densemap_route_cells uploads; nothing that
 * loamx_densemap_grid keeps is replaced or disturbed.
 * loamx_frontiers_best (host only, no device): *best = the index of the frontier with the smallest best_cost among those with
 * min_cost <= best_cost < LOAMX_ROUTE_UNREACHABLE, ties to the smaller index; LOAMX_FRONTIER_NONE when there is none.  min_cost
 * lets the caller skip the frontier it is standing on.  LOAMX_E_INVALID for a NULL best, or a NULL f with n > 0.
 * Ordering: as loamx_densemap_segment the calls wait for every add, run on the map's own stream and block until the outputs are back
 * through pinned memory.  The map is only read: every export is byte for byte what it was before the call.  Integer atomics only.
 * The work arrays live in the handle, are allocated by the first call, grow to the largest window asked for and are freed on
 * destroy.  labels and out may each be NULL: that output is skipped.  The outputs are written last, all or none.  An all-UNKNOWN
 * grid or an empty map is LOAMX_OK with every count zero.
 * LOAMX_E_INVALID, with a message that names the argument, nothing written to any output: NULL h, n_frontiers or stats;  a
 * configuration that fails loamx_grid_frontier_check (connectivity not 4 or 8;  min_unknown outside 1..8;  min_clear2 or min_cells 0)
 * or loamx_grid_route_check;  everything the grid or the route call under it refuses (cells NULL, a cls above 3);  nx * nz > 2^22
 * when a start is given;  nx * nz > 2^26 always.
 * LOAMX_E_CAPACITY: out given and capacity < F.  Only *n_frontiers is written, and it holds the needed count.
 * LOAMX_E_INTERNAL: a bound of the union-find was reached, which its invariant excludes. */
#define LOAMX_FRONTIER_NONE 0xFFFFFFFFu
typedef struct loamx_grid_frontier_config {
  uint32_t connectivity;   /* grouping of frontier cells, 4 or 8 (default 8) */
  uint32_t min_unknown;    /* UNKNOWN cells among the eight neighbours, 1..8 (default 1) */
  uint32_t min_clear2;     /* a frontier cell has clear2 >= this, >= 1 (default 1) */
  uint32_t min_cells;      /* frontiers with fewer cells are dropped, >= 1 (default 1) */
} loamx_grid_frontier_config;
typedef struct loamx_frontier {   /* 64 bytes */
  uint32_t min_cell;       /* smallest record index of its cells: its identity */
  uint32_t cells;          /* frontier cells in it */
  uint32_t lo[2], hi[2];   /* inclusive box, (rx, rz) */
  uint64_t sum_rx, sum_rz; /* sums of rx and of rz over its cells (the centroid's numerators) */
  uint64_t unknown_links;  /* sum of unknown8 over its cells: how wide the opening is */
  uint32_t reachable;      /* its cells with a finite cost in the field; 0 without a field */
  uint32_t best_cost;      /* smallest cost over its cells; LOAMX_ROUTE_UNREACHABLE: none, or no field */
  uint32_t best_cell;      /* smallest record index among its cells with cost == best_cost; LOAMX_FRONTIER_NONE: none */
  uint32_t reserved;       /* 0 */
} loamx_frontier;
void loamx_grid_frontier_default_config(loamx_grid_frontier_config* cfg);   /* host only */
int loamx_grid_frontier_check(const loamx_grid_frontier_config* cfg);        /* host only; names the first bad field */
int loamx_densemap_frontiers(loamx_densemap* h, const loamx_densemap_grid_config* grid_cfg /* NULL: the defaults */,
                             const loamx_densemap_static_rule* rule /* NULL: every voxel; else needs carving */,
                             const loamx_grid_route_config* route_cfg /* NULL: the defaults */,
                             const loamx_grid_frontier_config* cfg /* NULL: the defaults */, const uint32_t start_xz[2] /* NULL: no routing */,
                             uint32_t* labels /* nx * nz; NULL: not wanted */, loamx_frontier* out /* NULL: not wanted */,
                             uint64_t capacity, uint64_t* n_frontiers, uint64_t stats[6]);
int loamx_densemap_frontiers_cells(loamx_densemap* h, const loamx_grid_cell* cells, uint32_t nx, uint32_t nz,
                                   const loamx_grid_route_config* route_cfg /* NULL: the defaults */,
                                   const loamx_grid_frontier_config* cfg /* NULL: the defaults */, const uint32_t start_xz[2] /* NULL: no routing */,
                                   uint32_t* labels /* nx * nz; NULL: not wanted */, loamx_frontier* out /* NULL: not wanted */,
                                   uint64_t capacity, uint64_t* n_frontiers, uint64_t stats[6]);
int loamx_frontiers_best(const loamx_frontier* f, uint64_t n, uint32_t min_cost, uint32_t* best);   /* host only, no device */

/* Distance field (optional: a handle that never calls loamx_densemap_dist runs the kernels it ran, allocates what it allocated and
 * exports the same bytes).  "How far is the nearest surface from here, and where is it?": for every cell of a 3-D window of the
 * map the exact squared Euclidean distance, in cells, to the nearest occupied cell of the window, and which cell that is, computed
 * on the device from the table where it lies; then points are looked up in the field where it lies.  Every word is an integer with
 * one value: the field depends on neither the thread schedule, the order of the points, the split into add calls (without a rule)
 * nor the table's size or the number of rehashes.
 *
 * A cell is a cube of k = cell_leaves voxels on a side: voxel (ix, iy, iz) lies in cell (cx, cy, cz) = (floor(ix / k),
 * floor(iy / k), floor(iz / k)) — floor, not truncation: ix = -1, k = 3 gives cx = -1.  The window is the nx * ny * nz cells
 * cx in [x0, x0 + nx), cy in [y0, y0 + ny), cz in [z0, z0 + nz); with (rx, ry, rz) = (cx - x0, cy - y0, cz - z0), cell
 * (cx, cy, cz) is record (rz * ny + ry) * nx + rx.  A voxel qualifies when it lies in the window, holds n >= min_points points
 * and, with a rule, is not dynamic under it (the rule of the carving section, on the voxel's n and miss:
 * loamx_densemap_rule_is_dynamic).  A cell is occupied when it holds at least one qualifying voxel.
 * Per cell, with R = d_max and D = the smallest dx*dx + dy*dy + dz*dz (in cells) to an occupied cell of the window:
 *   d2   = (uint16_t) D when D <= R*R, else (R+1)*(R+1) ("capped"; also when the window has no occupied cell).  An occupied cell
 *          has 0.  Cells outside the window are not obstacles.  With R = 0 this is 0 on occupied cells and 1 elsewhere, with no
 *          special case.
 *   near = (uint32_t) rx' | ry' << 10 | rz' << 20 of an occupied cell at that distance: among the occupied cells of the window with
 *          dx*dx + dy*dy + dz*dz == D, the one with the smallest (rz', ry', rx') in lexicographic order.  An occupied cell names
 *          itself.  LOAMX_DIST_NONE when d2 is capped.
 * The distance is between cells, that is between cell centres: two points in cells D apart (d_a per axis) are at least
 * e * sqrt(sum over the axes of max(|d_a| - 1, 0)^2) apart, e = leaf * k; a body of radius r is clear of every occupied cell when
 * d2 >= (r / e + sqrt(3))^2.
 * loamx_densemap_dist: waits for the adds as download does, runs one memset and three kernels on the map's own stream (mark: one bit
 * per occupied cell; the x and y passes in one; the z pass, which writes d2, near and the counts) and blocks.  The planes wanted
 * come back through pinned memory; with out_d2 and out_near NULL only the four stats words cross.  Either way the field stays on
 * the device for loamx_densemap_dist_query until the next loamx_densemap_dist, loamx_densemap_reset or destroy: it shows the map as
 * it was at the call.  It changes nothing in the map.  The device buffers, 10 1/8 bytes per cell (0.68 GB at 2^26 cells), live in
 * the handle, grow to the largest window asked for and are freed on destroy.  An empty map is valid: every cell is capped.
 * stats: [0] qualifying voxels inside the window, [1] occupied cells, [2] cells with d2 <= R*R, [3] the largest d2 <= R*R, 0 when
 * there is none.
 * LOAMX_E_INVALID, with a message that names the argument, nothing written, the field of an earlier call kept: NULL h or stats;  a
 * configuration that fails loamx_densemap_dist_check;  a rule with den == 0;  a rule on a handle without carving.
 * loamx_densemap_dist_query: per point the two words of its cell.  A point's voxel is the one loamx_densemap_add puts it in,
 * i_a = (int)floorf(p_a * inv) per axis with inv = 1.0f / leaf in f32, under the key rule |floorf(p_a * inv)| < 2^20 on every axis,
 * without the range filter; its cell is the floor division above.  A point that fails the key rule (a NaN or an infinite
 * component fails it) or whose cell lies outside the window gets d2 = LOAMX_DIST_OUTSIDE and near = LOAMX_DIST_NONE.
 * stats: [0] points inside, [1] points outside, [2] inside and capped, [3] inside with d2 < min_d2, [4] (the smallest d2 of a point
 * inside) << 32 | the smallest index of a point with it, UINT64_MAX when no point is inside.  out NULL: the stats alone.  Runs on
 * the map's own stream and blocks; the map and the field are only read.  An empty cloud is LOAMX_OK with zero counts.
 * LOAMX_E_INVALID, nothing written: NULL h, points or stats;  a cloud descriptor that the adds refuse;  no field (no
 * loamx_densemap_dist yet, or a reset since).  LOAMX_E_CAPACITY, nothing written: out given and capacity < points->count.
 *
 * loamx_densemap_dist_check (host only): LOAMX_OK, or LOAMX_E_INVALID with a message that names the first field out of its bounds,
 * in the order cell_leaves, x0, y0, z0, nx, ny, nz, nx * ny * nz, min_points, d_max.
 * loamx_densemap_dist_window (host only): x0, nx, y0, ny, z0, nz of the window about centre[3] with half_extent[3], both in metres,
 * for cfg->cell_leaves; per axis, in double, e = (double)leaf * k, lo = floor(((double)c - (double)h) / e),
 * hi = floor(((double)c + (double)h) / e), first = lo, count = hi - lo + 1.  LOAMX_E_INVALID, cfg unchanged, when an argument is
 * NULL or not finite, leaf <= 0, a half extent < 0 or the result breaks a bound of loamx_densemap_dist_check.
 * loamx_dist_near_unpack (host only): rx = near & 1023, ry = near >> 10 & 1023, rz = near >> 20.  LOAMX_E_INVALID, nothing written,
 * for LOAMX_DIST_NONE, a word with a bit above the three fields, or a NULL pointer.
 * loamx_dist_metres (host only): sqrt((double)d2) * (double)leaf * (double)cell_leaves, the distance between the cell centres. */
#define LOAMX_DIST_NONE 0xFFFFFFFFu
#define LOAMX_DIST_OUTSIDE 0xFFFFFFFFu
typedef struct loamx_densemap_dist_config {
  uint32_t cell_leaves;    /* k, 1..64 (default 2) */
  int32_t  x0, y0, z0;     /* first cell of the window, |x0|, |y0|, |z0| <= 2^21 (default 0, 0, 0) */
  uint32_t nx, ny, nz;     /* 1..1024 each (near packs 10 bits per axis), nx * ny * nz <= 2^26 (default 128, 32, 128) */
  uint32_t min_points;     /* a voxel qualifies when n >= min_points, >= 1 (default 2) */
  uint32_t d_max;          /* R, cells, 0..254: (R+1)^2 = 65025 fits the 16 bits of d2 (default 16) */
} loamx_densemap_dist_config;
typedef struct loamx_dist_sample {   /* 8 bytes */
  uint32_t d2;     /* the cell's d2; LOAMX_DIST_OUTSIDE: the point has no cell in the window */
  uint32_t near;   /* the cell's near; LOAMX_DIST_NONE: capped, or outside */
} loamx_dist_sample;
void loamx_densemap_dist_default_config(loamx_densemap_dist_config* cfg);   /* host only */
int loamx_densemap_dist_check(const loamx_densemap_dist_config* cfg);        /* host only */
int loamx_densemap_dist_window(float leaf, const float centre[3], const float half_extent[3], loamx_densemap_dist_config* cfg);   /* host only */
int loamx_densemap_dist(loamx_densemap* h, const loamx_densemap_dist_config* cfg /* NULL: the defaults */,
                        const loamx_densemap_static_rule* rule /* NULL: every voxel; else needs carving */,
                        uint16_t* out_d2 /* nx * ny * nz; NULL: not wanted */, uint32_t* out_near /* nx * ny * nz; NULL: not wanted */,
                        uint64_t stats[4]);
int loamx_densemap_dist_query(loamx_densemap* h, const loamx_cloud* points, uint32_t min_d2, loamx_dist_sample* out /* NULL: stats only */,
                              uint64_t capacity, uint64_t stats[5]);
int loamx_dist_near_unpack(uint32_t near, uint32_t* rx, uint32_t* ry, uint32_t* rz);   /* host only */
double loamx_dist_metres(uint32_t d2, float leaf, uint32_t cell_leaves);               /* host only */

/* Routing in 3-D over the distance field (optional: a handle that never calls loamx_densemap_route3* runs the kernels it ran and
 * allocates what it allocated; loamx_densemap_dist, loamx_densemap_dist_query, the route calls and the frontier calls return the
 * bytes they returned).  "How does a flying or tall body get there?": the cost-to-go of every cell of a 3-D window towards a set of
 * goal cells, the next step per cell, and routes traced from many starts, computed on the device over the d2 plane of the distance
 * field where it lies; only what is asked for comes back.  The input is integer (d2) and so is the answer: shortest-path costs over
 * integer move costs are a unique fixed point that depends on neither the thread schedule, the number of relaxation rounds nor the
 * rounds per look.
 *
 * Cells, window, record index: those of the distance-field section.  A cell is (rx, ry, rz), window-relative, its record
 * (rz * ny + ry) * nx + rx.  Routing needs nx * ny * nz <= 2^22; the per-axis limits of loamx_densemap_dist_check stay.
 * Weight of a cell, w(c), from its d2 alone (the capped value (d_max + 1)^2 is a number like any other): w = 0 (blocked) when
 * d2 < min_d2; otherwise w = 1 + p, p = floor(soft_weight * (soft_d2 - d2) / soft_d2) when d2 < soft_d2, else 0.  So w is 0, or
 * 1..16.  loamx_route3_weight (host only) is this expression: 0..16, or a negative error for NULL or a configuration that fails its
 * check.  An occupied cell (d2 == 0) is always blocked, because min_d2 >= 1; a min_d2 above every d2 of the window blocks every
 * cell and is still LOAMX_OK.
 * Moves: direction d = 0..25 is (dx, dy, dz), in this order:
 *   axial, d = 0..5: (1,0,0) (-1,0,0) (0,1,0) (0,-1,0) (0,0,1) (0,0,-1);
 *   face diagonals, d = 6..17: (1,1,0) (-1,1,0) (1,-1,0) (-1,-1,0) (1,0,1) (-1,0,1) (1,0,-1) (-1,0,-1) (0,1,1) (0,-1,1) (0,1,-1)
 *   (0,-1,-1);
 *   space diagonals, d = 18 + i, i = 0..7: dx = i & 1 ? -1 : 1, dy = i & 2 ? -1 : 1, dz = i & 4 ? -1 : 1.
 * connectivity 6, 18 or 26 uses the directions d < connectivity: each connectivity is a prefix, and next prefers the straighter
 * move.  loamx_route3_move (host only) is this table.
 * A move a -> b is legal when b lies in the window, w(a) > 0 and w(b) > 0 and no corner is cut: every cell a + (sx, sy, sz) with
 * sx in {0, dx}, sy in {0, dy}, sz in {0, dz} has w > 0, which is two more cells for a face diagonal and six more for a space
 * diagonal.  Its cost is s * (w(a) + w(b)), s = 5, 7, 9 for one, two or three non-zero components: 10 / 14 / 18 on unit weights,
 * symmetric, and in the units of the 2-D field, so that a route that stays in a plane costs what the 2-D route costs.
 * Overflow: a move costs at most 9 * 32 = 288 and a path visits a cell at most once, so cost < 2^22 * 288 < 2^31.
 * Goals: n_goals triples (rx, ry, rz), 1 <= n_goals <= 4096.  A triple outside the window or on a blocked cell is ignored and not
 * counted in stats[2]; a cell named twice counts twice.  With no goal left every cell is unreachable and the call is still LOAMX_OK.
 * Field: one loamx_route_cell per cell (the 8-byte record of the routing section).  cost = the smallest sum of move costs to any
 * used goal, LOAMX_ROUTE_UNREACHABLE for a blocked cell or one with no path.  next = LOAMX_ROUTE3_GOAL when cost == 0,
 * LOAMX_ROUTE3_NONE when unreachable, otherwise the smallest d whose move c -> nb is legal and has cost[nb] + move == cost[c]; it
 * is derived from the final costs in a pass of its own.
 * stats[6]: traversable cells (w > 0);  reachable cells;  goals used;  the largest finite cost (0: none);  relaxation rounds
 * launched;  brick runs that did work (a brick: 8 x 8 x 8 cells).  The first four are part of the definition and exact, the last
 * two describe the schedule.
 *
 * loamx_densemap_route3: runs the distance field of dist_cfg / rule exactly as loamx_densemap_dist does with both planes NULL; that
 * field replaces the standing one and stays for loamx_densemap_dist_query; then routes on its d2 where it lies, with nothing stale.
 * loamx_densemap_route3_last: routes on the distance field that stands; LOAMX_E_INVALID when there is none.
 * loamx_densemap_route3_cells: the same on a d2 plane of the caller's, nx * ny * nz values in record order (an earlier field
 * painted with no-fly zones, or a hand-made one), uploaded to a buffer of the route's own; the standing distance field is neither
 * replaced nor disturbed.
 * loamx_densemap_route3_trace: routes over the field of this handle's last successful route3 call, traced on the device; only the
 * routes come back.  A route is the list of cells from the start, following next, up to and including the goal cell.  lengths[i]
 * is the full number of cells of route i, 0 when the start is outside the window or unreachable.  Of a route longer than capacity
 * only the first capacity triples are written; lengths[i] still holds the full length.  Start i's slice of out_xyz begins at
 * 3 * capacity * i; the words beyond its route are left untouched.
 * loamx_route3_trace (host only): the same walk over a field the caller holds, the same bytes.  It stops with LOAMX_E_INVALID,
 * nothing written, on a field that is not one of ours: a next above 27, a step that leaves the window, a step to a cell whose cost
 * is not strictly smaller (which also bounds the walk by nx * ny * nz steps), a route that ends on a cell that is no goal.
 * loamx_route3_points (host only): the cell centres of a route in metres, LOAM frame: per axis
 * x = (float)(((double)x0 + rx + 0.5) * (double)leaf * k).
 * loamx_densemap_dist_cell_of (host only): the cell of a position: in double, rx = floor((double)x / ((double)leaf * k)) - x0, y
 * and z alike; *inside = 0, r untouched, when the cell is outside the window.
 * Ordering: the route3 calls wait for the adds as loamx_densemap_dist does, run on the map's own stream, change nothing in the map
 * and block until what was asked for is back through pinned memory.  Integer atomics only.  The planes (13 bytes per cell beside
 * the distance field's) live in the handle, are allocated by the first route3 call, grow to the largest window asked for and are
 * freed on destroy.  loamx_densemap_reset drops the route3 field, as it drops the distance field.
 * LOAMX_E_INVALID, with a message that names the argument, nothing written to any output: NULL h, goals_xyz, starts_xyz, lengths,
 * d2, or out_xyz with capacity > 0;  n_goals or n_starts outside 1..4096;  a configuration that fails loamx_route3_check;
 * everything loamx_densemap_dist refuses (but for its stats);  nx * ny * nz > 2^22;  an axis outside 1..1024 in route3_cells;
 * route3_last on a handle that has no distance field;  route3_trace on a handle that has no route3 field (none yet, or a reset
 * since).  LOAMX_E_INTERNAL: the relaxation did not settle within nx * ny * nz + 2 rounds, which the kernel's invariant excludes.
 * loamx_route3_check (host only): names the first field out of its bounds, in the order of the struct. */
#define LOAMX_ROUTE3_GOAL 26u
#define LOAMX_ROUTE3_NONE 27u
typedef struct loamx_route3_config {
  uint32_t connectivity;   /* 6, 18 or 26 (default 26) */
  uint32_t min_d2;         /* smallest d2 of a traversable cell, >= 1 (default 1) */
  uint32_t soft_d2;        /* d2 below which a cell pays a penalty, 0..65025 (default 0) */
  uint32_t soft_weight;    /* largest penalty, 0..15 (default 0) */
} loamx_route3_config;
void loamx_route3_default_config(loamx_route3_config* cfg);   /* host only */
int loamx_route3_check(const loamx_route3_config* cfg);        /* host only */
int loamx_route3_weight(uint32_t d2, const loamx_route3_config* cfg);   /* host only */
int loamx_route3_move(uint32_t d, int32_t dxyz[3]);                     /* host only */
int loamx_densemap_route3(loamx_densemap* h, const loamx_densemap_dist_config* dist_cfg /* NULL: the defaults */,
                          const loamx_densemap_static_rule* rule /* NULL: every voxel; else needs carving */,
                          const loamx_route3_config* cfg /* NULL: the defaults */, const uint32_t* goals_xyz, uint32_t n_goals,
                          loamx_route_cell* out_field /* nx * ny * nz; NULL: not wanted */, uint64_t stats[6] /* NULL: not wanted */);
int loamx_densemap_route3_last(loamx_densemap* h, const loamx_route3_config* cfg /* NULL: the defaults */, const uint32_t* goals_xyz,
                               uint32_t n_goals, loamx_route_cell* out_field /* NULL: not wanted */, uint64_t stats[6] /* NULL: not wanted */);
int loamx_densemap_route3_cells(loamx_densemap* h, const uint16_t* d2 /* nx * ny * nz */, uint32_t nx, uint32_t ny, uint32_t nz,
                                const loamx_route3_config* cfg /* NULL: the defaults */, const uint32_t* goals_xyz, uint32_t n_goals,
                                loamx_route_cell* out_field /* NULL: not wanted */, uint64_t stats[6] /* NULL: not wanted */);
int loamx_densemap_route3_trace(loamx_densemap* h, const uint32_t* starts_xyz, uint32_t n_starts /* 1..4096 */,
                                uint32_t* out_xyz /* n_starts * capacity triples */, uint32_t capacity, uint32_t* lengths /* n_starts */);
int loamx_route3_trace(const loamx_route_cell* field, uint32_t nx, uint32_t ny, uint32_t nz, const uint32_t start[3],
                       uint32_t* out_xyz /* capacity triples */, uint32_t capacity, uint32_t* length);   /* host only */
int loamx_route3_points(const loamx_densemap_dist_config* dist_cfg, float leaf, const uint32_t* route_xyz, uint32_t n,
                        float* out_xyz /* 3 * n */);   /* host only */
int loamx_densemap_dist_cell_of(const loamx_densemap_dist_config* dist_cfg, float leaf, float x, float y, float z, uint32_t r[3],
                                int* inside);   /* host only */

/* Signed distance along the sweep rays, and a triangle mesh of it (optional: a handle that never calls loamx_densemap_tsdf_* or
 * loamx_densemap_mesh runs the kernels it ran, allocates what it allocated and exports the same bytes).  "Where is the surface?":
 * every ray of a sweep adds its signed distance to the cells it crosses near its end, as integers; the zero crossing of the
 * averaged field is extracted on the device as an indexed triangle mesh.  Every stored word is an integer sum: the field depends on
 * neither the thread schedule, the order of the points nor the split into calls (ray_stride counts i per call), and the mesh is one
 * fixed byte string.  All f32 arithmetic below is without fused multiply-add; / and sqrtf are correctly rounded.
 *
 * The field.  A window of nx * ny * nz cells of one voxel each: voxel (ix, iy, iz) with (rx, ry, rz) = (ix - x0, iy - y0, iz - z0)
 * inside [0, nx) x [0, ny) x [0, nz) is record (rz * ny + ry) * nx + rx.  Each cell holds W (uint32_t) and D (int64_t, two's
 * complement).  tau = trunc_leaves * leaf in f32; inv = 1.0f / leaf as the adds have it.
 * loamx_densemap_tsdf_begin: allocates the volume in the handle (12 bytes per cell; it grows to the largest window asked for and is
 * freed on destroy) or clears the one that stands, and clears the statistics.  loamx_densemap_reset drops the field.
 * Integration of point i of a call, p, with the call's origin o:
 *   - i % ray_stride != 0: not traced (stride).
 *   - d = p - o per axis, d2 = (dx*dx + dy*dy) + dz*dz; the insert's range filter with this configuration's min_range and max_range
 *     (d2 >= min_range*min_range, and d2 <= max_range*max_range when max_range > 0) and the key rule |floorf(p_a * inv)| < 2^20 on
 *     every axis; a point that fails either is not traced (filter).
 *   - len = sqrtf(d2); len == 0: dropped (zero length).
 *   - u_a = d_a / len;  back = free_space ? len : fminf(tau, len);  s_a = p_a - u_a * back;  e_a = p_a + u_a * tau.
 *   - the walk is carving's walk (above) from s to e instead of from the origin to the point: per axis so = s_a * inv, sp = e_a * inv,
 *     c = (int)floorf(so), the step sign, rem = |(int)floorf(sp) - c|, tmax and tdelta as there; n_steps = the sum of the three rem.
 *     A ray with n_steps > max_steps, or whose start cell fails the key rule (a NaN fails it), is not traced (steps or key).
 *   - all n_steps + 1 cells k = 0 .. n_steps are visited, both ends included; a visited cell outside the window is skipped.
 *   - a visited cell inside, with indices c and centre m_a = ((float)c_a + 0.5f) * leaf:
 *       sd = ((p_x - m_x) * u_x + (p_y - m_y) * u_y) + (p_z - m_z) * u_z
 *       r  = fminf(fmaxf(sd / tau, -1.f), 1.f)
 *       q  = (int)rintf(r * 1024.0f)                      (ties to even)
 *       W += 1 and D += q, both device atomics.
 * Positive is in front of the surface, toward the sensor.  With free_space = 1 the whole ray is walked and every cell between the
 * sensor and the band receives +1024: what moved away is averaged out by the rays that later pass through it.  Every later step
 * is exact while each cell's W < 2^25: then |D| <= 2^35 and the cross products of the mesh fit a signed 64-bit integer.
 * Sources, the four standard forms: loamx_densemap_tsdf_add (a cloud from the host and its origin), _add_from_map and
 * _add_from_pipeline (the registered cloud where it lies, as loamx_densemap_add_from_*; LOAMX_SKIPPED when there is none) and
 * _add_from_history: the logged calls [first_call, first_call + n_calls) where they lie, in one launch, call k of the window under
 * corrections[12 * k ..] (rebuild's per-call table: rounded to f32 once, the identity rule, the origin corrected by the same
 * expression; NULL: identities).  It needs history (loamx_densemap_enable_history), neither carving nor moments.  None of the
 * four touches the live map, the log or their statistics; the kernels run on the map's own stream behind the source and return
 * without a host wait (the history form waits).  They answer LOAMX_E_INVALID without a field.
 * loamx_densemap_tsdf_download: waits and returns the planes (either pointer may be NULL) and stats since _begin: [0] rays
 * traced, not traced by [1] stride, [2] filter, [3] step count or key, [4] zero length, [5] cells visited inside the window,
 * [6] cells with W > 0, [7] the largest W.  [0] + ... + [4] is the number of points offered.
 * loamx_densemap_tsdf_check (host only): LOAMX_OK, or LOAMX_E_INVALID naming the first field out of its bounds, in the order x0, y0,
 * z0, nx, ny, nz, nx * ny * nz, trunc_leaves, free_space, ray_stride, max_steps, min_range, max_range.
 * loamx_densemap_tsdf_window (host only): x0, nx, ... of the window about centre[3] with half_extent[3] in metres, per axis in
 * double lo = floor(((double)c - (double)h) / (double)leaf), hi = floor(((double)c + (double)h) / (double)leaf), first = lo,
 * count = max(hi - lo + 1, 2).  LOAMX_E_INVALID, cfg unchanged, as loamx_densemap_dist_window.
 *
 * The mesh: marching tetrahedra over the lattice of cell centres.  A cell is valid when W >= min_weight; a valid cell is inside
 * when D < 0 (an integer test: D == 0 is outside).
 * A cube is the 8 cells (x + bx, y + by, z + bz), corner number bx | by << 1 | bz << 2, for every lower cell with rx < nx - 1,
 * ry < ny - 1, rz < nz - 1.  Its six tetrahedra 0..5 follow the axis orders (1,2,4), (1,4,2), (2,1,4), (2,4,1), (4,1,2), (4,2,1):
 * order (a,b,c) has corners t0 = 0, t1 = a, t2 = a|b, t3 = 7 and parity f = 0,1,1,0,0,1 respectively.  A tetrahedron is processed
 * iff its four cells are valid (a cube need not be complete).  Every edge (t_i, t_j), i < j, runs from a cell to one that is larger
 * in each coordinate where they differ: seven directions x, y, xy, z, xz, yz, xyz numbered e = (t_j ^ t_i) - 1; the lower cell owns
 * the edge.
 * Triangles, with k the number of inside corners and E(i,j) the vertex on the edge between t_i and t_j:
 *   k = 0, 4: none.
 *   k = 1, 3: a = the position of the one inside (k = 3: the one outside) corner, o0 < o1 < o2 the other three positions; the
 *             triangle E(a,o0), E(a,o1), E(a,o2), its last two swapped when f + a + [k = 3] is odd.
 *   k = 2:    inside positions a < b, outside c < d; the quad q = E(a,c), E(a,d), E(b,d), E(b,c), reversed (q3, q2, q1, q0) when
 *             f + the number of inversions of the sequence (a,b,c,d) is odd; triangles (q0,q1,q2) and (q0,q2,q3).
 * (v1 - v0) x (v2 - v0) points to the positive side, free space.
 * Vertices: an edge (A, B), A its owner, used by at least one emitted triangle has one vertex.  N = D_A * W_B and
 * M = N - D_B * W_A as exact int64; t = (double)N / (double)M; per axis m_A = ((double)c_A + 0.5) * (double)leaf, m_B likewise,
 * v = (float)(m_A + t * (m_B - m_A)), no fused multiply-add.  axes: 0 LOAM frame (x, y, z), 1 sensor axes (z, x, y).
 * Order: vertices ascend by (owner's record, e); triangles by (cube's lower-cell record, tetrahedron, triangle).  verts: 3 f32
 * per vertex; tris: 3 uint32_t per triangle.
 * loamx_densemap_mesh: behind every tsdf add, four kernels and two scans on the map's own stream; the host reads the two totals to
 * size the buffers and nothing else crosses until the result does.  *n_verts and *n_tris are written even on LOAMX_E_CAPACITY
 * (cap_v < vertices or cap_t < triangles), and nothing else is then.  verts and tris both NULL with zero capacities: the counts
 * and the stats only.  stats: [0] valid cells, [1] inside cells, [2] tetrahedra processed, [3] tetrahedra with an invalid corner
 * and a sign change among their valid corners (holes), [4] vertices, [5] triangles.  An empty field is LOAMX_OK with zero counts.
 * LOAMX_E_INVALID, nothing written: NULL h, n_verts, n_tris or stats; one of verts, tris NULL and not the other; min_weight 0;
 * axes not 0 or 1; no field.
 * loamx_write_ply (host only): binary little-endian PLY, float x y z per vertex and list uchar int vertex_indices per face.
 * loamx_densemap_save_ply: loamx_densemap_mesh, then loamx_write_ply. */
typedef struct loamx_densemap_tsdf_config {
  int32_t  x0, y0, z0;      /* first voxel index of the window, each in [-2^21, 2^21] (default -64) */
  uint32_t nx, ny, nz;      /* 2..1024 each, nx * ny * nz <= 2^26 (default 128) */
  float    trunc_leaves;    /* 1..16: tau = trunc_leaves * leaf (default 3) */
  uint32_t free_space;      /* 0: the band only (default); 1: the whole ray */
  uint32_t ray_stride;      /* >= 1 (default 1) */
  uint32_t max_steps;       /* 1..65536 (default 4096) */
  float    min_range;       /* >= 0 (default 0) */
  float    max_range;       /* 0: none (default), else >= min_range */
} loamx_densemap_tsdf_config;
typedef struct loamx_densemap_mesh_config {
  uint32_t min_weight;      /* >= 1 (default 2) */
  int32_t  axes;            /* 0 or 1 (default 0) */
} loamx_densemap_mesh_config;
void loamx_densemap_tsdf_default_config(loamx_densemap_tsdf_config* cfg);   /* host only */
int loamx_densemap_tsdf_check(const loamx_densemap_tsdf_config* cfg);        /* host only */
int loamx_densemap_tsdf_window(float leaf, const float centre[3], const float half_extent[3], loamx_densemap_tsdf_config* cfg);   /* host only */
int loamx_densemap_tsdf_begin(loamx_densemap* h, const loamx_densemap_tsdf_config* cfg /* NULL: the defaults */);
int loamx_densemap_tsdf_add(loamx_densemap* h, const loamx_cloud* cloud, const float origin[3]);
int loamx_densemap_tsdf_add_from_map(loamx_densemap* h, loamx_map* m);
int loamx_densemap_tsdf_add_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot);
int loamx_densemap_tsdf_add_from_history(loamx_densemap* h, uint64_t first_call, uint64_t n_calls,
                                         const double* corrections /* 12 * n_calls; NULL: identities */);
int loamx_densemap_tsdf_download(loamx_densemap* h, uint32_t* out_w /* nx * ny * nz; NULL: not wanted */,
                                 int64_t* out_d /* nx * ny * nz; NULL: not wanted */, uint64_t stats[8]);
void loamx_densemap_mesh_default_config(loamx_densemap_mesh_config* cfg);   /* host only */
int loamx_densemap_mesh(loamx_densemap* h, const loamx_densemap_mesh_config* cfg /* NULL: the defaults */, float* verts, uint64_t cap_v,
                        uint32_t* tris, uint64_t cap_t, uint64_t* n_verts, uint64_t* n_tris, uint64_t stats[6]);
int loamx_write_ply(const char* path, const float* verts, uint64_t n_verts, const uint32_t* tris, uint64_t n_tris);   /* host only */
int loamx_densemap_save_ply(loamx_densemap* h, const loamx_densemap_mesh_config* cfg /* NULL: the defaults */, const char* path,
                            uint64_t stats[6]);

/* Objects: connected components of the voxel map (optional: a handle that never segments runs the kernels it ran and allocates what
 * it allocated).  "Which voxels belong together?": on the voxel lattice, Euclidean clustering with a tolerance of one leaf is
 * connected-component labelling of the selected voxels, done on the device where the table lies; a component list and one word
 * per voxel come back.  Every output word depends only on the set of selected voxels: not on the thread schedule, the table's
 * size, the number of rehashes or the order of the adds.
 *
 * Selection: a voxel (ix, iy, iz) with n points is selected iff n >= min_points, lo[a] <= i_a <= hi[a] on every axis, and it
 * passes `which`: ALL every such voxel; STATIC those the rule does not call dynamic; DYNAMIC those it does (the expression of
 * loamx_densemap_rule_is_dynamic on the voxel's n and miss).
 * Adjacency: two selected voxels are adjacent iff their index vectors differ by a non-zero d with every |d_a| <= 1 and
 * |d_x| + |d_y| + |d_z| <= 1 (connectivity 6: a shared face), <= 2 (18: a face or an edge), <= 3 (26: a face, an edge or a
 * corner).  It is decided on the indices, not on the packed key: a neighbour with any |i_a| >= 2^20 does not exist and is not
 * looked up, so nothing joins across the edge of the key range.  A voxel that is not selected (outside the window, say) connects
 * nothing.
 * Components: the classes of the transitive closure of adjacency.  A component is kept iff it has at least min_voxels voxels;
 * the kept ones are numbered 0 .. C-1 in ascending min_key, the smallest voxel key in them (key = (ix + 2^20) | (iy + 2^20) << 21
 * | (iz + 2^20) << 42), and segs[c] is component c: its min_key, the number of its voxels, the sum of their n, its inclusive
 * bounding box in voxel indices and the sum of the indices per axis, all exact integers.
 * Labels: labels[j] belongs to voxel j in the record order of loamx_densemap_download (ascending key): the number of its
 * component, LOAMX_SEGMENT_NONE when the voxel is not selected or its component was dropped.  *n_voxels is the map's voxel count
 * (the length of labels), *n_segs is C.
 * stats[6]: voxels selected;  components before min_voxels;  components kept;  voxels in kept components;  voxels of the largest
 * component (before min_voxels; 0: none);  hook attempts that lost to another thread.  The first five are part of the definition
 * and exact, the last describes the schedule.
 * loamx_segment_box (host only): metres, LOAM frame: lo_m[a] = (float)((double)lo[a] * (double)leaf), hi_m[a] =
 * (float)((double)(hi[a] + 1) * (double)leaf), centre[a] = (float)(((double)sum_idx[a] / (double)voxels + 0.5) * (double)leaf):
 * the mean of the voxel centres.  LOAMX_E_INVALID for a NULL argument or voxels == 0.
 * Ordering: as loamx_densemap_raycast the call waits for every add, runs on the map's own stream and blocks until the outputs are
 * back through pinned memory.  The map is only read: every export is byte for byte what it was before the call.  Integer
 * atomics only.  The work arrays live in the handle, are allocated by the first call, sized by the table's slots, grown when the
 * table has grown and freed on destroy.  labels and segs may each be NULL: that output is skipped (and, without labels, the
 * voxels' keys do not cross to the host).  An empty map is LOAMX_OK with every count zero and nothing launched beyond the read
 * of the map's counters.
 * LOAMX_E_INVALID, with a message that names the argument, nothing written to any output and the handle as it was: NULL h,
 * n_voxels, n_segs or stats;  a configuration that fails loamx_densemap_segment_check (which > 2;  connectivity not 6, 18 or 26;
 * min_points or min_voxels 0;  lo[a] > hi[a];  a bound outside +-(2^20 - 1));  which != ALL on a handle without carving;  a rule
 * whose den is 0 (the rule is read only when which != ALL).
 * LOAMX_E_CAPACITY: labels given and label_capacity < the map's voxels, or segs given and seg_capacity < C.  Nothing is written
 * to labels, segs or stats; *n_voxels and *n_segs hold the needed counts. */
#define LOAMX_SEGMENT_NONE 0xFFFFFFFFu
#define LOAMX_SEGMENT_ALL 0u      /* every voxel that passes min_points and the window */
#define LOAMX_SEGMENT_STATIC 1u   /* ... and is not dynamic under the rule (needs carving) */
#define LOAMX_SEGMENT_DYNAMIC 2u  /* ... and is dynamic under the rule (needs carving) */
typedef struct loamx_densemap_segment_config {
  uint32_t which;          /* LOAMX_SEGMENT_ALL / _STATIC / _DYNAMIC (default ALL) */
  uint32_t connectivity;   /* 6, 18 or 26 (default 26) */
  uint32_t min_points;     /* a voxel with fewer points is not selected, >= 1 (default 1) */
  uint32_t min_voxels;     /* components with fewer voxels are dropped, >= 1 (default 1) */
  int32_t lo[3], hi[3];    /* inclusive window in voxel indices (ix, iy, iz); default -(2^20 - 1) .. 2^20 - 1: everything */
} loamx_densemap_segment_config;
typedef struct loamx_segment {   /* 72 bytes */
  uint64_t min_key;        /* smallest voxel key of the component: its identity */
  uint64_t voxels;         /* voxels in it */
  uint64_t points;         /* sum of their n */
  int32_t lo[3], hi[3];    /* inclusive bounding box in voxel indices */
  int64_t sum_idx[3];      /* sum of the voxel indices per axis (the centroid's numerator) */
} loamx_segment;
void loamx_densemap_segment_default_config(loamx_densemap_segment_config* cfg);   /* host only */
int loamx_densemap_segment_check(const loamx_densemap_segment_config* cfg);       /* host only */
int loamx_densemap_segment(loamx_densemap* h, const loamx_densemap_segment_config* cfg /* NULL: the defaults */,
                           const loamx_densemap_static_rule* rule /* NULL: the default rule; read only when which != ALL */,
                           uint32_t* labels /* NULL: not wanted */, uint64_t label_capacity, uint64_t* n_voxels,
                           loamx_segment* segs /* NULL: not wanted */, uint64_t seg_capacity, uint64_t* n_segs, uint64_t stats[6]);
int loamx_segment_box(const loamx_segment* s, float leaf, float lo_m[3], float hi_m[3], float centre[3]);   /* host only */

/* Objects of a sweep that is not in the map (optional, as above).  "What stands in this sweep that the map does not know?": the
 * points of a cloud are tested against the live map, the ones that pass are clustered on the voxel lattice of the map, and every
 * point gets the number of its object.  The map is only read, and nothing of the cloud stays in the handle.  Every output word but
 * stats[12] depends only on the multiset of points and on the words of the map: not on the thread schedule, the size of either
 * table or the order of the adds.
 *
 * The cloud and origin are in the map frame, exactly as loamx_densemap_add takes them.
 * Admission: point i is admitted iff loamx_densemap_add on this handle would add it: the same range filter about origin (the
 * handle's min_range / max_range) and the same key rule (every |floor(c * (1 / leaf))| < 2^20; NaN and infinities fail), by the
 * same f32 expressions.  The cell c of an admitted point is the cell add would put it in.
 * Mapped: a voxel of the map is mapped iff it is in the live table, holds n >= map_min_points and, when a rule is given, is not
 * dynamic under it (the expression of loamx_densemap_rule_is_dynamic on its n and miss).
 * Near: an admitted point is near iff some cell c' with max_a |c'_a - c_a| <= margin is mapped.  It is decided on the indices:
 * a cell with any |i_a| >= 2^20 does not exist and is not looked up.
 * Selection by `which`: LOAMX_CLOUD_ALL enters every admitted point (no lookup); _NEW the admitted points that are not near;
 * _KNOWN those that are.  The entered points go into a scratch table of the map's own format (the same key, the same fixed-point
 * sums n, Sx, Sy, Sz): its words are those of a fresh handle of this configuration fed with exactly the entered points.
 * Clustering: the voxels of the scratch table are grouped exactly as loamx_densemap_segment with which = LOAMX_SEGMENT_ALL groups
 * a map's: the same connectivity, min_points (of entered points in a voxel OF THE CLOUD), window, min_voxels and record struct;
 * the kept components are numbered in ascending min_key.
 * Outputs: segs: the kept components, byte for byte what loamx_densemap_segment returns for that fresh handle.  labels[i], in
 * point order: the number of the component of point i's voxel, LOAMX_SEGMENT_NONE when the point did not enter, its voxel was not
 * selected or its component was dropped.  *n_points is the cloud's count (the length of labels), *n_segs the kept components.
 * stats[13]: [0] points offered;  [1] dropped by range;  [2] dropped by the key rule;  [3] admitted but rejected by the map
 * test;  [4] entered ([0] = [1] + [2] + [3] + [4]);  [5] voxels of the scratch table;  [6] selected voxels;  [7] components
 * before min_voxels;  [8] components kept;  [9] voxels in kept components;  [10] voxels of the largest component;  [11] points
 * with a label other than NONE;  [12] hook attempts that lost to another thread.  [0..11] are part of the definition and exact,
 * [12] describes the schedule.
 * The from_map / from_pipeline forms take the registered cloud of m's last process() / of the slot-th stream of p's last step
 * where it lies on the device, about that sweep's origin, as loamx_densemap_raycast_from_map does; LOAMX_SKIPPED, nothing
 * written, when that call produced no registered cloud.
 * Ordering: as loamx_densemap_raycast and loamx_densemap_segment the call waits for every add, runs on the map's own stream, only
 * reads the live table and blocks until the outputs are back through pinned memory; every export of the map is byte for byte what
 * it was before.  Integer atomics only.  The scratch table (a power of two of at least twice the cloud's count, at least 1024
 * slots), one key and one id word per point and the staging blocks live in the handle, are allocated by the first call, grow to
 * the largest cloud and are freed on destroy; loamx_densemap_segment's work arrays are shared.  labels and segs may each be NULL:
 * that output is skipped (without labels the second kernel does not run).  Outputs are written last, all or none.  An empty
 * cloud is LOAMX_OK with every count zero and nothing launched; an empty map is valid: nothing is near.  Any `which` works on a
 * handle without carving when rule is NULL.
 * LOAMX_E_INVALID, with a message that names the argument, nothing written: NULL h, points (m, p), origin, n_points, n_segs or
 * stats;  a configuration that fails loamx_densemap_segment_cloud_check (which > 2;  margin > 2;  map_min_points 0;
 * connectivity not 6, 18 or 26;  min_points or min_voxels 0;  lo[a] > hi[a];  a bound outside +-(2^20 - 1));  a rule whose den
 * is 0;  a rule on a handle without carving;  a source on another device;  a cloud of more than 2^30 points.
 * LOAMX_E_CAPACITY: labels given and label_capacity < the cloud's count, or segs given and seg_capacity < the kept components.
 * Only *n_points and *n_segs are written: they hold the needed counts.
 *
 * loamx_segments_match (host only, no device): following objects from call to call.  For each cur[j] the prev[i] whose inclusive
 * box, grown by gap voxels on every side, shares the most cells with cur[j]'s box: per axis max(0, min(prev.hi + gap, cur.hi) -
 * max(prev.lo - gap, cur.lo) + 1), the product of the three taken exactly (128 bits); ties go to the smaller min_key;
 * prev_of_cur[j] = that i, LOAMX_SEGMENT_NONE when no box overlaps.  gap in 0..1024, n_prev < 2^32 - 1.  Nothing else of
 * tracking is built: no motion model, no ids kept in the library. */
#define LOAMX_CLOUD_ALL 0u     /* every admitted point */
#define LOAMX_CLOUD_NEW 1u     /* admitted points with no mapped voxel within `margin` */
#define LOAMX_CLOUD_KNOWN 2u   /* admitted points with one */
typedef struct loamx_densemap_segment_cloud_config {
  uint32_t which;            /* LOAMX_CLOUD_ALL / _NEW / _KNOWN (default NEW) */
  uint32_t margin;           /* 0, 1 or 2: Chebyshev radius, in voxels, of the neighbourhood looked up in the map (default 1) */
  uint32_t map_min_points;   /* a map voxel counts as mapped with n >= this, >= 1 (default 1) */
  uint32_t connectivity;     /* 6, 18 or 26 (default 26) */
  uint32_t min_points;       /* a voxel OF THE CLOUD is selected with >= this many entered points, >= 1 (default 1) */
  uint32_t min_voxels;       /* components with fewer voxels are dropped, >= 1 (default 1) */
  int32_t lo[3], hi[3];      /* inclusive window in voxel indices (ix, iy, iz); default -(2^20 - 1) .. 2^20 - 1: everything */
} loamx_densemap_segment_cloud_config;
void loamx_densemap_segment_cloud_default_config(loamx_densemap_segment_cloud_config* cfg);   /* host only */
int loamx_densemap_segment_cloud_check(const loamx_densemap_segment_cloud_config* cfg);       /* host only; names the first bad field */
int loamx_densemap_segment_cloud(loamx_densemap* h, const loamx_cloud* points, const float origin[3],
                                 const loamx_densemap_segment_cloud_config* cfg /* NULL: the defaults */,
                                 const loamx_densemap_static_rule* rule /* NULL: every voxel; else needs carving */,
                                 uint32_t* labels /* NULL: not wanted */, uint64_t label_capacity, uint64_t* n_points,
                                 loamx_segment* segs /* NULL: not wanted */, uint64_t seg_capacity, uint64_t* n_segs, uint64_t stats[13]);
int loamx_densemap_segment_cloud_from_map(loamx_densemap* h, loamx_map* m, const loamx_densemap_segment_cloud_config* cfg,
                                          const loamx_densemap_static_rule* rule, uint32_t* labels, uint64_t label_capacity,
                                          uint64_t* n_points, loamx_segment* segs, uint64_t seg_capacity, uint64_t* n_segs,
                                          uint64_t stats[13]);
int loamx_densemap_segment_cloud_from_pipeline(loamx_densemap* h, loamx_pipeline* p, uint32_t slot,
                                               const loamx_densemap_segment_cloud_config* cfg, const loamx_densemap_static_rule* rule,
                                               uint32_t* labels, uint64_t label_capacity, uint64_t* n_points, loamx_segment* segs,
                                               uint64_t seg_capacity, uint64_t* n_segs, uint64_t stats[13]);
int loamx_segments_match(const loamx_segment* prev, uint64_t n_prev, const loamx_segment* cur, uint64_t n_cur,
                         uint32_t gap /* voxels, 0..1024 */, uint32_t* prev_of_cur /* n_cur words */);   /* host only */

/* Regions, eviction to tile files and paging (optional: a handle that never calls them runs the kernels it ran and exports the same
 * bytes).  A map of a whole run cannot stay in device memory; these calls hand out a part of the map by place, take a part of it out
 * into a file, and keep the map around a moving centre with the rest in a directory of tile files.  Every word of a voxel is an
 * integer sum and loamx_densemap_merge_file adds a file into a live table word for word, so whatever is taken out into a file and
 * merged back restores the map bit for bit.
 *
 * Region: an inclusive window of voxel indices (ix, iy, iz), as in loamx_densemap_segment_config, and a side.  INSIDE selects the
 * voxels with lo[a] <= i_a <= hi[a] on every axis, OUTSIDE the others.  loamx_densemap_region_check: LOAMX_E_INVALID with a message
 * that names the field for lo[a] > hi[a], a bound outside +-(2^20 - 1), side > 1, reserved != 0; every call below runs it first.
 * Host-only helpers, no device:
 *   region_default   everything, INSIDE.
 *   region_about     the window of the box centre +- half (LOAM frame, metres): in double, lo_a = floor((c_a - h_a) / leaf) and
 *                    hi_a = floor((c_a + h_a) / leaf), both clamped to +-(2^20 - 1).  LOAMX_E_INVALID: a non-finite input, a negative
 *                    half extent, a leaf that create refuses.
 *   tile_of          tile_a = floor(i_a / T), rounded towards minus infinity (index -1 lies in tile -1); T = tile_voxels in [1, 2^20].
 *   tile_region      INSIDE, lo = tile * T, hi = tile * T + T - 1, clamped to +-(2^20 - 1); a tile that holds no index of that range:
 *                    LOAMX_E_INVALID.
 *   tile_name        "tile_<tx>_<ty>_<tz>.lxdm", signed decimal, with its NUL into buf (cap too small: LOAMX_E_INVALID).
 *
 * Reading a region.  count_region: counts[0] = the selected voxels, counts[1] = the sum of their n.  download_region: the records
 * of loamx_densemap_download for the selected voxels only, in ascending key order; out->count is the capacity on the way in and the
 * count on the way out (LOAMX_E_CAPACITY: out->count = the needed count, nothing else written).  save_region: an 'LXDM' version 1 file
 * of the selected voxels by the writer of loamx_densemap_save (temporary name, rename); flags, leaf and the carving configuration are
 * the handle's, `offered` is the sum of n of the file's voxels, and dropped by range, dropped by key and the six carve statistics are
 * 0.  load, merge_file and file_info(deep) accept it as it is.  All three wait for the adds as download does, run on the map's own
 * stream and only read the map: one pass over the keys selects, and only the selected records cross to the host.
 *
 * loamx_densemap_evict(h, region, path, removed): the selected voxels leave the map, into the file of save_region when path is not
 * NULL, discarded when it is.  removed[0] = voxels, removed[1] = points (the sum of their n).  Order: the adds are waited for and the
 * selected voxels counted; the new table is allocated, the smallest power of two of slots that is >= initial_slots and >= 2 x the
 * voxels that stay (the table SHRINKS: bounded memory is the point; prune keeps its size); with a path the file is written; the
 * voxels that are not selected are rehashed into the new table with every word they hold (n, S*, miss, stamp, moments); the table is
 * replaced.  A failed allocation or a failed write leaves the map, its statistics and the directory as they were, with no file and
 * no .part file: the allocation comes before the file, so no file can exist for voxels the map still holds.
 * Statistics: `offered` decreases by removed[1]; the two drop counts and the carve statistics stay.  So evict(region, path) followed
 * by merge_file(path) restores get_stats (but for slots), get_carve_stats and every export, loamx_densemap_save included, bit for bit.
 * With a cap, an add refused before an evict is admitted after it.  The frozen snapshot and the coarse levels are not touched, as
 * with prune.  A handle with history may evict; as with prune, a rebuild brings the voxels back from the log.
 *
 * loamx_densemap_file_merge(path_a, path_b, path_out) (host only, no device): the records of two files added per key as
 * loamx_densemap_merge defines it (n, S* and the moments modulo 2^64, miss modulo 2^32, header statistics summed; the carving
 * configuration is a's).  Both files get the deep check; the bits of the leaf and the flags must be equal (LOAMX_E_INVALID names
 * the field).  The output is written under a temporary name and renamed; path_out may equal path_a.
 *
 * loamx_densemap_page(h, cfg, centre, stats): the map stays resident around `centre` (LOAM frame, metres), the rest lives in
 * cfg->dir as one file per tile of tile_voxels^3 voxels, named by tile_name.  The centre tile is tile_of(floor(centre / leaf))
 * (in double, clamped); the keep box is the tiles within radius[a] of it on axis a.
 *   Page in: every tile of the keep box that has a file in dir is merged with merge_file, in ascending (tz, ty, tx), and the file is
 *   unlinked once its merge succeeded.  LOAMX_E_CAPACITY from merge_file ends the call with that status: the tiles not yet merged
 *   stay on disk, and nothing is paged out.
 *   Page out: one evict of OUTSIDE the keep box brings the records down once; the host buckets them by tile; a tile that has a file
 *   already is merged into it on the host (far returns land in tiles that were paged out earlier).  Every tile file of the call is
 *   first written as .part, then all are renamed, and only then is the table rehashed.  A failed write removes the .part files and
 *   leaves the map and the directory unchanged.  Nothing to page out: the table stays as it is.
 *   stats: [0] tiles paged in, [1] voxels merged in, [2] tile files written, [3] voxels paged out, [4] tile files that were merged
 *   with an existing one, [5] resident voxels afterwards.
 * Invariant: at every return, the map of the whole run is the resident map plus every tile file, summed as merge sums.
 * Known limits: with carving, rays do not count misses on voxels that are not resident.  page is not safe against the process dying
 * between the renames and the rehash (the voxels are then in the files AND in the map).  A handle with history cannot page in,
 * because merge_file refuses it. */
#define LOAMX_REGION_INSIDE 0u
#define LOAMX_REGION_OUTSIDE 1u
typedef struct loamx_densemap_region {
  int32_t lo[3], hi[3];   /* inclusive window in voxel indices (ix, iy, iz), as in loamx_densemap_segment_config */
  uint32_t side;          /* INSIDE: lo[a] <= i_a <= hi[a] on every axis; OUTSIDE: the negation */
  uint32_t reserved;      /* 0 */
} loamx_densemap_region;
typedef struct loamx_densemap_page_config {
  const char* dir;        /* the tile directory; it must exist */
  uint32_t tile_voxels;   /* T: voxels per tile edge, in [1, 2^20] */
  uint32_t radius[3];     /* tiles kept on either side of the centre tile, per axis */
} loamx_densemap_page_config;
void loamx_densemap_region_default(loamx_densemap_region* region);                                                /* host only */
int loamx_densemap_region_check(const loamx_densemap_region* region);                                             /* host only */
int loamx_densemap_region_about(float leaf, const float centre[3], const float half[3], loamx_densemap_region* region);   /* host only */
int loamx_densemap_tile_of(const int32_t idx[3], uint32_t tile_voxels, int32_t tile[3]);                          /* host only */
int loamx_densemap_tile_region(const int32_t tile[3], uint32_t tile_voxels, loamx_densemap_region* region);       /* host only */
int loamx_densemap_tile_name(const int32_t tile[3], char* buf, uint64_t cap);                                     /* host only */
int loamx_densemap_file_merge(const char* path_a, const char* path_b, const char* path_out);                      /* host only */
int loamx_densemap_count_region(loamx_densemap* h, const loamx_densemap_region* region, uint64_t counts[2]);
int loamx_densemap_download_region(loamx_densemap* h, const loamx_densemap_region* region, loamx_cloud* out, int axes);
int loamx_densemap_save_region(loamx_densemap* h, const loamx_densemap_region* region, const char* path);
int loamx_densemap_evict(loamx_densemap* h, const loamx_densemap_region* region, const char* path /* NULL: discard */,
                         uint64_t removed[2]);
int loamx_densemap_page(loamx_densemap* h, const loamx_densemap_page_config* cfg, const float centre[3], uint64_t stats[6]);

/* ------------------------------------------------------------------------------------------------------------
 * Place recognition (not in the reference): a database of rotation-invariant sweep descriptors in device memory (Scan Context: a
 * ring x sector polar grid of maximum heights around the sensor) and an exhaustive search for the earlier entries that look like a
 * query, with the yaw between the two.  Detection only: a match becomes a constraint in loamx_densemap_align_many and an edge of
 * loamx_posegraph (below).
 *
 * Descriptor of a cloud about an origin o (LOAM frame: x left, y up, z forward), everything per point in f32, no fused multiply-add:
 *   d = p - o per component;  a = d.z, b = d.x;  r2 = a*a + b*b;  h = d.y + height_offset.
 *   The point is used when x, y, z are finite, r2 >= min_range^2, r2 < max_range^2 (the squares in f32) and h > 0.
 *   ring   i = min((int)(sqrtf(r2) * ring_scale), R - 1),  ring_scale = (float)R / max_range  (sqrtf and / correctly rounded).
 *   sector: S boundary directions (c_k, s_k) = ((float)cos(2 pi k / S), (float)sin(2 pi k / S)), cos / sin evaluated in double on the
 *          host (loamx_place_sector_table returns them);  cross(k) = c_k*b - s_k*a.  The sector is the smallest k with cross(k) >= 0
 *          and cross((k + 1) mod S) < 0: the angle from +z towards +x lies in [2 pi k / S, 2 pi (k + 1) / S).  A point for which no k
 *          qualifies (a = b = 0) is dropped.  No atan2 enters the definition.
 *   cell   D[i][k] = the maximum h over its points, 0 when empty — a maximum does not depend on the order of the points, so an entry, and
 *          every byte derived from it, does not depend on the thread schedule.
 *   ring key  rk[i] = (D[i][0] + D[i][1] + ... in ascending k, one f32 addition at a time) / (float)S.
 * Distance of a query Q and a stored C at shift s (0 <= s < S): nq[j] = sqrtf(sum_i Q[i][j]^2), nc alike (i ascending, each product
 * rounded, then added);  dot(j, s) = sum_i Q[i][j] * C[i][(j + s) mod S] likewise;  the terms dot(j, s) / (nq[j] * nc[(j + s) mod S])
 * are summed over the columns j, ascending, where both norms are > 0;  d(s) = 1 - sum / (float)count, and 1 when count is 0.  The
 * distance of the pair is the smallest d(s), ties to the smaller s, and `shift` is that s:  Q[i][j] ~ C[i][(j + shift) mod S].
 * Yaw convention: yaw_hint = shift * 2 pi / S is the yaw (rot_y of the pose convention above, mod 2 pi) of the query's frame relative
 * to the stored entry's frame.  For sensor-frame clouds that is the heading of the revisit relative to the first visit; the clouds of
 * add_from_map / add_from_pipeline are in the map frame — levelled and headed by the pose estimate — so there it is the yaw DRIFT
 * between the two visits.
 * Search for a query with id q (a query that is not stored: q = the number of entries): the candidates are the entries with
 * id + exclude_recent < q.  With n_candidates K > 0 and more than K candidates they are first cut to the K smallest by
 * (sum_i (rk_q[i] - rk_c[i])^2 in ascending i, id); with K = 0 every candidate is compared.  Result: the n_results best by
 * (distance, id) ascending.
 * Ordering: an add from a mapper or a pipeline is enqueued on that handle's own stream behind the kernel that wrote the registered
 * cloud and does not block the caller; ids are the running count of entries.  Queries, get_descriptor and save wait for every add.
 * The table of entries doubles on its own, on the device.  A source on another device than the database: LOAMX_E_INVALID.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct loamx_place loamx_place;
typedef struct loamx_place_config {
  int n_rings;              /* R, 1..64 (default 20) */
  int n_sectors;            /* S, 4..128 (default 60) */
  float max_range;          /* > 0 (default 80 m) */
  float min_range;          /* >= 0, < max_range (default 0) */
  float height_offset;      /* the sensor's height above the ground, so that heights are positive (default 2.0 m) */
  int n_candidates;         /* K: 0 = exhaustive search (default); 1..256 = ring-key pre-selection */
  uint32_t exclude_recent;  /* loamx_place_query_entry: entries this close in id to the query are not candidates (default 50) */
  uint32_t max_entries;     /* cap on stored entries; 0 = bounded by device memory only */
  uint32_t initial_entries; /* room at creation, a power of two (default 1024) */
  int device;
} loamx_place_config;
typedef struct loamx_place_match {
  uint32_t id;
  uint32_t shift;            /* yaw_hint = shift * 2 pi / n_sectors */
  float distance;
  float ring_key_distance;
} loamx_place_match;
#define LOAMX_PLACE_MAX_RESULTS 64

void loamx_place_default_config(loamx_place_config* cfg);            /* host only, no device needed */
loamx_place* loamx_place_create(const loamx_place_config* cfg);
void loamx_place_destroy(loamx_place* h);
int loamx_place_reset(loamx_place* h);
uint32_t loamx_place_size(loamx_place* h);                           /* entries, those still in flight included; no wait */
/* host only: table[2k] = c_k, table[2k + 1] = s_k for k < n_sectors */
int loamx_place_sector_table(int n_sectors, float* table);
/* a cloud from the host, described about origin[3]; *id (may be NULL) = the new entry.  LOAMX_E_CAPACITY, database unchanged, when
 * max_entries would be passed */
int loamx_place_add(loamx_place* h, const loamx_cloud* points, const float origin[3], uint32_t* id);
/* the registered full-resolution cloud of m's last process() / process_linked() where it lies, origin = that sweep's transformAftMapped
 * translation; LOAMX_SKIPPED, and no entry, when that call produced no registered cloud */
int loamx_place_add_from_map(loamx_place* h, loamx_map* m, uint32_t* id);
/* the registered cloud of the slot-th stream registered in p's last step (the slot of loamx_pipeline_download_full_res); LOAMX_SKIPPED
 * when the last step registered nothing */
int loamx_place_add_from_pipeline(loamx_place* h, loamx_pipeline* p, uint32_t slot, uint32_t* id);
/* the n_results (<= LOAMX_PLACE_MAX_RESULTS) best earlier entries for the stored entry `id` (the configuration's exclude_recent), and
 * for a cloud that is not stored (exclude_recent as passed; 0 = every entry); *n_found = records written */
int loamx_place_query_entry(loamx_place* h, uint32_t id, loamx_place_match* matches, uint32_t n_results, uint32_t* n_found);
int loamx_place_query(loamx_place* h, const loamx_cloud* points, const float origin[3], uint32_t exclude_recent, loamx_place_match* matches,
                      uint32_t n_results, uint32_t* n_found);
/* entry id: desc[R * S] (ring-major) and ring_key[R]; either may be NULL */
int loamx_place_get_descriptor(loamx_place* h, uint32_t id, float* desc, float* ring_key);
/* the database as a file ('LXPL', version, R, S, the three f32 parameters, the count; then the descriptors and the ring keys), so that a
 * map snapshot can travel with its keyframes.  load replaces the entries of a handle whose R, S, ranges and height_offset equal the
 * file's (LOAMX_E_INVALID otherwise, handle unchanged); the loaded handle answers every query with the same bytes */
int loamx_place_save(loamx_place* h, const char* path);
int loamx_place_load(loamx_place* h, const char* path);

/* Views described from a dense map (optional: a handle that never calls these runs the kernels it ran, allocates what it allocated and
 * answers with the same bytes).  "Where am I in a loaded map?": a map that arrived by loamx_densemap_load or merge_file has no sweeps
 * and therefore no place entries.  loamx_place_add_views describes the map from many virtual view points in one call, on the device:
 * no ray, hit or voxel crosses to the host and no launch is spent per view point.  The chain is load -> loamx_densemap_grid ->
 * loamx_grid_view_origins -> loamx_place_add_views -> loamx_place_query (the live sweep) -> loamx_place_view_pose ->
 * loamx_densemap_align_many / align_pyramid.
 *
 * A view is a virtual sensor at an origin o in the map frame (LOAM axes).  Its entry is what loamx_place_add would store for a cloud
 * V(o) described about o with the database's own R, S, ranges and height_offset: the same f32 arithmetic, the same sector table, the
 * same ring key.  Two modes define V(o):
 *   LOAMX_PLACE_VIEW_CAST (default): the caller gives n_rays offsets off[j] (f32 triples).  Ray j runs from o to end_j = o + off[j],
 *     one f32 addition per component, and is cast exactly as loamx_densemap_raycast casts it: that section's walk, max_steps,
 *     skip_steps, min_points, the optional rule, the end cell included.  V(o) is the positions x, y, z of the records with status HIT
 *     or HIT_END (the bytes of loamx_ray_hit).  View o is loamx_densemap_raycast(ends, o) followed by loamx_place_add(hit positions,
 *     o), byte for byte.  Several rays that hit the same voxel change nothing: a cell is a maximum.
 *   LOAMX_PLACE_VIEW_VOXELS: V(o) is the exported positions (loamx_densemap_download, axes 0) of every voxel with n >= min_points that
 *     the rule, if given, does not call dynamic: the map seen through walls.  A cheaper index for open terrain and a baseline for the
 *     other mode.  offsets must be NULL and n_rays 0.
 * An entry depends on the map's words, o, the offsets and the configuration alone: not on the order of origins or rays, on how the
 * origins are split into calls, on the table's size or on the thread schedule.  Views are ordinary entries afterwards: query,
 * query_entry, get_descriptor, save and load treat them as such.  Entry *first_id + i belongs to origins[3 i ..].
 * stats: [0] entries added;  [1..5] the five counts of loamx_densemap_raycast (NOT_TRACED, MISS, HIT, HIT_END, cells looked up) summed
 * over all views, integer sums;  in VOXELS mode [1] is the number of qualifying voxels and [2..5] are 0.
 * Ordering: the call waits for the map's adds as download does, runs on the map's own stream behind every place add enqueued so far
 * and blocks until the entries stand.  The table of entries grows in one step to the power of two that holds them.  An empty map is
 * valid: n all-zero entries.  A probe overflow is reported by the map's next reading call, as for a ray cast.
 * LOAMX_E_INVALID, with a message that names the argument, both handles unchanged: NULL pl, dm or origins;  a mode other than the
 * two;  n outside 1..LOAMX_PLACE_VIEW_MAX_ORIGINS;  in CAST mode NULL offsets, n_rays outside 1..LOAMX_PLACE_VIEW_MAX_RAYS or
 * max_steps outside 1..65536;  in VOXELS mode offsets given or n_rays != 0;  min_points == 0;  a rule with den == 0 or on a map
 * without carving;  an origin or offset that is not finite;  handles on different devices.  LOAMX_E_CAPACITY, nothing added: max_entries
 * would be passed.
 *
 * loamx_place_view_rays (host only): the offsets of a lidar of n_elevations rings with n_azimuth rays each, ray (e, a) at index
 * e * n_azimuth + a: in double, az = 2 pi a / n_azimuth, el = (double)elevations[e] (radians), offset = ((float)(range * cos el *
 * sin az), (float)(range * sin el), (float)(range * cos el * cos az)), the products from left to right: azimuth runs from +z towards
 * +x, as the sectors do.  LOAMX_E_INVALID: NULL elevations or offsets;  n_azimuth or n_elevations 0;  their product above
 * LOAMX_PLACE_VIEW_MAX_RAYS;  range not finite or not positive;  an elevation that is not finite.
 * loamx_grid_view_origins (host only): where a vehicle can stand, as view origins.  The cells (rx, rz) of a grid with rx % stride == 0
 * and rz % stride == 0 are looked at in ascending record order; a cell is kept when it is FREE with clear2 >= min_clear2, as
 * x = (float)(((double)x0 + rx + 0.5) * (double)leaf * k), z alike (the expression of loamx_grid_route_points), y = elevation +
 * sensor_height, one f32 addition.  *n is the full count; only the first `capacity` triples are written.  LOAMX_E_INVALID: NULL cells,
 * cfg or n;  NULL origins with capacity > 0;  leaf not positive;  stride 0;  sensor_height not finite;  a configuration that fails
 * loamx_densemap_grid_check.
 * loamx_place_view_pose (host only): the start pose (row-major 3x4, map <- query frame) that a match (id, shift) of a query described
 * about query_origin implies for the view at view_origin: in double, psi = shift * 2 pi / n_sectors, R = rot_y(psi) =
 * [[cos psi, 0, sin psi], [0, 1, 0], [-sin psi, 0, cos psi]] — the yaw convention above: the query's frame has turned by +yaw_hint —
 * and t = view_origin - R query_origin: t_x = v_x - (cos psi q_x + sin psi q_z), t_y = v_y - q_y, t_z = v_z - (cos psi q_z -
 * sin psi q_x).  LOAMX_E_INVALID: NULL view_origin or pose;  n_sectors outside 4..128;  shift >= n_sectors;  an origin that is not finite. */
#define LOAMX_PLACE_VIEW_CAST 0
#define LOAMX_PLACE_VIEW_VOXELS 1
#define LOAMX_PLACE_VIEW_MAX_ORIGINS 4096
#define LOAMX_PLACE_VIEW_MAX_RAYS 65536
typedef struct loamx_place_view_config {
  uint32_t mode;                   /* LOAMX_PLACE_VIEW_CAST (default) or LOAMX_PLACE_VIEW_VOXELS */
  uint32_t max_steps, skip_steps;  /* as loamx_densemap_raycast_config (defaults 4096, 0); CAST only */
  uint32_t min_points;             /* a voxel with fewer points is not seen, >= 1 (default 1) */
} loamx_place_view_config;
void loamx_place_view_default_config(loamx_place_view_config* cfg);   /* host only */
int loamx_place_view_rays(uint32_t n_azimuth, const float* elevations, uint32_t n_elevations, float range,
                          float* offsets /* 3 * n_azimuth * n_elevations */);   /* host only */
int loamx_place_add_views(loamx_place* pl, loamx_densemap* dm, const float* origins /* 3 * n */, uint32_t n,
                          const float* offsets /* 3 * n_rays; NULL in VOXELS mode */, uint32_t n_rays,
                          const loamx_place_view_config* cfg /* NULL: the defaults */,
                          const loamx_densemap_static_rule* rule /* NULL: every voxel; else needs carving */,
                          uint32_t* first_id /* may be NULL */, uint64_t stats[6] /* may be NULL */);
int loamx_grid_view_origins(const loamx_grid_cell* cells, const loamx_densemap_grid_config* cfg, float leaf, uint32_t stride,
                            uint32_t min_clear2, float sensor_height, float* origins /* 3 * capacity */, uint64_t capacity,
                            uint64_t* n);   /* host only */
int loamx_place_view_pose(const float view_origin[3], uint32_t shift, int n_sectors, const float query_origin[3] /* NULL: 0 */,
                          double pose[12]);   /* host only */

/* ------------------------------------------------------------------------------------------------------------
 * Pose graph (not in the reference, which never closes a loop): the run's poses optimised on the device, the link between
 * loamx_densemap_align_many / align_pyramid (a 6-DOF constraint between two sweeps) and loamx_densemap_rebuild (one rigid correction
 * per sweep).  All arithmetic is FP64, no fused multiply-add; every sum has one fixed order, so a run is reproducible to the bit.
 *
 * Poses are double[12], a row-major 3x4 matrix (R | t) mapping node frame to map frame: the layout of
 * loamx_densemap_align_result.pose and of rebuild's corrections.
 * Edge (i, j, Z, Omega): Z = (R_z, t_z) is the measured T_i^-1 T_j; Omega is a symmetric 6x6 information matrix given as its 21
 * upper-triangle entries, row-major.
 * Residual: with A = T_i^-1 T_j = (R_A, t_A) and E = Z^-1 A = (R_E, t_E):
 *   R_A = R_i^T R_j,  t_A = R_i^T (t_j - t_i);   R_E = R_z^T R_A,  t_E = R_z^T (t_A - t_z);
 *   r = [t_E ; Log(R_E)]: translation first, then the rotation vector of angle in [0, pi].
 *   Log(R): v = the vector of (R - R^T) / 2, c = (trace R - 1) / 2, angle = atan2(|v|, c), Log = v * angle / |v|, and v itself below
 *   1e-8 rad.  Exp(w) = I + a [w]x + b [w]x^2 with a = sin|w| / |w|, b = (1 - cos|w|) / |w|^2, and a = 1, b = 1/2 below 1e-8 rad.
 *   The series branches are part of the definition.  The caller keeps |Log(R_E)| <= pi - 1e-6.
 * Cost: chi2_e = r^T Omega r;  F = sum_e rho_e(chi2_e);  rho(s) = s for plain edges; for edges flagged LOAMX_PG_EDGE_ROBUST with
 *   huber_delta > 0: rho(s) = s if s <= delta^2, else 2 delta sqrt(s) - delta^2.  The solver treats this as IRLS, with the weight
 *   w_e = min(1, delta / sqrt(chi2)) evaluated at the linearisation point.
 * Retraction: delta_k = (v, w):  t_k <- t_k + R_k v,  R_k <- R_k Exp(w).  A free node's rotation is then made orthonormal again by
 *   Gram-Schmidt on its columns (c0 normalised; c1 minus its part along c0, normalised; c2 = c0 x c1).  Fixed nodes are never written:
 *   get_poses returns them byte for byte as they were given.
 * Jacobians of r at delta = 0, with phi = Log(R_E) and Q = Jr^-1(phi) = I + 1/2 [phi]x + (1/|phi|^2 - (1 + cos|phi|) / (2 |phi|
 *   sin|phi|)) [phi]x^2 (coefficient 1/12 below 1e-8 rad); rows t, phi; columns v, w:
 *   J_j = [[R_E, 0], [0, Q]],   J_i = [[-R_z^T, R_z^T [t_A]x], [0, -Q R_A^T]].
 * Gauge: nodes carry a `fixed` flag, and every connected component of the graph must contain a fixed node; an isolated node must
 *   itself be fixed.
 * One step solves (H + lambda D) delta = -g over the free nodes, H = sum_e w_e J^T Omega J, g = sum_e w_e J^T Omega r, D the 6x6
 *   block diagonal of H, by conjugate gradients preconditioned with the inverse of (1 + lambda) D per node (6x6 Cholesky; a node with a
 *   pivot that is not positive gets a zero step).  CG ends at the first k with r_k.z_k <= cg_tolerance^2 r_0.z_0 or at
 *   max_cg_iterations; the stop is found on the device, so the result does not depend on cg_batch.
 * Levenberg-Marquardt: a step is accepted iff it lowers F (then lambda <- lambda / 10); a rejected step restores the poses and raises
 *   lambda tenfold (to 1e-6 from 0), up to a cap of 1e12 (status 2).  Converged (status 0): an accepted step with max |delta| <= eps_step
 *   or one that lowered F by <= eps_cost * F; also a rejected step with max |delta| <= eps_step (at the minimum rounding alone decides
 *   whether F falls).  max_iterations counts every step tried.
 *
 * Refused with LOAMX_E_INVALID, a message that names the argument, and nothing changed: a NULL where it is not allowed; an id beyond
 * the nodes; i == j; a non-finite entry; a rotation with max |R^T R - I| > 1e-6 or a determinant that is not positive; an info with a
 * negative diagonal entry; optimize / linearise on a graph that fails the gauge check.  LOAMX_E_CAPACITY, handle unchanged: an
 * allocation for growth failed (rooms double).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct loamx_posegraph loamx_posegraph;
typedef struct loamx_posegraph_config {
  uint32_t max_iterations;      /* LM steps tried, 0..10000 (default 50); 0: optimize changes nothing */
  uint32_t max_cg_iterations;   /* per step, 1..100000 (default 500) */
  uint32_t cg_batch;            /* CG iterations enqueued per host look, 1..64 (default 16) */
  uint32_t initial_nodes, initial_edges;   /* room at creation, 1..2^26 (defaults 1024, 2048); both grow by doubling */
  double cg_tolerance;          /* (0, 1): CG ends at the first k with r_k.z_k <= tol^2 * r_0.z_0 (default 1e-8) */
  double eps_step;              /* > 0: converged when an accepted step has max |delta| <= eps_step (default 1e-9) */
  double eps_cost;              /* >= 0: ... or lowered F by <= eps_cost * F (default 1e-12) */
  double lambda_init;           /* >= 0 (default 1e-6) */
  double huber_delta;           /* >= 0; 0: ROBUST flags are ignored (default 0) */
  int device;
} loamx_posegraph_config;
#define LOAMX_PG_EDGE_ROBUST 1u
typedef struct loamx_posegraph_edge {   /* 280 bytes */
  uint32_t i, j, flags, reserved;
  double z[12];
  double info[21];
} loamx_posegraph_edge;
typedef struct loamx_posegraph_result {
  uint32_t iterations, accepted, cg_iterations, looks;
  int status;                   /* 0 converged, 1 max_iterations, 2 lambda reached its cap without an accepted step */
  double cost_initial, cost_final, last_step, lambda_final;
} loamx_posegraph_result;

/* host only, no device needed */
void loamx_posegraph_default_config(loamx_posegraph_config* cfg);
int loamx_posegraph_check(const loamx_posegraph_config* cfg);   /* names the first field out of its bounds */
int loamx_posegraph_between(const double Ti[12], const double Tj[12], double z[12]);   /* z = Ti^-1 Tj: the odometry edge of two sweeps */
int loamx_posegraph_residual(const double Ti[12], const double Tj[12], const double z[12], double r[6]);
/* Omega = diag(1 / sigma_t^2 three times, 1 / sigma_r^2 three times); both sigmas > 0 */
int loamx_posegraph_info_diagonal(double sigma_t, double sigma_r, double info[21]);
/* LOAMX_E_INVALID and *bad_node = the smallest node id of a component without a fixed node (only i and j of the edges are read) */
int loamx_posegraph_check_gauge(uint32_t n_nodes, const uint8_t* fixed, const loamx_posegraph_edge* edges, uint64_t n_edges, uint32_t* bad_node);
/* out_k = after_k * before_k^-1 for n poses: the corrections[12 * n] that loamx_densemap_rebuild takes */
int loamx_posegraph_corrections(const double* before, const double* after, uint32_t n, double* out);

loamx_posegraph* loamx_posegraph_create(const loamx_posegraph_config* cfg);   /* NULL: the defaults */
void loamx_posegraph_destroy(loamx_posegraph* h);
int loamx_posegraph_reset(loamx_posegraph* h);                                /* no nodes, no edges; the rooms and the statistics stay */
/* n new free nodes with ids *first_id (may be NULL) .. *first_id + n - 1 */
int loamx_posegraph_add_nodes(loamx_posegraph* h, const double* poses, uint32_t n, uint32_t* first_id);
int loamx_posegraph_set_fixed(loamx_posegraph* h, uint32_t id, int fixed);
int loamx_posegraph_set_poses(loamx_posegraph* h, uint32_t first, uint32_t n, const double* poses);
int loamx_posegraph_get_poses(loamx_posegraph* h, uint32_t first, uint32_t n, double* poses);
int loamx_posegraph_add_edges(loamx_posegraph* h, const loamx_posegraph_edge* edges, uint64_t n);
int loamx_posegraph_size(loamx_posegraph* h, uint32_t* nodes, uint64_t* edges);
/* the probe: the linearisation at the current poses with the weights of lambda = 0.  chi2[n_edges], grad[6 * n_nodes] (g per node),
 * diag[36 * n_nodes] (the node's block of H, row-major), *cost = F; each may be NULL.  Fixed nodes get zeros in grad and diag */
int loamx_posegraph_linearise(loamx_posegraph* h, double* chi2, double* grad, double* diag, double* cost);
int loamx_posegraph_optimize(loamx_posegraph* h, loamx_posegraph_result* result);   /* result may be NULL */
/* launches, looks (host round trips), CG iterations, linearisations since the handle's creation; never cleared */
int loamx_posegraph_get_stats(loamx_posegraph* h, uint64_t stats[4]);

#ifdef __cplusplus
}
#endif
#endif /* LOAMX_H */
