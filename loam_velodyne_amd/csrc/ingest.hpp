// Raw-sweep ingestion: MultiScanRegistration::process, src/lib/MultiScanRegistration.cpp:160-238 —
// axis remap, NaN / zero / out-of-field rejection, vertical angle -> ring (MultiScanMapper :41-66), azimuth -> relTime
// with the halfPassed unwrapping, stable split into per-ring clouds.  Other lidars bring their ring from a table of elevations or a
// ring field and their relTime from a time field (SensorParams); one set of kernels serves every combination.
#pragma once
#include "common.h"

namespace loamx {

struct MapperParams {
  float lower, upper, factor;   // degrees, degrees, (n_rings - 1) / (upper - lower) as a float (MultiScanRegistration.cpp:41-50)
  uint32_t n_rings;
};

// IMU de-skew of the kept points (projectPointToStartOfSweep, src/lib/BasicScanRegistration.cpp:101-147): the host keeps the
// IMU state machine and hands the device one table per sweep.
struct ImuTable {
  uint32_t H = 0;                // history length; 0 = no IMU data (projection is the identity)
  uint32_t idx0 = 0;             // _imuIdx when the sweep's loop starts
  const double* dt = nullptr;    // [H] toSec(_scanTime - history[j].stamp)
  const double* dstamp = nullptr;   // [H] toSec(history[j].stamp - history[j-1].stamp), j >= 1
  const float* state = nullptr;  // [H][9] roll, pitch, yaw, position xyz, velocity xyz
  float start_c[3] = {1, 1, 1}, start_s[3] = {0, 0, 0};   // cos / sin of _imuStart roll, pitch, yaw
  float start_pos[3] = {0, 0, 0}, start_vel[3] = {0, 0, 0};
  double rel_sweep_base = 0;     // toSec(_scanTime - _sweepStart)
};
// _imuCur / _imuPositionShift as the LAST kept point of the sweep leaves them (they feed updateIMUTransform, :258-281)
struct ImuLast {
  float roll, pitch, yaw, pos[3], vel[3], shift[3];
  uint32_t idx, valid;
};

// Sensor model (loamx_sensor_model, include/loamx.h) as the kernels see it: where a record's ring and relTime come from.  The
// reference's mapper is the model RING_BOUNDS + TIME_AZIMUTH.
enum RingSrc : int { RING_BOUNDS = 0, RING_TABLE = 1, RING_FIELD = 2 };
enum TimeSrc : int { TIME_AZIMUTH = 0, TIME_FIELD = 1 };
struct SensorParams {
  MapperParams M;                        // n_rings always; lower / upper / factor for RING_BOUNDS
  int ring_src = RING_BOUNDS, time_src = TIME_AZIMUTH;
  float table[256] = {};                 // RING_TABLE: n_rings elevations (degrees, strictly increasing)
  float max_err = 0;                     // RING_TABLE: max_angle_error_deg
  uint32_t ring_off = 0, ring_type = 0, time_off = 0, time_type = 0;   // field offsets in the record, LOAMX_FIELD_*
  double time_scale = 1;                 // TIME_FIELD: seconds per unit
  uint32_t* ring_fld = nullptr;          // [n] device: the ring field of every record (RING_FIELD; filled by unpack_records)
  double* time_fld = nullptr;            // [n] device: the time field of every record (TIME_FIELD; filled by unpack_records)
};
// the checks of a raw entry point that takes the reference's mapper, and the mapper as SensorParams (MultiScanMapper::set,
// MultiScanRegistration.cpp:41-50); throws LOAMX_E_INVALID
void mapper_check(float lower, float upper, uint32_t n_rings, uint32_t stride);
SensorParams mapper_params(float lower, float upper, uint32_t n_rings);
// validated model (loamx_sensor_model_check) -> SensorParams without the device arrays; throws LOAMX_E_INVALID
void sensor_model_check(const loamx_sensor_model& m, uint32_t stride);
SensorParams sensor_params(const loamx_sensor_model& m);
// records (x, y, z float32 at byte offsets 0 / 4 / 8 of every `stride` bytes; the payload crosses PCIe as it came) -> float4 (x, y, z, 0)
// and, where the model reads them, the ring field (sp.ring_fld) and the time field as a double (sp.time_fld): k_raw_unpack for a
// model that reads no field, k_sensor_unpack otherwise
void unpack_records(const void* d_bytes, uint32_t stride, uint32_t n, const SensorParams& sp, float4* d_out, hipStream_t st);

class RawBinner {
 public:
  static constexpr uint32_t MAX_RINGS = 256;
  void init(hipStream_t st) { st_ = st; }
  // d_raw: n records (x, y, z, unused) in sensor axes and firing order; sp.ring_fld / sp.time_fld: this sweep's unpacked fields.
  // d_out (capacity n): the kept points in the LOAM frame, rings concatenated, intensity = ring + relTime.  d_ring_cnt[n_rings]:
  // points per ring.  Asynchronous.  Launches k_raw_init, k_raw_classify<ring, time>, (TIME_FIELD: k_sns_tref,) k_raw_colscan, (with
  // IMU data: k_raw_imu_need<time>, k_raw_imu_suffix,) k_raw_scatter<time>.
  void run(const float4* d_raw, uint32_t n, const SensorParams& sp, float scan_period, float4* d_out, uint32_t* d_ring_cnt,
           const ImuTable* imu = nullptr, ImuLast* d_last = nullptr);

 private:
  hipStream_t st_ = nullptr;
  DevBuf<int> ring_of_;
  DevBuf<uint32_t> blk_cnt_, blk_pre_, scratch_, imu_first_, blk_idx_;
  DevBuf<double> blk_tmin_, tref_;
};

}  // namespace loamx
