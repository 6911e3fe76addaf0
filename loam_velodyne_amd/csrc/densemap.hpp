// Dense global map (include/loamx.h, loamx_densemap_*): an open-addressing hash table of voxels in HBM, fed with registered sweeps on the
// device.  Each slot holds a 64-bit key (EMPTY = all ones; a key is < 2^63) and four 64-bit words: n, Sx, Sy, Sz (integer sums of the
// 20-bit fixed-point offsets inside the voxel, so the table does not depend on the order of the additions).
#pragma once
#include "common.h"

namespace loamx {

constexpr unsigned long long DM_EMPTY = ~0ull;
constexpr int DM_QBITS = 20;              // fixed-point bits of the offset inside a voxel
constexpr int DM_KBITS = 21;              // bits per axis of the key: i + 2^20, |i| < 2^20
constexpr float DM_QSCALE = 1048576.f;    // 2^20
constexpr float DM_IMAX = 1048576.f;      // |i| must stay below this

// Where a device-side add reads: a registered cloud that some other handle keeps in HBM, the stream that wrote it, and the pose of the
// sweep.  Filled by the internal accessors of mapping.hip / pipeline.hip (the handle structs stay where they are).
struct DenseSource {
  const float4* pts = nullptr;
  uint32_t n = 0;
  hipStream_t stream = nullptr;
  int device = 0;
  float origin[3] = {0.f, 0.f, 0.f};
  bool has_cloud = false;    // false: the last call produced no registered cloud (the add is LOAMX_SKIPPED)
};

}  // namespace loamx

// internal accessors (not exported in include/loamx.h): the registered cloud of the mapper's last process() / process_linked(), and of
// the slot-th stream registered in the pipeline's last step (LOAMX_E_INVALID for a slot beyond them)
void loamx_map_dense_source(loamx_map* h, loamx::DenseSource& out);
void loamx_pipeline_dense_source(loamx_pipeline* h, uint32_t slot, loamx::DenseSource& out);
