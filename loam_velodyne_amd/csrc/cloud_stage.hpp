// How a cloud reaches a feature of the dense map (densemap*.hip) or the place database (place.hip): a DenseSource, the points where they
// lie on the device.  A mapper, a pipeline slot and the sweep log fill one; a cloud from the host goes up through a DmCloudStage, which
// fills one too.  A new feature that reads a cloud takes a DenseSource.
#pragma once
#include "common.h"
#include "pinned_copy.hpp"

namespace loamx {

// `behind` runs behind whatever `ahead` holds now (one stream: it does already, and no event is issued)
inline void dm_stream_behind(hipStream_t behind, hipStream_t ahead) {
  if (behind == ahead) return;
  hipEvent_t ev = nullptr;
  LX_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, ahead);
  if (e == hipSuccess) e = hipStreamWaitEvent(behind, ev, 0);
  (void)hipEventDestroy(ev);   // (the wait keeps what it needs)
  LX_HIP(e);
}

struct DmCloudStage;

// Where a feature reads its cloud: points that lie in HBM, the stream that wrote them, and the origin of the sweep (an alignment's
// centre).  Filled by the internal accessors of mapping.hip / pipeline.hip (the handle structs stay where they are), by
// DenseMap::history_source and, for a cloud from the host, by DmCloudStage::source.  A body reads the cloud at points(), once, at the
// place where it first needs it: a cloud from the host goes up there, so a call that is refused or skipped before has moved nothing
struct DenseSource {
  const float4* pts = nullptr;
  uint32_t n = 0;
  hipStream_t stream = nullptr;
  int device = 0;
  float origin[3] = {0.f, 0.f, 0.f};
  bool has_cloud = false;    // false: the last call produced no registered cloud (the feature is LOAMX_SKIPPED)
  const loamx_cloud* host = nullptr;   // a checked cloud that is still on the host, and the stager it goes up through
  DmCloudStage* via = nullptr;
  inline const float4* points() const;
};

// A cloud from the host on its way to the device: a pinned block and a device block, grown to the largest cloud.  The one way up for the
// dense map and the place database; each feature that stages keeps one of its own, so that their clouds stay resident independently
// of each other, and every call on one stager passes the same stream, the handle's own (as scan.hpp asks of a scan state).
//
// The rule, the same for every user:
//   - The pinned block is rewritten only when the fetch that read it has run: stage() records a guard event behind its fetch, and the
//     next stage() waits for that event before it packs.  settle() is the same wait for a handle that is about to wait for its work.
//   - The device block is replaced (a cloud larger than any before) only when the stream is idle: stage() synchronises it first, so
//     that nothing enqueued behind an earlier stage() still reads the block that goes.  A cloud that fits costs no wait.
//   - A stager whose every user waits for the stream before it returns (the alignments, the segmentation, the distance query) is
//     constructed without the guard: the fetch has run when the next stage() packs.  With it such a user would pay one event record
//     per call and a wait for an event that has completed, measured at 7 us of the 165 us of a blocking align_step (CHANGELOG.md).
struct DmCloudStage {
  explicit DmCloudStage(bool guard = true) : guarded_(guard) {}
  DmCloudStage(const DmCloudStage&) = delete;
  DmCloudStage& operator=(const DmCloudStage&) = delete;
  ~DmCloudStage() { if (ev_staged_) (void)hipEventDestroy(ev_staged_); }

  // the points of a checked cloud, packed, in the device block, enqueued on st (count + 1 entries: an empty cloud has a pointer too)
  const float4* stage(const loamx_cloud* c, hipStream_t st) {
    const uint32_t n = c->count;
    settle();
    h_.reserve((size_t)n + 1);
    if (d_.p && (size_t)n + 1 > d_.cap) LX_HIP(hipStreamSynchronize(st));
    d_.reserve((size_t)n + 1);
    if (n) {
      pack_cloud(c, h_.p);
      fetch_from_pinned(d_.p, h_.p, n, st);
      if (guarded_) {
        if (!ev_staged_) LX_HIP(hipEventCreateWithFlags(&ev_staged_, hipEventDisableTiming));
        LX_HIP(hipEventRecord(ev_staged_, st));
        staged_pending_ = true;
      }
    }
    return d_.p;
  }
  // a checked cloud as the source of a feature: staged by points() on the handle's own stream st, about origin (NULL: zeros)
  DenseSource source(const loamx_cloud* c, const float origin[3], hipStream_t st, int device) {
    DenseSource s;
    s.host = c;
    s.via = this;
    s.n = c->count;
    s.stream = st;
    s.device = device;
    for (int a = 0; a < 3; a++) s.origin[a] = origin ? origin[a] : 0.f;
    s.has_cloud = true;
    return s;
  }
  // the pinned block is free: the last fetch has run
  void settle() {
    if (staged_pending_) { LX_HIP(hipEventSynchronize(ev_staged_)); staged_pending_ = false; }
  }

 private:
  PinBuf<float4> h_;
  DevBuf<float4> d_;
  hipEvent_t ev_staged_ = nullptr;   // the guard: behind the last fetch
  bool staged_pending_ = false;
  const bool guarded_;
};

inline const float4* DenseSource::points() const { return host ? via->stage(host, stream) : pts; }

}  // namespace loamx

// internal accessors (not exported in include/loamx.h): the registered cloud of the mapper's last process() / process_linked(), and of
// the slot-th stream registered in the pipeline's last step (LOAMX_E_INVALID for a slot beyond them)
void loamx_map_dense_source(loamx_map* h, loamx::DenseSource& out);
void loamx_pipeline_dense_source(loamx_pipeline* h, uint32_t slot, loamx::DenseSource& out);
