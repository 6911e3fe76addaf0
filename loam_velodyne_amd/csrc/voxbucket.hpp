// Bucketed voxel-grid down-sampling of the registration's stack clouds (pcl::VoxelGrid semantics, BasicLaserMapping.cpp:512-527)
// in three short launches — no phase barriers, no multi-pass global sort, no histogram:
//   k_vb_plan     four workgroups per segment (sweep x {corner, surf}): 512 evenly spaced points of the segment are ranked by their
//                 voxel (iz, iy, ix) — each workgroup ranks a quarter of the keys, four threads to a key — and every
//                 (512 / buckets)-th one becomes a splitter, stored by the thread that finds its key at that rank: the segment's
//                 voxel order is cut into ceil(points / VB_T) contiguous ranges ("buckets") of about VB_T points each.  One record
//                 per bucket (VbBk) carries what k_vb_reduce needs of the segment.  When the caller hands it a VbPoseInit, one
//                 workgroup of an even segment also sets its sweep up (pose from the guess, cleared statistics and marks): the
//                 registration's k_pose_init launch in front of the stage goes.
//   k_vb_stack    one thread per point: the map -> sensor round trip itself (:512-516), the exact voxel, its bucket (binary search
//                 over the segment's splitters), the bucket's point count (counters aggregated per workgroup) and ONE 16-bit word
//                 per point: its bucket inside its segment (VB_REFUSED where the point was not taken).  Per chunk of 256 points
//                 the smallest and largest bucket its accepted points touch.  No slot arrays: nothing is scattered.
//   k_vb_reduce   one workgroup per bucket: the bucket COLLECTS its points itself, in input order — it scans the bucket words of its
//                 segment's chunks (those whose bucket range holds it) and compacts the matching positions — gathers every point
//                 once, into LDS, at its rank e in that order, linearises the voxel indices over the bucket's own bounding box
//                 (few bits) and sorts (voxel index << e bits | e) with a stable LSD radix sort in LDS on the VOXEL bits alone: input
//                 order inside a voxel is the stable sort's own doing.  Run heads, output offset from a look-back over the earlier
//                 buckets' head counts, voxel means summed in input order from the points in LDS.
// Buckets are ranges of the voxel order, so the buckets of a segment one after the other ARE pcl::VoxelGrid's output order, whatever
// the splitters: the sample only balances the load.  A bucket over capacity (a sample that missed a dense spot, more than VB_CAP
// points in one voxel), a coordinate beyond +-2^20 voxels, a segment box with more than INT_MAX voxels (PCL's pass-through case)
// raise the run's fail word; the kernels then leave an empty result and the host re-runs the sweep(s) through the general kernel
// (k_vox_ds_seg).  Output is bit-identical to that kernel's (same voxel order, same summation order).
#pragma once
#include "common.h"
#include "dev_math.hpp"

namespace loamx {

#ifndef VB_CAP_LOG2
#define VB_CAP_LOG2 12
#endif
constexpr int VB_CAP = 1 << VB_CAP_LOG2;        // points per bucket at most (4096: a 512-thread workgroup with 106 KB of LDS, one per CU)
constexpr int VB_T = VB_CAP / 2;                // target points per bucket
constexpr int VB_SAMPLE = 512;                  // sample size per segment (= threads of k_vb_plan); also the most buckets a segment may have
constexpr int VB_MAXSEG = 4096;
constexpr int VB_CHUNK = 256;                   // points per chunk summary (= threads of k_vb_stack)
constexpr uint16_t VB_REFUSED = 0xffffu;        // bucket word of a point that no bucket took (a bucket inside its segment is < VB_SAMPLE)

struct VbSeg {        // plan of one segment
  uint32_t bucket0;   // first bucket (index into the run's bucket arrays)
  uint32_t nbuckets;
  uint32_t pos_bits;  // bits of the largest input position inside the segment
  uint32_t pad;
};

// the registration's per-sweep set-up, done by k_vb_plan on the way (registration.hip, k_pose_init: the same stores)
struct VbPoseInit {
  const float* guess = nullptr;   // [ns][6] rx ry rz tx ty tz; nullptr: nothing to set up
  Pose* poses = nullptr;
  int* stats = nullptr;           // [ns][8] (SweepStats), cleared
  int* seg_minmax = nullptr;      // [ns][12] voxel bounds of the sweep's two segments (general kernel), reset
  uint32_t* ticket = nullptr;     // [ns] cleared
  uint32_t* full_done = nullptr;  // [ns] cleared
  uint32_t ns = 0;
};

struct alignas(16) VbBk {   // plan of one bucket: what k_vb_reduce needs of its segment
  uint32_t seg, sbeg, send;   // the segment and its range of the input
  uint32_t bucket0, pos_bits; // as in VbSeg
  uint32_t pad[3];
};

class VoxBucket {
 public:
  void init(hipStream_t st) { st_ = st; }
  // segments = contiguous ranges [h_seg_off[k], h_seg_off[k+1]) of the n input points (read from in, or from src[k] when given);
  // segment k belongs to sweep k / 2 (poses) and uses inv_even / inv_odd = 1 / leaf by parity.  stack receives the round-trip
  // points, out / d_out_off the voxel means and the nseg + 1 output offsets.  Asynchronous on the stream.
  // init (optional): sweep s = segment 2 s is set up by the plan, one launch ahead of the first reader of d_poses.
  void run(const float4* in, const float4* const* d_src, uint32_t n, const uint32_t* d_seg_off, const uint32_t* h_seg_off, uint32_t nseg,
           const Pose* d_poses, float inv_even, float inv_odd, float4* stack, float4* out, uint32_t* d_out_off,
           const VbPoseInit* init = nullptr);
  static bool fits(uint32_t n, uint32_t nseg) { return nseg >= 1 && nseg <= (uint32_t)VB_MAXSEG && n >= 1 && n < (1u << 24); }
  // after the stream has been synchronised: did the last run() give up (the caller must redo it with the general kernel)?
  bool failed() const { return h_fail_.p && *(volatile uint32_t*)h_fail_.p == epoch_; }
  // device word / value a later kernel of the same stream can test to skip work that would use the empty result
  const uint32_t* d_fail_word() const { return ctl_.p; }
  uint32_t epoch() const { return epoch_; }
  uint32_t why() const;   // after failed(): bit mask of the give-up reasons (voxbucket.hip, vb_fail)
  void check();   // throws when a look-back wait timed out
  uint32_t last_buckets() const { return nb_; }
  // the last run's plan, read-only (loamx_voxbucket_probe): one VbSeg per segment, per bucket its splitter and its point count
  const VbSeg* d_segs() const { return segs_.p; }
  const unsigned long long* d_lo() const { return lo_.p; }
  const uint32_t* d_cnt() const { return cnt_.p; }

 private:
  hipStream_t st_ = nullptr;
  DevBuf<VbSeg> segs_;
  DevBuf<unsigned long long> lo_;          // per bucket: the smallest voxel key it takes (the first bucket of a segment: 0)
  DevBuf<VbBk> bk_;                        // per bucket: its segment's record
  DevBuf<int> box_;                        // [nseg][6] voxel bounds of the stack points (k_vb_reduce; PCL's pass-through test)
  DevBuf<uint32_t> cnt_, heads_, ctl_;     // per bucket: points, run heads + 1 once published; ctl: [0] fail epoch, [1] arrivals of k_vb_reduce
  DevBuf<uint16_t> bword_;                 // per point: its bucket inside its segment, or VB_REFUSED (padded to whole chunks)
  DevBuf<uint2> crange_;                   // per chunk of VB_CHUNK points: smallest / largest bucket (of the run) its accepted points touch
  PinBuf<uint32_t> h_fail_;                // [0] fail epoch (host-visible copy), [1] timeout, [2..] epoch of the last run that met reason r
  uint32_t epoch_ = 0, nb_ = 0;
  bool ctl_ready_ = false;
};

}  // namespace loamx
