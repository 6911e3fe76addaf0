// Scan-to-map registration engine shared by the batched mode (loamx_batch_*) and the sequential
// BasicLaserMapping replacement (loamx_map_*).  Host classes; kernels live in registration.hip.
#pragma once
#include <functional>
#include "common.h"
#include "dev_math.hpp"
#include "reg_schedule.hpp"
#include "submap_index.hpp"
#include "voxel.hpp"
#include "voxbucket.hpp"

namespace loamx {

constexpr int LX_RES_THREADS = 256;
constexpr int LX_NSUM = 28;   // 21 upper-triangular AtA + 6 AtB + row count

struct SweepStats {
  int iterations, sel, corner_q, surf_q, degenerate, done, pad0, pad1;
};

// check word of the pinned (pose, statistics) mirror of one sweep: the host polls `done` while the kernel may still be
// storing, and takes the pair only when the word it finds matches the words it read (SweepStats::pad1 of the mirror)
__host__ __device__ inline int mirror_check_word(const SweepStats& st, const Pose& T) {
  const unsigned* w = reinterpret_cast<const unsigned*>(&T);
  unsigned x = 0x5bd1e995u ^ (unsigned)st.iterations ^ ((unsigned)st.sel << 8) ^ ((unsigned)st.degenerate << 30);
  for (int i = 0; i < (int)(sizeof(Pose) / 4); i++) x = (x << 5 | x >> 27) ^ w[i];
  return (int)x;
}

struct RegParams {
  int max_iterations = 10;
  float delta_t_abort = 0.05f, delta_r_abort = 0.05f;
  float corner_leaf = 0.2f, surf_leaf = 0.4f;
};

// Registers up to max_sweeps sweeps' (corner_last, surf_last) against the two indexed sub-maps.
class Registrar {
 public:
  Registrar(int device, uint32_t max_sweeps);
  ~Registrar();
  RegParams params;
  SubMapIndex corner_index, surf_index;
  // Double-buffered sub-map (BASELINE configs[4]): the NEXT epoch's map is indexed on a stream of its own
  // while sweeps are still registered against the current one; swap_submap() makes it current at a batch boundary.
  // The caller's buffers are only read until the staged build has finished (the index keeps a cell-sorted copy).
  void stage_submap_device(const float4* d_corner, uint32_t nc, const float4* d_surf, uint32_t ns, hipEvent_t wait_for = nullptr);
  void stage_submap_host(const loamx_cloud* corner, const loamx_cloud* surf);
  bool submap_staged() const { return next_staged_; }
  void swap_submap();
  bool double_buffer_full = false;   // stage_full() alternates between two buffers (the pipeline's asynchronous downloads)
  bool defer_full = false;    // run_async() leaves the full-resolution clouds unregistered; finish_with_poses() does it
  void finish_with_poses(const float* poses6);
  std::function<void()> on_first_wait;   // early_exit: called once, right before run_async() first blocks on the flags
  bool early_exit = false;    // run_async() may block on the done flags to skip the launches after convergence
  hipStream_t stream() const { return st_; }

  // frozen sub-map (host records or device float4)
  void set_submap_host(const loamx_cloud* corner, const loamx_cloud* surf);
  void set_submap_device(const float4* d_corner, uint32_t nc, const float4* d_surf, uint32_t ns, bool sync = true);

  // stage inputs (H2D, async on the stream)
  void upload(uint32_t n_sweeps, const loamx_cloud* corner_last, const loamx_cloud* surf_last, const loamx_cloud* full_res,
              const float* guess6, bool wait = true);
  // same with device-resident packed float4 inputs (copied device-to-device; async on the stream)
  void upload_device(uint32_t n_sweeps, const float4* const* corner_last, const uint32_t* n_corner, const float4* const* surf_last,
                     const uint32_t* n_surf, const float4* const* full_res, const uint32_t* n_full, const float* guess6);
  // reserve the full-resolution staging area for the next upload_device() and return it: the caller fills
  // [full_offset(s), full_offset(s+1)) itself (e.g. with a fused re-projection kernel) and passes full_res = NULL
  float4* stage_full(uint32_t n_sweeps, const uint32_t* n_full);
  float4* stage_full_next(uint32_t n_sweeps, const uint32_t* n_full);   // NULL: not possible now
  bool adopt_full_next(uint32_t n_sweeps, const uint32_t* n_full);      // false: nothing (matching) was pre-staged
  // device-only: stack round trip + voxel DS + LM iterations (+ full-res registration)
  // force_general: the stack clouds' voxel grid through the general kernel (the repeat of a run whose bucketed stage gave up)
  void run_async(bool force_general = false);
  void sync();
  void download(float* poses6, int* stats4);
  void download_stats(SweepStats* out);
  int download_full_res(uint32_t sweep, loamx_cloud* out);
  void download_full_res_async(uint32_t sweep, const loamx_cloud* into = nullptr);   // into: the cloud download_full_res() will be given (a pinned one takes the copy directly)
  void set_submap_device_split(const float4* d_corner, uint32_t nc, hipStream_t corner_stream, const float4* d_surf, uint32_t ns, bool bounds_done = false);
  // down-sampled query clouds of a sweep (device pointers valid until the next run); counts need a sync'd download
  void download_ds(uint32_t sweep, std::vector<float4>& corner_ds, std::vector<float4>& surf_ds);
  // their sizes alone (corner, surf): what SweepStats::corner_q / surf_q hold once a Gauss-Newton update has run — a run without one leaves them unwritten
  void download_ds_counts(uint32_t sweep, uint32_t counts[2]);
  // registered (final-pose) DS clouds, for map insertion: device array + offsets
  const float4* d_ds_points() const { return ds_pts_.p; }
  const uint32_t* d_ds_offsets() const { return ds_off_.p; }
  const Pose* d_poses() const { return poses_.p; }
  const float4* d_full_res() const { return full_.p; }
  uint32_t full_offset(uint32_t s) const { return h_full_off_[s]; }

  // parity hook (loamx_batch_knn_probe): exact 5-NN of n map-frame points in the corner (0) / surf (1) sub-map index
  void knn_probe(int which, const float* xyz, uint32_t n, uint32_t* idx5, float* d2_5);
  void qr6_probe(const float* ata, const float* atb, uint32_t n, float* x_coop, float* x_scalar);
  void xrec_stress(uint32_t pairs, uint32_t rounds, unsigned long long out4[4]);
  void set_timing(bool on, bool per_launch = true) { timing_ = on; launch_timing_ = per_launch; }   // per_launch: event pairs around every Gauss-Newton launch
  void get_timing(float ms[4], uint64_t counts[4]);
  uint32_t n_sweeps() const { return n_sweeps_; }
  bool submap_sufficient() const { return corner_index.size() > 10 && surf_index.size() > 100; }

 private:
  int device_;
  uint32_t max_sweeps_, n_sweeps_ = 0;
  hipStream_t st_ = nullptr;
  bool timing_ = false, timed_run_ = false, launch_timing_ = true;

  // owned copies of a host-provided sub-map
  DevBuf<float4> own_corner_, own_surf_;

  // inputs: segments 2s (corner), 2s+1 (surf)
  PinBuf<float4> h_in_, h_full_;
  std::vector<uint32_t> h_seg_off_, h_full_off_;
  PinBuf<float> h_guess_;        // finish_with_poses(): 6 per sweep
  DevBuf<float4> in_, stack_, ds_pts_, full_, full_alt_;
  DevBuf<uint32_t> ds_off_;
  DevBuf<float> guess_;
  bool full_staged_ = false, full_next_staged_ = false;   // stage_full() / stage_full_next() wrote h_full_off_ / next_full_off_ for the next upload_device()
  std::vector<uint32_t> next_full_off_;
  hipEvent_t ev_look_ = nullptr;
  PinBuf<float4> h_full_dl_;      // download_full_res(): pinned landing area of one sweep's registered cloud
  // What the host knows about the current run: assigned afresh by every attempt of run_async(); finish_with_poses() keeps only the owed verdict
  struct Run {
    bool vb_unchecked = false;     // the attempt took the bucketed voxel path and its fail word has not been looked at yet
    bool mirrors_written = false;  // h_poses_ / h_stats_ hold (after a stream sync) this run's final values
    bool results_final = false;    // ... and the host has seen them complete: fetch_results() need not wait for the stream
    int full_dl_sweep = -1;        // the sweep whose copy download_full_res_async() has enqueued since the clouds were registered (-1: none)
    void* full_dl_direct = nullptr;   // ... straight into this caller memory
  } run_;
  VoxelPipeline vox_;
  // the stack clouds' voxel grid normally takes the bucketed path (voxbucket.hpp); a run that gives up is repeated through the
  // general kernel as soon as the host has synchronised with it (LOAMX_VOX_LEGACY=1 forces the general kernel)
  VoxBucket vb_;
  bool vb_disabled_ = false;   // LOAMX_VOX_LEGACY
  bool jacobi_eig_ = false;    // LOAMX_EIG_JACOBI: the edge fit's eigen-decomposition by the oracle's Jacobi iteration instead of the closed form
  void enqueue_front(bool legacy);   // sweep set-up (k_pose_init, or inside k_vb_plan) + stack round trip + voxel grid
  void enqueue_full(int mode);       // transformFullResToMap
  void redo_if_bucket_path_failed(); // after a stream sync
  uint32_t n_in_ = 0, n_full_ = 0, max_q_per_sweep_ = 0;
  struct RunTrace;   // LOAMX_REG_TRACE: host stamps of one run_async()
  // inputs, written once for upload() and upload_device(): checks, offsets, reserves / the parameter block and its four views
  template <class Count> void plan_inputs_(uint32_t n_sweeps, bool staged, Count&& count);
  size_t write_param_block_(const float* guess6, const float4* const* corner_src, const float4* const* surf_src, const float4* const* full_src);
  void begin_attempt_(bool legacy);
  RegOutcome run_iterations(RunTrace& tr);   // the Ops of reg_schedule(): Gauss-Newton launches, looks at the mirrors, full-resolution launches
  bool bucket_stage_gave_up_();              // the owed verdict, looked at (after a wait that covers the voxel stage)
  void dump_gn_profile_();                   // LOAMX_PROF_GN builds
  bool wait_for_mirrors();
  void fetch_results();
  int pred_iters_ = 4;        // early_exit: iterations to enqueue before the first look at the done flags

  DevBuf<Pose> poses_;
  DevBuf<SweepStats> stats_;
  DevBuf<float> matP_;        // 36 per sweep
  DevBuf<double> partials_;   // per sweep x blocks x LX_NSUM
  // views of the per-run parameters (separate buffers after upload(), one block after upload_device())
  const float* d_guess_ = nullptr;
  const uint32_t* d_seg_off_ = nullptr;
  const uint32_t* d_full_off_ = nullptr;
  const float4* const* d_src_ = nullptr;
  DevBuf<char> blob_;
  PinBuf<char> h_blob_;
  SubMapIndex corner_next_, surf_next_;
  DevBuf<float4> next_corner_, next_surf_;
  PinBuf<float4> h_next_corner_, h_next_surf_;
  hipStream_t st_build_ = nullptr;
  hipEvent_t ev_build_ = nullptr, ev_swap_ = nullptr;
  bool next_staged_ = false, swapped_once_ = false;
  DevBuf<uint32_t> arrive_;   // per sweep: k_gn_iter workgroups that have delivered their tile sums
  DevBuf<uint32_t> full_done_;   // per sweep: tag of the k_transform_full launch that registered its full-resolution cloud
  uint32_t full_tag_ = 0;
  uint32_t nblk_ = 0;

  std::vector<hipEvent_t> ev_;   // timing events: [0]=run start, [1]=run end, then pairs per Gauss-Newton launch
  int n_res_launch_ = 0;
  PinBuf<SweepStats> h_stats_;
  PinBuf<Pose> h_poses_;
};

}  // namespace loamx
