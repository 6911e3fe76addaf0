// Batched streaming pipeline: n independent streams, each advancing one sweep per step through
//   feature extraction (BasicScanRegistration) -> odometry (BasicLaserOdometry) -> registration against a frozen
//   sub-map (BasicLaserMapping::optimizeTransformTobeMapped, transformAssociateToMap, transformFullResToMap).
// This is the batched-sweep mode of BASELINE.json's north_star: the streams are the independent units that are sharded
// across GPUs; every stream keeps the reference's sequential semantics (its odometry state, its
// transformBefMapped / transformAftMapped), only the map is frozen for the epoch.  All device work of a step runs on one
// HIP stream with inputs resident in HBM; the host touches only offsets and 6-float poses between the stages.
#include "pinned_copy.hpp"
#include "features.hpp"
#include "odometry.hpp"
#include "registration.hpp"
#include "hostlink.hpp"
#include "densemap.hpp"
#include "odom_lookahead.hpp"
#include <atomic>
#include <deque>
#include <chrono>
#include <mutex>
#include <memory>

namespace loamx {

// what odometry hands on to the registration of the same sweep
struct OdomPub {
  HTwist transform, transform_sum;
  OdomStats stats = {0, 0, 0, 0};
  int rc = LOAMX_SKIPPED;
  const float4* last_corner = nullptr; uint32_t n_last_corner = 0;
  const float4* last_surf = nullptr; uint32_t n_last_surf = 0;
  ToEndParams to_end;
};

struct PipeStreamState {
  HTwist bef, aft, tobe, incre;   // mapping-side transforms (transformSum comes from the odometry stream)
  OdomPub cur;                    // odometry results of the step being registered (the look-ahead's wait in Pipeline::ores)
  SweepStats map_stats = {0, 0, 0, 0, 0, 0, 0, 0};
  bool mapped = false;
};

class Pipeline {
 public:
  Pipeline(const loamx_scanreg_config& fc, const loamx_odom_config& oc, const loamx_map_config& mc, uint32_t n_streams)
      : reg(mc.device, n_streams), fcfg(fc), n_streams_(n_streams), st(n_streams), imu(n_streams), map_imu(n_streams), map_imu_seq(n_streams, 0) {
    // The odometry of the streams runs as G independent chains ("groups"), each with its own OdometryBatch, HIP stream and host thread:
    // a stream whose sweep needs 25 iterations (BasicLaserOdometry.cpp:246 runs to maxIterations when the stop test at :613-620 never
    // fires) delays only its own group, and the two steps of look-ahead absorb it — with ONE chain every step paid the launch pairs of
    // the slowest of all streams (profiles/r03: 5.2 pairs per step for a mean of 7.1 iterations).  Default 2: measured on MI355X
    // (profiles/r04_groups_ab.md) 1 -> 2 chains gains 8 %, but with 4 (six busy HIP streams in the process) EVERY chain slows down
    // (registration 0.55 -> 0.88 ms, k_gn_iter 64 -> 93 us) and the step is 35 % slower than with one.
    // Round 4 / 5, measured and removed: an engine that let EVERY stream run at its own pace inside shared launches (a per-stream state
    // machine on the device).  Bit-identical, but slower on the bench workload even with six steps of look-ahead and its thread off
    // the runtime's locks (16.3 k sweeps/s against the chains' 17.9 k, profiles/r05_ab.md): the code is in the history (odom_engine.inc).
    OdomParams op;
    op.scan_period = oc.scan_period;
    op.max_iterations = diag_env("LOAMX_ODOM_MAXIT") ? atoi(diag_env("LOAMX_ODOM_MAXIT")) : oc.max_iterations;   // (diagnostic override, LOAMX_DIAG builds only)
    if (op.max_iterations < 1 || op.max_iterations > 255) throw Error(LOAMX_E_INVALID, "odometry max_iterations must be in [1, 255]");   // (k_odom_lm tags its exchange records with iteration + 1 in 8 bits)
    op.delta_t_abort = oc.delta_t_abort;
    op.delta_r_abort = oc.delta_r_abort;
    {
      int g = (int)std::min<uint32_t>(n_streams, 2);
      if (const char* e = diag_env("LOAMX_ODOM_GROUPS")) g = atoi(e);
      n_groups = (uint32_t)std::max(1, std::min(g, (int)std::min<uint32_t>(n_streams, MAX_GROUPS)));
    }
    for (uint32_t g = 0; g < n_groups; g++) {
      chains.emplace_back(new OdomChain());
      OdomChain& c = *chains.back();
      c.s0 = (uint32_t)((uint64_t)g * n_streams / n_groups);
      c.s1 = (uint32_t)((uint64_t)(g + 1) * n_streams / n_groups);
      c.ob.reset(new OdometryBatch(mc.device, c.s1 - c.s0, nullptr));
    }
    for (auto& o : ores) o.resize(n_streams);
    for (auto& tr : imu) tr.history_size = std::max(200, fc.imu_history_size);
    reg.params.max_iterations = mc.max_iterations;
    reg.early_exit = true;   // step() blocks on M(t) anyway
    reg.double_buffer_full = true;   // two full-resolution staging buffers: the next step's re-projected clouds are written while this step's are registered (prestage_gather)
    reg.params.delta_t_abort = mc.delta_t_abort;
    reg.params.delta_r_abort = mc.delta_r_abort;
    reg.params.corner_leaf = mc.corner_filter_size;
    reg.params.surf_leaf = mc.surf_filter_size;
    for (auto& c : chains) { c->ob->params = op; c->ob->set_keep(OR - 2); }
    device = mc.device;
    if (getenv("LOAMX_NO_LOOKAHEAD")) prefetch = false;   // debugging / profiling: run the stages one after the other
    const double spin_us = diag_env("LOAMX_SPIN_US") ? atof(diag_env("LOAMX_SPIN_US")) : 400.0;   // diagnostic
    la.reset(new LookAhead(
        n_groups, [this](uint32_t g, int k) { run_chain_step(*chains[g], (uint32_t)k); }, [this] { (void)hipSetDevice(device); },
        std::chrono::duration_cast<std::chrono::steady_clock::duration>(std::chrono::duration<double, std::micro>(spin_us))));
  }
  Registrar reg;
  // Look-ahead rings: what a look-ahead step leaves behind for its registration (feature offsets, odometry results, events, timers)
  // lives in slot step % OR, so the odometry may run up to OR - 2 steps ahead of the registration (ahead_depth below)
  static constexpr int OR = 16;
  // stage timers are read lazily (an elapsed time is taken once both events have completed) so that measuring never
  // makes the host wait for a stage
  struct LazyTimer {
    hipEvent_t a = nullptr, b = nullptr;
    bool pending = false;
    float ms = 0.f;
    void start(hipStream_t s) {
      if (!a) { LX_HIP(hipEventCreate(&a)); LX_HIP(hipEventCreate(&b)); }
      pending = false;
      LX_HIP(hipEventRecord(a, s));
    }
    void stop(hipStream_t s) { LX_HIP(hipEventRecord(b, s)); pending = true; }
    bool resolve() {   // true: a time has just been taken
      if (!pending || hipEventQuery(b) != hipSuccess) return false;
      LX_HIP(hipEventElapsedTime(&ms, a, b));
      pending = false;
      return true;
    }
    void destroy() { if (a) { (void)hipEventDestroy(a); (void)hipEventDestroy(b); a = b = nullptr; } }
  };
  // one odometry chain: the streams [s0, s1) and their batch object (own HIP stream); its host thread and its position are the
  // look-ahead gate's (`la`)
  struct OdomChain {
    uint32_t s0 = 0, s1 = 0;
    std::unique_ptr<OdometryBatch> ob;
    hipEvent_t ev_tail[OR] = {};   // recorded behind O(k)'s tail (re-projection + index build) on the chain's stream
    LazyTimer tm[OR];                    // chain timer of step k % OR (the chain's thread's own)
    std::atomic<float> ms{0.f};          // length of the chain's most recent timed pass on its HIP stream
    double tr[4] = {0, 0, 0, 0};
    std::atomic<float> last_us{0.f};     // host time of the chain's most recent pass (LOAMX_PIPE_TRACE)
  };
  static constexpr uint32_t MAX_GROUPS = 16;
  uint32_t n_groups = 1;
  std::vector<std::unique_ptr<OdomChain>> chains;
  OdomChain& chain_of(uint32_t s) { uint32_t g = 0; while (g + 1 < n_groups && s >= chains[g]->s1) g++; return *chains[g]; }
  OdometryBatch& OB(uint32_t s) { return *chain_of(s).ob; }
  uint32_t LS(uint32_t s) { return s - chain_of(s).s0; }   // index of stream s inside its group
  loamx_scanreg_config fcfg;
  uint32_t n_streams_;
  int device;
  std::vector<PipeStreamState> st;
  std::vector<std::unique_ptr<FeatureExtractor>> fx;   // one staged batch per step (upload) or a ring of RING slots (stage_step)
  // Streaming input (loamx_pipeline_stage_step): step t lives in slot t % RING; steps t .. t + RING - 2 may be in flight while
  // t + RING - 1 is being staged.  The copies run on a stream of their own; launch_features() orders the extraction behind their event.
  static constexpr uint32_t RING = 8;
  bool streaming = false;
  // streaming: steps below staged_hi have been staged.  stage_step* may run on ONE other thread than step(): it publishes the slot
  // (release) after everything of it is enqueued, step() reads the count once (acquire); the two never touch the same slot — the
  // stager works on the slot of step t + RING - 1 at most while steps <= t + RING - 2 are in flight
  std::atomic<uint32_t> staged_hi{0};
  hipStream_t cstream = nullptr, dstream = nullptr;      // H2D staging / D2H of the registered clouds
  hipEvent_t ev_stage[RING] = {};
  hipEvent_t ev_reg_done = nullptr, ev_d2h[2] = {nullptr, nullptr};
  bool d2h_pending[2] = {false, false};
  uint64_t downloads_direct = 0, downloads_hip = 0;      // asynchronous downloads issued to the SDMA engine directly / through hipMemcpyAsync
  HostLinkDma hostlink;                                   // the same downloads on the SDMA engine directly (hostlink.hpp)
  HostLinkUp uplink;                                      // ... and the staging copies of stage_step (slot = t % RING); LOAMX_H2D_DIRECT=0: through HIP
  uint32_t up_runs[RING] = {};                            // block copies of the slot's step handed to uplink (0: none, the HIP copy stream carried them)
  std::atomic<long> last_step{-1};                        // the last step that has run (-1: none yet)
  std::vector<uint32_t> last_full_off;                   // offsets of the registered clouds of the last step (k-th mapped stream)
  std::vector<uint32_t> last_who;                        // ... and the stream of each (loamx_densemap_add_from_pipeline: its pose)
  // Raw input (loamx_pipeline_stage_step_raw): per slot the payloads, their binned clouds and what the binning leaves behind
  struct RawSlot {
    bool raw = false, finalized = true;
    std::vector<uint32_t> count, off;            // raw points per stream, their offsets in the slot's arrays
    DevBuf<char> d_bytes;
    DevBuf<float4> d_raw4, d_binned;
    DevBuf<uint32_t> d_ring_fld;                 // stage_step_sensor: the records' ring / time fields (as the model reads them)
    DevBuf<double> d_time_fld;
    DevBuf<uint32_t> d_ring_cnt;                 // [stream][n_rings]
    PinBuf<uint32_t> h_ring_cnt;
    DevBuf<ImuLast> d_last;
    PinBuf<ImuLast> h_last;
    DevBuf<double> d_imu_d;
    DevBuf<float> d_imu_f;
    PinBuf<double> h_imu_d;
    PinBuf<float> h_imu_f;
    std::vector<uint32_t> imu_H;
    std::vector<float> imu_trans;                // [stream][12], valid once finalized
    std::vector<double> scan_time;               // [stream] the sweeps' time stamps (laserOdometryTime of the mapping-side blend); empty: none given
    std::vector<uint64_t> map_imu_upto;          // [stream] mapping-side IMU messages that had arrived at staging time
    hipEvent_t ev_ingest = nullptr;
    uint32_t n_rings = 0;
  };
  RawSlot rawslot[RING];
  std::vector<ImuTracker> imu;                   // one IMU state machine per stream
  // Mapping-side IMU history (LaserMapping's own /imu/data subscription: IMUState2 {stamp, roll, pitch}, 200 deep —
  // BasicLaserMapping.cpp:602-605) per stream, for transformUpdate's roll / pitch blend (:171-200).  Messages are numbered: a sweep is
  // blended with the messages that had arrived when it was STAGED (stage_step_raw), however far the staging runs ahead of its step.
  struct MapImu { double stamp; float roll, pitch; uint64_t seq; };
  std::vector<std::deque<MapImu>> map_imu;
  std::vector<uint64_t> map_imu_seq;
  std::mutex map_imu_mu;                         // (update_imu may come from the staging thread)
  void map_imu_push(uint32_t s, double stamp, float roll, float pitch) {
    std::lock_guard<std::mutex> lk(map_imu_mu);
    if (map_imu[s].size() >= 200) map_imu[s].pop_front();
    map_imu[s].push_back(MapImu{stamp, roll, pitch, map_imu_seq[s]++});
  }
  // the IMU part of transformUpdate (:173-200) for one stream's pose; false: no message had arrived when the sweep was staged
  bool map_imu_blend(uint32_t s, uint64_t seq_limit, double odo_time, float scan_period, float* p6) {
    std::lock_guard<std::mutex> lk(map_imu_mu);
    const std::deque<MapImu>& Hq = map_imu[s];
    size_t n = 0;
    while (n < Hq.size() && Hq[n].seq < seq_limit) n++;
    if (!n) return false;
    size_t i = 0;
    while (i < n - 1 && (odo_time - Hq[i].stamp) + scan_period > 0) i++;
    float roll, pitch;
    if (i == 0 || (odo_time - Hq[i].stamp) + scan_period > 0) {
      roll = Hq[i].roll; pitch = Hq[i].pitch;   // scan time newer than the newest or older than the oldest IMU message
    } else {
      const float ratio = (float)(((Hq[i].stamp - odo_time) - scan_period) / (Hq[i].stamp - Hq[i - 1].stamp));
      const float inv = 1 - ratio;
      roll = Hq[i].roll * inv + Hq[i - 1].roll * ratio;
      pitch = Hq[i].pitch * inv + Hq[i - 1].pitch * ratio;
    }
    p6[0] = (float)(0.998 * p6[0] + 0.002 * pitch);
    p6[2] = (float)(0.998 * p6[2] + 0.002 * roll);
    return true;
  }
  RawBinner binner;
  FeatureExtractor& FX(uint32_t t) { return *fx[streaming ? t % RING : t]; }
  char& LA(uint32_t t) { return launched[streaming ? t % RING : t]; }
  uint32_t n_staged() const { return streaming ? staged_hi.load(std::memory_order_acquire) : (uint32_t)fx.size(); }
  // feature extraction of step t+1 is independent of odometry / registration of step t (in the reference they are
  // different ROS nodes): it runs on its own HIP stream, launched one step ahead, and overlaps with them
  hipStream_t fstream = nullptr;
  bool prefetch = true;
  std::vector<char> launched;
  PinBuf<uint32_t> h_off3[OR];
  hipEvent_t evF[OR][2] = {};
  LazyTimer tmM[2];   // registration: by step parity (the odometry chains keep their own timers, OdomChain)
  float feat_ms[OR] = {};
  int f_hi = -1;                       // features of steps <= f_hi have been launched (calling thread)
  // Steps the odometry chains may run ahead of the registration.  A stream that needs all 25 iterations needs them for five or six
  // sweeps in a row (a chain then takes ~570 us per step against the registration's ~430): on average the chains keep up, and a deeper
  // look-ahead lets them build the lead that such a run eats (depth 2: 15.6 k sweeps/s, 4: 16.6 k, 6: 16.9 k, 8 - 12: 16.4 - 16.6 k;
  // profiles/r04_ab.md).  The streaming ring holds RING = 8 slots: the same six steps.
  int ahead_depth = std::max(1, std::min(diag_env("LOAMX_ODOM_AHEAD") ? atoi(diag_env("LOAMX_ODOM_AHEAD")) : 6, OR - 2));
  int depth() const { return !prefetch ? 0 : (streaming ? std::min(ahead_depth, (int)RING - 2) : ahead_depth); }
  float last_ms[4] = {0, 0, 0, 0};
  std::atomic<bool> timing{false};

  // The odometry chains run on persistent host threads of their own and AHEAD of the registration: odometry O(k) of a stream only
  // depends on its O(k-1) and on the features F(k), never on a registration (separate ROS nodes in the reference) and never on another
  // stream, so a chain goes on to O(k+1) as soon as its O(k) is done, up to depth() steps ahead of the step being registered —
  // registration and odometry are serial chains across steps and the slowest sets the pace, not their sum.  The calling thread launches
  // the features (the only thread that does) and raises the gate's limit; every chain publishes its own position.  Results wait in a
  // ring of OR slots, the re-projected clouds in rotating buffers (OdometryBatch::set_keep), so step k's inputs stay valid while O(k+1)
  // ... O(k+depth) run.  The gate itself — limit, positions, worker threads, the kept error — is odom_lookahead.hpp.
  std::vector<OdomPub> ores[OR];       // [step % OR][stream]; a chain writes its own streams only
  std::unique_ptr<LookAhead> la;
  // a worker's job: one step of one chain, with the chain's trace stamps
  void run_chain_step(OdomChain& c, uint32_t k) {
    const auto tc0 = std::chrono::steady_clock::now();
    c.tr[0] = tr_us(); run_odometry(c, k); c.tr[3] = tr_us();
    c.last_us.store((float)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tc0).count(), std::memory_order_relaxed);
  }
  // calling thread: block until the look-ahead has finished every step it has been allowed to run (its kernels are enqueued then:
  // a device synchronisation afterwards covers them).  Returns the last step whose odometry is published for every stream, -1 if none.
  int drain_lookahead() { return prefetch ? la->drain() : la->done_min(); }
  // calling thread: stop the look-ahead and wait until every worker is idle (LookAhead::park).  restart >= 0: the caller jumped
  void park_odometry(int restart) {
    if (restart >= 0) pre_t = -1;   // (a pre-staged re-projection belongs to the run that is abandoned)
    la->park(restart);
  }

  ~Pipeline() {
    la.reset();   // (joins the workers)
    for (auto& c : chains) {
      for (auto& e : c->ev_tail) if (e) (void)hipEventDestroy(e);
      for (auto& tm : c->tm) tm.destroy();
    }
    fx.clear();
    for (auto& a : evF) for (auto& e : a) if (e) (void)hipEventDestroy(e);
    for (auto& tm : tmM) tm.destroy();
    for (auto& e : ev_stage) if (e) (void)hipEventDestroy(e);
    for (auto& r : rawslot) if (r.ev_ingest) (void)hipEventDestroy(r.ev_ingest);
    for (auto& e : ev_d2h) if (e) (void)hipEventDestroy(e);
    if (ev_reg_done) (void)hipEventDestroy(ev_reg_done);
    if (cstream) { (void)hipStreamSynchronize(cstream); (void)hipStreamDestroy(cstream); }
    if (dstream) { (void)hipStreamSynchronize(dstream); (void)hipStreamDestroy(dstream); }
    if (fstream) (void)hipStreamDestroy(fstream);
  }

  void launch_features(uint32_t t) {
    TraceRange trace_range("loamx:features");
    finalize_raw(t);
    FeatureExtractor& F = FX(t);
    const uint32_t ns = n_streams_, nring = F.total_rings();
    if (streaming) {
      LX_HIP(hipStreamWaitEvent(fstream, ev_stage[t % RING], 0));   // this slot's H2D copies (the tables; the sweeps too unless ROCr carried them)
      if (up_runs[t % RING]) { uplink.wait((int)(t % RING)); up_runs[t % RING] = 0; }   // (issued a step or more ago)
    }
    PinBuf<uint32_t>& hb = h_off3[t % OR];
    hb.reserve(3 * (ns + 1) + nring + 2);
    for (auto& e : evF[t % OR]) if (!e) LX_HIP(hipEventCreate(&e));
    LX_HIP(hipEventRecord(evF[t % OR][0], fstream));
    F.run_async();
    // (the four offset tables lie back to back on the device in the host layout run_odometry() reads: one copy)
    LX_REQUIRE(F.n_offsets() == 3 * (ns + 1) + nring + 1, "internal: offset table layout");
    store_to_pinned_u32(hb.p, F.d_offsets(), F.n_offsets(), fstream);   // (by a kernel: a small device-to-host hipMemcpyAsync blocks its caller for milliseconds now and then — pinned_copy.hpp)
    LX_HIP(hipEventRecord(evF[t % OR][1], fstream));
    LA(t) = 1;
  }

  std::unique_ptr<FeatureExtractor> new_extractor_() {
    auto f = std::make_unique<FeatureExtractor>(device, fstream);
    f->params = feat_params_from(fcfg);
    return f;
  }
  // (upload / first use of the streaming ring) the feature stream, idle, and no extractor left on it
  void feature_stream_() {
    if (!fstream) fstream = create_stream(env_priority("LOAMX_PRIO_FEAT", -1), diag_env("LOAMX_FEAT_CU_STRIDE") ? atoi(diag_env("LOAMX_FEAT_CU_STRIDE")) : 0, /*part=*/1);
    LX_HIP(hipStreamSynchronize(fstream));
    fx.clear();
  }
  // ... and the input starts over with n_slots slots: every chain back to step 0
  void restart_input_(uint32_t n_slots, bool ring) {
    streaming = ring;
    staged_hi = 0;
    last_step = -1;
    launched.assign(n_slots, 0);
    la->reset();
    f_hi = -1;
  }

  void upload(uint32_t n_steps, const loamx_cloud* clouds, const uint32_t* const* ring_size, const uint32_t* n_rings) {
    LX_REQUIRE(n_steps >= 1 && clouds && ring_size && n_rings, "invalid argument");
    LX_HIP(hipSetDevice(device));
    feature_stream_();
    restart_input_(n_steps, false);
    for (uint32_t t = 0; t < n_steps; t++) {
      auto f = new_extractor_();
      f->upload(n_streams_, clouds + (size_t)t * n_streams_, ring_size + (size_t)t * n_streams_, n_rings + (size_t)t * n_streams_);
      fx.push_back(std::move(f));
    }
  }

  // what stage_step*(t) requires before it touches slot t % RING (`entry` names the entry point in the error text)
  void begin_staging_(uint32_t t, const char* entry) {
    LX_HIP(hipSetDevice(device));
    if (!streaming) {   // first use: switch to the ring of slots
      LX_REQUIRE(t == 0, "streaming input starts at step 0");
      feature_stream_();
      for (uint32_t k = 0; k < RING; k++) fx.push_back(new_extractor_());
      if (!cstream) cstream = create_stream(0);
      for (auto& e : ev_stage) if (!e) LX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      restart_input_(RING, true);   // (streaming is set once the ring stands: a failure above leaves the set-up to be done again)
    }
    LX_REQUIRE(t == staged_hi.load(), "steps must be staged in order");
    LX_REQUIRE(t < RING || last_step.load() + (long)RING >= (long)t, std::string(entry) + "(t) needs step(t - 8) to have run: only eight steps can be in flight");
  }
  // ... and its end: step t is published to step() (release) after everything of it is enqueued
  void publish_staged_(uint32_t t) {
    LA(t) = 0;
    staged_hi.store(t + 1, std::memory_order_release);
  }

  // Streaming input: stage ONE step (sweep s of the step = clouds[s]) without blocking; steps arrive in order.  Slot t % RING
  // is free once step t - RING has been registered, which the caller's own order of calls guarantees (stage(t) after step(t - RING)).
  void stage_step(uint32_t t, const loamx_cloud* clouds, const uint32_t* const* ring_size, const uint32_t* n_rings) {
    LX_REQUIRE(clouds && ring_size && n_rings, "invalid argument");
    begin_staging_(t, "stage_step");
    TraceRange trace_range("loamx:pipeline:stage_step");
    if (t > 0) finalize_raw(t - 1);
    rawslot[t % RING].raw = false;
    rawslot[t % RING].finalized = true;
    // The sweeps' block copies go to ROCr directly when source and destination are the runtime's own allocations (hostlink.hpp: a copy
    // stream of the HIP runtime would be a fifth busy HIP stream): the blocks are counted first (the group's size must be known when
    // it begins), then issued; launch_features() waits for the slot's signal on the host — a whole step later.
    static const bool direct = !(diag_env("LOAMX_H2D_DIRECT") && atoi(diag_env("LOAMX_H2D_DIRECT")) == 0);
    const int slot = (int)(t % RING);
    up_runs[slot] = 0;
    uint32_t n_blocks = 0;
    bool all_direct = direct;
    if (direct) {   // (the runs of clouds that lie back to back, as upload_async forms them)
      for (uint32_t s = 0; s < n_streams_ && all_direct;) {
        all_direct = clouds[s].stride == 16 && clouds[s].intensity_offset == 12;
        uint32_t e = s + 1;
        size_t cnt = clouds[s].count;
        while (all_direct && e < n_streams_ && (const char*)clouds[e].data == (const char*)clouds[s].data + sizeof(float4) * cnt) cnt += clouds[e++].count;
        if (cnt) { n_blocks++; all_direct = all_direct && uplink.host_ok(clouds[s].data, sizeof(float4) * cnt); }
        s = e;
      }
    }
    if (all_direct && n_blocks) {
      uplink.begin(slot, n_blocks);
      uint32_t issued = 0;
      try {
        fx[slot]->upload_async(n_streams_, clouds, ring_size, n_rings, cstream, ev_stage[slot], [&](void* dst, const void* src, size_t bytes) {
          if (!uplink.can_copy_h2d(dst, src, bytes)) throw Error(LOAMX_E_HIP, "internal: a staging block is not ROCr's memory after all");
          uplink.copy_h2d(slot, dst, src, bytes);
          issued++;
          return true;
        });
      } catch (...) {
        uplink.abandon(slot);
        throw;
      }
      up_runs[slot] = issued;
    } else {
      fx[slot]->upload_async(n_streams_, clouds, ring_size, n_rings, cstream, ev_stage[slot]);
    }
    publish_staged_(t);
  }

  // Raw input: step t as the sensor delivered it — per stream one revolution of (x, y, z) records in sensor axes and firing
  // order (the /velodyne_points payload, MultiScanRegistration.cpp:160-238).  The payloads cross PCIe as they are and are
  // re-strided, binned into rings and (with IMU data) de-skewed on the device, all on the copy stream; ring sizes and the IMU
  // state the projection loop leaves behind come back through pinned memory and are consumed by finalize_raw().
  void stage_step_raw(uint32_t t, const void* const* raw_xyz, const uint32_t* counts, uint32_t stride, const loamx_multiscan_mapper& mapper,
                      const double* scan_time) {
    LX_REQUIRE(raw_xyz && counts, "invalid argument");
    mapper_check(mapper.lower_bound_deg, mapper.upper_bound_deg, mapper.n_scan_rings, stride);
    stage_records_(t, raw_xyz, counts, stride, mapper_params(mapper.lower_bound_deg, mapper.upper_bound_deg, mapper.n_scan_rings), scan_time);
  }
  // the same with a sensor model (loamx_sensor_model): ring and relTime from the model's sources, the records unpacked on the device
  void stage_step_sensor(uint32_t t, const void* const* records, const uint32_t* counts, uint32_t stride, const loamx_sensor_model& model,
                         const double* scan_time) {
    LX_REQUIRE(records && counts, "invalid argument");
    sensor_model_check(model, stride);
    stage_records_(t, records, counts, stride, sensor_params(model), scan_time);
  }
  void stage_records_(uint32_t t, const void* const* raw_xyz, const uint32_t* counts, uint32_t stride, const SensorParams& model,
                      const double* scan_time) {
    begin_staging_(t, "stage_step_raw");
    TraceRange trace_range("loamx:pipeline:stage_step_raw");
    if (t > 0) finalize_raw(t - 1);   // the IMU state machine advances sweep by sweep: this step's table needs the previous reset
    const uint32_t ns = n_streams_, nr = model.M.n_rings;
    RawSlot& R = rawslot[t % RING];
    R.raw = true;
    R.finalized = false;
    R.n_rings = nr;
    R.count.assign(counts, counts + ns);
    R.off.assign(ns + 1, 0);
    for (uint32_t s = 0; s < ns; s++) {
      LX_REQUIRE(raw_xyz[s] || counts[s] == 0, "NULL raw cloud");
      R.off[s + 1] = R.off[s] + counts[s];
    }
    const uint32_t ntot = R.off[ns];
    R.d_bytes.reserve((size_t)ntot * stride + 16);
    R.d_raw4.reserve((size_t)ntot + 1);
    R.d_binned.reserve((size_t)ntot + 1);
    if (model.ring_src == RING_FIELD) R.d_ring_fld.reserve((size_t)ntot + 1);
    if (model.time_src == TIME_FIELD) R.d_time_fld.reserve((size_t)ntot + 1);
    R.d_ring_cnt.reserve((size_t)ns * nr + 1);
    R.h_ring_cnt.reserve((size_t)ns * nr + 1);
    R.d_last.reserve(ns);
    R.h_last.reserve(ns);
    R.imu_H.assign(ns, 0);
    R.imu_trans.assign((size_t)12 * ns, 0.f);
    if (scan_time) R.scan_time.assign(scan_time, scan_time + ns); else R.scan_time.clear();
    {
      std::lock_guard<std::mutex> lk(map_imu_mu);
      R.map_imu_upto = map_imu_seq;
    }
    if (!R.ev_ingest) LX_HIP(hipEventCreateWithFlags(&R.ev_ingest, hipEventDisableTiming));
    // IMU tables (one per stream with data), staged back to back
    size_t Htot = 0;
    for (uint32_t s = 0; s < ns; s++) { R.imu_H[s] = imu[s].size(); Htot += R.imu_H[s]; }
    if (Htot) {
      R.h_imu_d.reserve(2 * Htot); R.h_imu_f.reserve(9 * Htot); R.d_imu_d.reserve(2 * Htot); R.d_imu_f.reserve(9 * Htot);
    }
    binner.init(cstream);
    LX_HIP(hipMemsetAsync(R.d_last.p, 0, sizeof(ImuLast) * ns, cstream));
    size_t hbase = 0;
    std::vector<ImuTable> tables(ns);
    for (uint32_t s = 0; s < ns; s++) {
      if (scan_time) imu[s].set_scan_time(scan_time[s]);
      const uint32_t H = R.imu_H[s];
      if (H) {
        imu[s].fill_table(R.h_imu_d.p + 2 * hbase, R.h_imu_f.p + 9 * hbase, tables[s]);
        tables[s].dt = R.d_imu_d.p + 2 * hbase;
        tables[s].dstamp = R.d_imu_d.p + 2 * hbase + H;
        tables[s].state = R.d_imu_f.p + 9 * hbase;
        hbase += H;
      }
    }
    if (Htot) {
      LX_HIP(hipMemcpyAsync(R.d_imu_d.p, R.h_imu_d.p, sizeof(double) * 2 * Htot, hipMemcpyHostToDevice, cstream));
      LX_HIP(hipMemcpyAsync(R.d_imu_f.p, R.h_imu_f.p, sizeof(float) * 9 * Htot, hipMemcpyHostToDevice, cstream));
    }
    for (uint32_t s = 0; s < ns; s++) {
      const uint32_t n = counts[s];
      if (n) LX_HIP(hipMemcpyAsync(R.d_bytes.p + (size_t)R.off[s] * stride, raw_xyz[s], (size_t)n * stride, hipMemcpyHostToDevice, cstream));
      SensorParams sp = model;
      sp.ring_fld = model.ring_src == RING_FIELD ? R.d_ring_fld.p + R.off[s] : nullptr;
      sp.time_fld = model.time_src == TIME_FIELD ? R.d_time_fld.p + R.off[s] : nullptr;
      unpack_records(R.d_bytes.p + (size_t)R.off[s] * stride, stride, n, sp, R.d_raw4.p + R.off[s], cstream);
      binner.run(R.d_raw4.p + R.off[s], n, sp, fcfg.scan_period, R.d_binned.p + R.off[s], R.d_ring_cnt.p + (size_t)s * nr,
                 R.imu_H[s] ? &tables[s] : nullptr, R.imu_H[s] ? R.d_last.p + s : nullptr);
    }
    LX_HIP(hipMemcpyAsync(R.h_ring_cnt.p, R.d_ring_cnt.p, sizeof(uint32_t) * ns * nr, hipMemcpyDeviceToHost, cstream));
    LX_HIP(hipMemcpyAsync(R.h_last.p, R.d_last.p, sizeof(ImuLast) * ns, hipMemcpyDeviceToHost, cstream));
    LX_HIP(hipEventRecord(R.ev_ingest, cstream));
    publish_staged_(t);
  }

  // second half of a raw step's staging, once its binning has finished (long before it is needed in steady state): the IMU
  // state machines take over what the projection loops left behind and are reset for the next sweep (processScanlines:
  // reset(scanTime), updateIMUTransform), and the binned clouds are handed to the slot's feature extractor with their ring
  // sizes.  Idempotent; called in step order from stage_step*(t + 1) and launch_features(t), whichever comes first.
  std::mutex raw_mu;   // finalize_raw(t) is reached from the stager (stage_step*(t + 1)) and from the thread that launches the features of t
  void finalize_raw(uint32_t t) {
    if (!streaming) return;
    std::lock_guard<std::mutex> lk(raw_mu);
    RawSlot& R = rawslot[t % RING];
    if (!R.raw || R.finalized) return;
    LX_HIP(hipEventSynchronize(R.ev_ingest));
    const uint32_t ns = n_streams_, nr = R.n_rings;
    std::vector<const uint32_t*> rs(ns);
    std::vector<uint32_t> nrv(ns, nr);
    for (uint32_t s = 0; s < ns; s++) {
      if (R.imu_H[s] && R.h_last.p[s].valid) imu[s].apply_last(R.h_last.p[s]);
      imu[s].begin_sweep();
      memcpy(&R.imu_trans[12 * (size_t)s], imu[s].imu_trans(), sizeof(float) * 12);
      rs[s] = R.h_ring_cnt.p + (size_t)s * nr;
    }
    fx[t % RING]->upload_device(ns, R.d_binned.p, R.off.data(), rs.data(), nrv.data(), cstream, ev_stage[t % RING]);
    R.finalized = true;
  }

  // Registered full-resolution clouds of the step that just ran -> caller memory, asynchronously on a copy stream (the next
  // step's kernels do not wait for it: the registrar alternates between two full-resolution buffers).  Packed float4 records
  // only (a DMA cannot re-stride); out[k] receives the k-th stream that was registered.
  void download_step_async(loamx_cloud* out, uint32_t n_out) {
    LX_REQUIRE(out, "NULL argument");
    LX_REQUIRE(reg.double_buffer_full, "call loamx_pipeline_enable_async_downloads() before the first step");
    LX_HIP(hipSetDevice(device));
    const uint32_t nw = last_full_off.empty() ? 0u : (uint32_t)last_full_off.size() - 1;
    LX_REQUIRE(n_out >= nw, "fewer output descriptors than registered streams");
    const int par = (int)((run_count + 1) & 1);   // the buffer the last run used
    int rc_cap = LOAMX_OK;
    for (uint32_t k = 0; k < nw; k++) {
      check_cloud(&out[k], false);
      LX_REQUIRE(out[k].stride == 16 && out[k].intensity_offset == 12, "asynchronous downloads need packed float4 records (stride 16, intensity at 12)");
    }
    struct Run { char* dst; const char* src; size_t bytes; };
    std::vector<Run> runs;
    for (uint32_t k = 0; k < nw;) {   // destinations that lie back to back (and are filled exactly) share one copy, as in upload_async
      uint32_t e = k;
      size_t cnt = 0;
      char* base = (char*)out[k].data;
      do {
        const uint32_t n = last_full_off[e + 1] - last_full_off[e];
        const uint32_t m = std::min(n, out[e].count);
        if (n > out[e].count) rc_cap = LOAMX_E_CAPACITY;
        out[e].count = n;
        cnt += m;
        e++;
        if (m != n) break;   // a truncated cloud ends the run
      } while (e < nw && (char*)out[e].data == base + sizeof(float4) * cnt);
      if (cnt) runs.push_back(Run{base, (const char*)(reg.d_full_res() + last_full_off[k]), sizeof(float4) * cnt});
      k = e;
    }
    // The copies go to the SDMA engine directly (hostlink.hpp: the HIP runtime may pick its blit kernel for them, which stalls
    // every kernel that writes to host memory meanwhile) when source and destination are ROCr allocations; else through HIP.
    static const bool via_hip = diag_env("LOAMX_D2H_HIP") != nullptr;   // diagnostic: always hipMemcpyAsync
    bool direct = !via_hip && !runs.empty();
    for (const Run& r : runs) direct = direct && hostlink.can_copy(r.dst, r.src, r.bytes);
    wait_download(par);   // (a caller that downloads the same step twice)
    if (direct) {
      if (ev_reg_done) LX_HIP(hipEventSynchronize(ev_reg_done));   // step() has returned: the registration is complete and its clouds are visible
      try {
        hostlink.begin(par, (uint32_t)runs.size());
        for (const Run& r : runs) hostlink.copy_d2h(par, r.dst, r.src, r.bytes);
        downloads_direct++;
      } catch (const Error&) {   // ROCr refused a copy: the slot has been freed (HostLinkDma::abandon); the whole group goes through HIP
        direct = false;
      }
    }
    if (!direct && !runs.empty()) {
      if (!dstream) dstream = create_stream(0);
      if (!ev_d2h[par]) LX_HIP(hipEventCreateWithFlags(&ev_d2h[par], hipEventDisableTiming));
      LX_HIP(hipStreamWaitEvent(dstream, ev_reg_done, 0));
      for (const Run& r : runs) LX_HIP(hipMemcpyAsync(r.dst, r.src, r.bytes, hipMemcpyDeviceToHost, dstream));
      LX_HIP(hipEventRecord(ev_d2h[par], dstream));
      d2h_pending[par] = true;
      downloads_hip++;
    }
    if (rc_cap != LOAMX_OK) throw Error(LOAMX_E_CAPACITY, "an output cloud is smaller than the registered cloud (count fields hold the needed sizes)");
  }
  void wait_download(int par) {
    hostlink.wait(par);
    if (d2h_pending[par]) { LX_HIP(hipEventSynchronize(ev_d2h[par])); d2h_pending[par] = false; }
  }
  void wait_downloads() {
    for (int par = 0; par < 2; par++) wait_download(par);
  }
  uint64_t run_count = 0;   // registrations run so far (parity = which full-resolution buffer)

  // odometry of staged step t for the streams of one chain (needs the step's features, launched by the calling thread); results go to
  // ores[t % OR]
  void run_odometry(OdomChain& c, uint32_t t) {
    const uint32_t ns = n_streams_, ng = c.s1 - c.s0;
    FeatureExtractor& F = FX(t);
    LX_REQUIRE(LA(t), "internal: odometry of a step whose features were not launched");
    OdometryBatch& odom = *c.ob;
    uint32_t* hb = h_off3[t % OR].p;
    uint32_t* ho[3] = {hb, hb + (ns + 1), hb + 2 * (ns + 1)};
    uint32_t* hlf = hb + 3 * (ns + 1);
    wait_event(evF[t % OR][1]);
    F.check_finite_input();   // (LOAMX_E_INVALID out of step(): a staged sweep with NaN / Inf coordinates)
    c.tr[1] = tr_us();
    const bool timed = timing.load(std::memory_order_relaxed);   // latched: the caller flips the flag while this chain runs steps ahead
    if (timed && c.s0 == 0) LX_HIP(hipEventElapsedTime(&feat_ms[t % OR], evF[t % OR][0], evF[t % OR][1]));
    std::vector<OdomInput> in(ng);
    std::vector<int> rc(ng, 0);
    for (uint32_t s = c.s0; s < c.s1; s++) {
      const uint32_t la = hlf[F.ring_base(s)], lb = hlf[F.ring_base(s + 1)];
      in[s - c.s0] = OdomInput{F.d_feat(0) + ho[0][s], ho[0][s + 1] - ho[0][s], F.d_feat(1) + ho[1][s], ho[1][s + 1] - ho[1][s],
                               F.d_feat(2) + ho[2][s], ho[2][s + 1] - ho[2][s], F.d_less_flat() + la, lb - la};
    }
    const int slot = (int)(t % OR);
    if (timed) c.tm[slot].start(odom.stream());   // this chain's own event pair for this step: both ends are recorded by this thread in this call
    if (streaming && rawslot[t % RING].raw)   // imuTrans of this sweep (ScanRegistration publishes it with the clouds; LaserOdometry.cpp:239-248)
      for (uint32_t s = c.s0; s < c.s1; s++) odom.update_imu(s - c.s0, &rawslot[t % RING].imu_trans[12 * (size_t)s]);
    odom.process(in.data(), rc.data(), true);   // returns once the poses are known; clouds ready at odom.tail_event()
    c.tr[2] = tr_us();
    if (!c.ev_tail[slot]) LX_HIP(hipEventCreateWithFlags(&c.ev_tail[slot], hipEventDisableTiming));
    LX_HIP(hipEventRecord(c.ev_tail[slot], odom.stream()));   // behind the tail that process() enqueued
    if (timed) c.tm[slot].stop(odom.stream());   // the chain of step t = everything process() enqueued, tail included
    for (auto& tm : c.tm)   // (the elapsed time of an older step is taken once its events have completed: measuring never waits)
      if (tm.resolve()) c.ms.store(tm.ms, std::memory_order_relaxed);
    for (uint32_t s = c.s0; s < c.s1; s++) {
      const uint32_t l = s - c.s0;
      OdomStream& O = odom.stream_state(l);
      OdomPub& N = ores[slot][s];
      N.transform = O.transform;
      N.transform_sum = O.transform_sum;
      N.stats = O.stats;
      N.rc = rc[l];
      N.last_corner = odom.d_last_corner(l); N.n_last_corner = O.n_last_corner;
      N.last_surf = odom.d_last_surf(l); N.n_last_surf = O.n_last_surf;
      N.to_end = odom.to_end_params(l, true);
    }
  }
  // Head of M(t+1) that does not depend on M(t): transformToEnd of the next step's full-resolution clouds (LaserOdometry.cpp:326) into
  // the registrar's OTHER staging buffer, enqueued behind M(t)'s first Gauss-Newton launches while the host waits for them — as soon
  // as the odometry of t+1 is known (it runs ahead).  step(t+1) then finds its clouds re-projected: one copy + one 12-25 us kernel less
  // between two steps' registrations.  (The host waits for M(t) at an event recorded in front of this work: Registrar::run_iterations.)
  int pre_t = -1;   // the step whose full-resolution clouds have been pre-staged
  void prestage_gather(int tn, int last_staged, hipStream_t s_) {
    static const bool off = !(diag_env("LOAMX_PRESTAGE") && atoi(diag_env("LOAMX_PRESTAGE")) != 0);   // measured: no gain (15.44 k with, 15.51 k without; profiles/r04_ab.md) — the step is not bound by this copy + kernel; opt-in
    if (off || !prefetch || pre_t == tn || tn > last_staged || tn < 1) return;
    const uint32_t ns = n_streams_;
    if (la->done_min() < tn) return;
    FeatureExtractor& F = FX((uint32_t)tn);
    std::vector<const float4*> fsrc;
    std::vector<uint32_t> nfr;
    std::vector<ToEndParams> tep;
    for (uint32_t s = 0; s < ns; s++) {
      const OdomPub& N = ores[tn % OR][s];
      if (N.rc != LOAMX_OK) continue;
      fsrc.push_back(F.d_cloud() + F.point_base(s));
      nfr.push_back(F.point_base(s + 1) - F.point_base(s));
      tep.push_back(N.to_end);
    }
    const uint32_t nw = (uint32_t)fsrc.size();
    if (!nw) return;
    const int par = (int)(run_count & 1);   // the buffer the NEXT run uses: its last download (two runs ago) must have finished
    hostlink.wait(par);
    if (d2h_pending[par]) { LX_HIP(hipStreamWaitEvent(s_, ev_d2h[par], 0)); d2h_pending[par] = false; }
    float4* dst = reg.stage_full_next(nw, nfr.data());
    if (!dst) return;
    std::vector<uint32_t> foff(nw + 1, 0);
    for (uint32_t k = 0; k < nw; k++) foff[k + 1] = foff[k] + nfr[k];
    chains[0]->ob->to_end_gather(dst, foff.data(), fsrc.data(), tep.data(), nw, s_);
    pre_t = tn;
  }

  // Software pipeline over consecutive steps (the stages are separate ROS nodes in the reference, so nothing in a later
  // stage of step t feeds an earlier stage of step t+1):
  //   registration M(t) on the registrar's stream  ||  odometry O(t+1) on the odometry stream  ||  features F(t+2)
  // step(t) returns when M(t) is complete; O(t+1) / F(t+2) are look-ahead whose results are kept for the next call.
  // host-side timeline of one step (LOAMX_PIPE_TRACE=1): microseconds since step() entry
  bool trace = getenv("LOAMX_PIPE_TRACE") != nullptr;
  std::chrono::steady_clock::time_point tr0, tr_exit = std::chrono::steady_clock::now();
  double tr_us() const { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tr0).count(); }

  // what the stages of one step() share
  struct Step {
    uint32_t t = 0;
    int ti = 0, last_staged = -1;
    LookaheadWindow w;               // how far features / odometry are released at each point of this step (odom_lookahead.hpp)
    bool late_pending = false;       // the late release is still to come
    hipStream_t s_ = nullptr;        // the registrar's stream
    std::vector<uint32_t> who;       // the streams that are registered (a stream's first sweep only initialises the odometry), in
    std::vector<const float4*> cl, sl, fsrc;   // order; everything below is indexed like it
    std::vector<uint32_t> ncl, nsl, nfr;
    std::vector<float> guess;
    std::vector<ToEndParams> to_end;
    uint32_t nw = 0;                 // = who.size()
    float f_ms = 0.f;
    double gap_us = 0, tr[5] = {0, 0, 0, 0, 0};   // trace marks: M-start, M-enqueued, M-downloaded, O-joined, download-wait
  };
  // features of the steps up to k (launched by the calling thread only, in step order)
  void launch_features_upto(int k) {
    while (f_hi < k) { ++f_hi; if (!LA((uint32_t)f_hi)) launch_features((uint32_t)f_hi); }
  }

  // 1. this step's odometry: published by the look-ahead (the normal case), or run now
  void join_odometry_(Step& S) {
    const uint32_t t = S.t;
    const int ti = S.ti;
    if (la->jumped(ti)) {   // for some chain this is neither a finished step nor its next one: the caller jumped, the chains restart here
      park_odometry(ti);
      f_hi = ti - 1;
    }
    LX_REQUIRE(ti + (OR - 2) >= la->done_max(), "this step's odometry results have been overwritten: steps run in order");
    if (ti > la->done_min()) {
      launch_features_upto(S.w.feat_join);
      if (prefetch) {
        la->allow(S.w.odom_join);
        la->wait(ti);
      } else {
        if (la->limit() >= 0) park_odometry(-1);   // the look-ahead was switched off: the chains go on here
        for (uint32_t g = 0; g < n_groups; g++)
          if (ti > la->done(g)) { run_odometry(*chains[g], t); la->ran_inline(g, ti); }
      }
    }
    LA(t) = 0;   // every chain has consumed the step's features (a restart at this step extracts them again: their offsets' slot is reused by step t + 3)
    for (uint32_t s = 0; s < n_streams_; s++) st[s].cur = ores[t % OR][s];
    S.f_ms = feat_ms[t % OR];
    // the re-projected "last" clouds of THIS sweep are produced at the tails of the odometry chains
    for (auto& c : chains) LX_HIP(hipStreamWaitEvent(S.s_, c->ev_tail[t % OR], 0));
  }
  // 2. look-ahead while M(t) runs: the odometry chains may go on now, and further once M(t) is enqueued (release_late_).  In steady
  // state this call and the one in join_odometry_ find nothing to do — the previous step's late release went that far — and the one
  // new step of features / odometry is released by release_late_, off M(t)'s critical path
  void release_lookahead_(Step& S) {
    launch_features_upto(S.w.feat_reg);
    la->allow(S.w.odom_reg);
    S.late_pending = S.w.late;
  }
  // ... the late part: reached from the registration's first host wait (reg.on_first_wait) and again behind run_async(); once in effect
  void release_late_(Step& S) {
    if (!S.late_pending) return;
    S.late_pending = false;
    launch_features_upto(S.w.feat_late);
    la->allow(S.w.odom_late);
  }
  // 3. what the registration of the registered streams reads: the odometry's clouds, the initial guesses, the full-resolution sources
  void gather_inputs_(Step& S) {
    S.tr[0] = tr_us();
    if (timing) tmM[S.t & 1].start(S.s_);
    const uint32_t ns = n_streams_;
    FeatureExtractor& F = FX(S.t);
    S.cl.resize(ns); S.sl.resize(ns); S.fsrc.resize(ns);
    S.ncl.resize(ns); S.nsl.resize(ns); S.nfr.resize(ns);
    for (uint32_t s = 0; s < ns; s++) {
      PipeStreamState& P = st[s];
      if (P.cur.rc != LOAMX_OK) continue;   // a stream's first sweep only initialises the odometry
      transform_associate_to_map(P.cur.transform_sum, P.bef, P.aft, P.incre, P.tobe);
      float g[6];
      P.tobe.get(g);
      S.guess.insert(S.guess.end(), g, g + 6);
      const uint32_t k = (uint32_t)S.who.size();
      S.cl[k] = P.cur.last_corner; S.ncl[k] = P.cur.n_last_corner;
      S.sl[k] = P.cur.last_surf; S.nsl[k] = P.cur.n_last_surf;
      S.fsrc[k] = F.d_cloud() + F.point_base(s);
      S.nfr[k] = F.point_base(s + 1) - F.point_base(s);
      S.to_end.push_back(P.cur.to_end);
      S.who.push_back(s);
    }
    S.nw = (uint32_t)S.who.size();
  }
  // 4. the full-resolution clouds are re-projected to the sweep end before they are registered (LaserOdometry.cpp:326): one fused
  // kernel writes them straight into the registrar's staging area — unless the previous step pre-staged them (prestage_gather)
  void stage_full_res_(Step& S) {
    if (!S.nw) { last_full_off.clear(); last_who.clear(); return; }
    const uint32_t nw = S.nw;
    std::vector<uint32_t> foff(nw + 1, 0);
    for (uint32_t k = 0; k < nw; k++) foff[k + 1] = foff[k] + S.nfr[k];
    const bool adopted = pre_t == S.ti && reg.adopt_full_next(nw, S.nfr.data());   // re-projected already, behind the previous step's first iterations
    pre_t = -1;
    if (!adopted) {
      if (reg.double_buffer_full) {   // this run reuses the buffer of the run before last: its download must have finished
        const int par = (int)(run_count & 1);
        const double tw0 = trace ? tr_us() : 0.0;
        hostlink.wait(par);   // (two steps old: landed long ago)
        if (trace) S.tr[4] = tr_us() - tw0;
        if (d2h_pending[par]) { LX_HIP(hipStreamWaitEvent(S.s_, ev_d2h[par], 0)); d2h_pending[par] = false; }
      }
      float4* full_dst = reg.stage_full(nw, S.nfr.data());
      chains[0]->ob->to_end_gather(full_dst, foff.data(), S.fsrc.data(), S.to_end.data(), nw, S.s_);
    }
    last_full_off = foff;
    last_who = S.who;
    run_count++;
  }
  // 5. registration against the frozen sub-map: enqueue everything for M(t)
  void enqueue_registration_(Step& S) {
    if (!S.nw) return;
    const uint32_t nw = S.nw;
    const RawSlot& R = rawslot[S.t % RING];
    reg.upload_device(nw, S.cl.data(), S.ncl.data(), S.sl.data(), S.nsl.data(), nullptr, nullptr, S.guess.data());
    // transformUpdate's IMU blend (BasicLaserMapping.cpp:171-200) changes transformTobeMapped BEFORE the full-resolution cloud is
    // registered (:235-240): a step with mapping-side IMU data for any of its streams registers its clouds after the blend
    bool blend = false;
    static const bool no_blend = diag_env("LOAMX_NO_MAP_IMU_BLEND") != nullptr;   // (tests: what the poses would be without the blend)
    if (!no_blend && streaming && R.raw && !R.scan_time.empty())
      for (uint32_t k = 0; k < nw; k++) blend = blend || R.map_imu_upto[S.who[k]] > 0;
    reg.defer_full = blend;
    reg.on_first_wait = [&]() { release_late_(S); prestage_gather(S.ti + 1, S.last_staged, S.s_); };
    reg.run_async();
    reg.on_first_wait = nullptr;
    if (blend) {
      std::vector<float> p6(6 * (size_t)nw);
      reg.download(p6.data(), nullptr);
      if (reg.submap_sufficient())   // (transformUpdate is only reached when the optimisation ran, :628-629)
        for (uint32_t k = 0; k < nw; k++)
          (void)map_imu_blend(S.who[k], R.map_imu_upto[S.who[k]], R.scan_time[S.who[k]], fcfg.scan_period, &p6[6 * (size_t)k]);
      reg.finish_with_poses(p6.data());
      reg.defer_full = false;
    }
    if (reg.double_buffer_full) {
      if (!ev_reg_done) LX_HIP(hipEventCreateWithFlags(&ev_reg_done, hipEventDisableTiming));
      LX_HIP(hipEventRecord(ev_reg_done, S.s_));
    }
  }
  // 6. what may follow M(t)'s launches: the late release and the next step's pre-staging (no-ops when the first wait's callback did them)
  void release_behind_registration_(Step& S) {
    release_late_(S);
    if (S.nw) prestage_gather(S.ti + 1, S.last_staged, S.s_);
    if (timing) tmM[S.t & 1].stop(S.s_);
    S.tr[1] = tr_us();
  }
  // 7. finish M(t): poses and statistics of the registered streams
  int collect_(Step& S) {
    int ret = LOAMX_SKIPPED;
    if (S.nw) {
      std::vector<float> poses(6 * (size_t)S.nw);
      std::vector<SweepStats> ss(S.nw);
      reg.download(poses.data(), nullptr);
      reg.download_stats(ss.data());
      for (uint32_t k = 0; k < S.nw; k++) {
        PipeStreamState& P = st[S.who[k]];
        P.map_stats = ss[k];
        P.mapped = true;
        if (reg.submap_sufficient()) {   // transformUpdate (BasicLaserMapping.cpp:171-203, :628-629)
          P.tobe.set(&poses[6 * (size_t)k]);
          P.bef = P.cur.transform_sum;
          P.aft = P.tobe;
        }
      }
      ret = LOAMX_OK;
    }
    S.tr[2] = tr_us();
    return ret;
  }
  // 8. the step has run: trace line (LOAMX_PIPE_TRACE) and stage times
  void finish_step_(Step& S) {
    const uint32_t t = S.t;
    S.tr[3] = tr_us();
    last_step = (long)t;
    tr_exit = std::chrono::steady_clock::now();
    if (trace) {
      fprintf(stderr, "[pipe t=%u] caller gap %.0f | M-start %.0f  M-enqueued %.0f  M-downloaded %.0f  O-joined %.0f  (download-wait %.0f) |", t, S.gap_us, S.tr[0], S.tr[1], S.tr[2], S.tr[3], S.tr[4]);
      for (uint32_t g = 0; g < n_groups; g++) {   // (each chain's most recent pass, whichever step that was: start, features ready, process() returned, end)
        const OdomChain& c = *chains[g];
        fprintf(stderr, " O[%u-%u): %.0f %.0f %.0f %.0f done %d pass %.0f us |", c.s0, c.s1, c.tr[0], c.tr[1], c.tr[2], c.tr[3], la->done(g), (double)c.last_us.load());
      }
      fprintf(stderr, " f_hi %d o_limit %d staged %u", f_hi, la->limit(), n_staged());
      fprintf(stderr, "\n");
    }
    if (timing) {
      for (auto& x : tmM) x.resolve();
      last_ms[0] = S.f_ms;             // on the feature stream (overlapped)
      {   // the odometry chains (overlapped with the registrations): the longest chain's most recent timed pass
        float m = 0.f;
        for (auto& c : chains) m = std::max(m, c->ms.load(std::memory_order_relaxed));
        last_ms[1] = m;
      }
      last_ms[2] = tmM[t & 1].pending ? tmM[(t + 1) & 1].ms : tmM[t & 1].ms;   // the previous step's while this one is in flight
      last_ms[3] = last_ms[2];
    }
  }

  int step(uint32_t t) {
    TraceRange trace_range("loamx:pipeline:step");
    LX_REQUIRE(t < n_staged(), "step index beyond the staged sweeps");
    LX_REQUIRE(!streaming || t + RING >= staged_hi.load(), "this step's slot has been re-staged already");   // (slot t % RING is rewritten by staging step t + RING)
    Step S;
    const auto t_entry = std::chrono::steady_clock::now();
    S.gap_us = std::chrono::duration<double, std::micro>(t_entry - tr_exit).count();   // the caller's time between two steps
    tr0 = t_entry;
    LX_HIP(hipSetDevice(device));
    S.t = t;
    S.ti = (int)t;
    S.s_ = reg.stream();
    S.last_staged = (int)n_staged() - 1;
    S.w = lookahead_window(S.ti, depth(), S.last_staged, prefetch);
    join_odometry_(S);
    release_lookahead_(S);
    gather_inputs_(S);
    stage_full_res_(S);
    enqueue_registration_(S);
    release_behind_registration_(S);
    const int ret = collect_(S);
    finish_step_(S);
    return ret;
  }
};

}  // namespace loamx

using namespace loamx;

struct loamx_pipeline {
  Pipeline p;
  loamx_pipeline(const loamx_scanreg_config& f, const loamx_odom_config& o, const loamx_map_config& m, uint32_t n) : p(f, o, m, n) {}
};

extern "C" {

loamx_pipeline* loamx_pipeline_create(const loamx_scanreg_config* fcfg, const loamx_odom_config* ocfg, const loamx_map_config* mcfg,
                                      uint32_t n_streams) {
  loamx_pipeline* h = nullptr;
  guard([&]() {
    loamx_scanreg_config f;
    loamx_odom_config o;
    loamx_map_config m;
    if (fcfg) f = *fcfg; else loamx_scanreg_default_config(&f);
    if (ocfg) o = *ocfg; else loamx_odom_default_config(&o);
    if (mcfg) m = *mcfg; else loamx_map_default_config(&m);
    LX_REQUIRE(n_streams >= 1 && n_streams <= 1024, "n_streams must be in [1, 1024]");
    LX_REQUIRE(f.device == m.device && o.device == m.device, "all three configurations must name the same device");
    LX_REQUIRE(f.max_corner_less_sharp == 0 || f.max_corner_less_sharp >= f.max_corner_sharp, "max_corner_less_sharp must be >= max_corner_sharp");
    h = new loamx_pipeline(f, o, m, n_streams);
    return LOAMX_OK;
  });
  return h;
}
void loamx_pipeline_destroy(loamx_pipeline* h) { delete h; }

int loamx_pipeline_set_frozen(loamx_pipeline* h, const loamx_cloud* corner_map, const loamx_cloud* surf_map) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->p.reg.set_submap_host(corner_map, surf_map); return LOAMX_OK; });
}
int loamx_pipeline_set_frozen_device(loamx_pipeline* h, const void* d_corner, uint32_t nc, const void* d_surf, uint32_t ns) {
  return guard([&]() {
    LX_REQUIRE(h && (d_corner || !nc) && (d_surf || !ns), "NULL argument");
    h->p.reg.set_submap_device((const float4*)d_corner, nc, (const float4*)d_surf, ns);
    return LOAMX_OK;
  });
}
int loamx_pipeline_stage_frozen_device(loamx_pipeline* h, const void* d_corner, uint32_t nc, const void* d_surf, uint32_t ns, void* wait_event) {
  return guard([&]() {
    LX_REQUIRE(h && (d_corner || !nc) && (d_surf || !ns), "NULL argument");
    h->p.reg.stage_submap_device((const float4*)d_corner, nc, (const float4*)d_surf, ns, (hipEvent_t)wait_event);
    return LOAMX_OK;
  });
}
int loamx_pipeline_stage_frozen(loamx_pipeline* h, const loamx_cloud* corner_map, const loamx_cloud* surf_map) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    h->p.reg.stage_submap_host(corner_map, surf_map);
    return LOAMX_OK;
  });
}
int loamx_pipeline_swap_frozen(loamx_pipeline* h) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    if (!h->p.reg.submap_staged()) return (int)LOAMX_SKIPPED;
    h->p.reg.swap_submap();
    return (int)LOAMX_OK;
  });
}
int loamx_pipeline_set_state(loamx_pipeline* h, uint32_t stream, const float* transform, const float* transform_sum, const float* bef,
                             const float* aft) {
  return guard([&]() {
    LX_REQUIRE(h && stream < h->p.n_streams_, "invalid stream");
    h->p.park_odometry(-1);   // the odometry chains stop where they are; the sweeps they have not processed yet start from the new state
    if (transform) h->p.OB(stream).stream_state(h->p.LS(stream)).transform.set(transform);
    if (transform_sum) h->p.OB(stream).stream_state(h->p.LS(stream)).transform_sum.set(transform_sum);
    if (bef) h->p.st[stream].bef.set(bef);
    if (aft) h->p.st[stream].aft.set(aft);
    return LOAMX_OK;
  });
}
int loamx_pipeline_upload(loamx_pipeline* h, uint32_t n_steps, const loamx_cloud* clouds, const uint32_t* const* ring_size,
                          const uint32_t* n_rings) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->p.upload(n_steps, clouds, ring_size, n_rings); return LOAMX_OK; });
}
int loamx_pipeline_stage_step(loamx_pipeline* h, uint32_t step, const loamx_cloud* clouds, const uint32_t* const* ring_size, const uint32_t* n_rings) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->p.stage_step(step, clouds, ring_size, n_rings); return LOAMX_OK; });
}
int loamx_pipeline_stage_step_raw(loamx_pipeline* h, uint32_t step, const void* const* raw_xyz, const uint32_t* counts, uint32_t stride,
                                  const loamx_multiscan_mapper* mapper, const double* scan_time_sec) {
  return guard([&]() {
    LX_REQUIRE(h && mapper, "NULL argument");
    h->p.stage_step_raw(step, raw_xyz, counts, stride, *mapper, scan_time_sec);
    return LOAMX_OK;
  });
}
int loamx_pipeline_stage_step_sensor(loamx_pipeline* h, uint32_t step, const void* const* records, const uint32_t* counts, uint32_t stride,
                                     const loamx_sensor_model* m, const double* scan_time_sec) {
  return guard([&]() {
    LX_REQUIRE(h && m, "NULL argument");
    h->p.stage_step_sensor(step, records, counts, stride, *m, scan_time_sec);
    return LOAMX_OK;
  });
}
int loamx_pipeline_update_imu(loamx_pipeline* h, uint32_t stream, double stamp_sec, float roll, float pitch, float yaw, const float acc_xyz[3]) {
  return guard([&]() {
    LX_REQUIRE(h && acc_xyz && stream < h->p.n_streams_, "invalid argument");
    h->p.imu[stream].update(stamp_sec, roll, pitch, yaw, acc_xyz);
    h->p.map_imu_push(stream, stamp_sec, roll, pitch);   // (the same topic feeds LaserMapping's history in the reference's node graph)
    return LOAMX_OK;
  });
}
int loamx_pipeline_enable_async_downloads(loamx_pipeline* h) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->p.reg.double_buffer_full = true; return LOAMX_OK; });
}
int loamx_pipeline_download_step_async(loamx_pipeline* h, loamx_cloud* out, uint32_t n_out) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->p.download_step_async(out, n_out); return LOAMX_OK; });
}
int loamx_pipeline_download_counts(loamx_pipeline* h, uint64_t counts[2]) {
  return guard([&]() {
    LX_REQUIRE(h && counts, "NULL argument");
    counts[0] = h->p.downloads_direct;
    counts[1] = h->p.downloads_hip;
    return LOAMX_OK;
  });
}
int loamx_pipeline_wait_downloads(loamx_pipeline* h) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); h->p.wait_downloads(); return LOAMX_OK; });
}
int loamx_pipeline_step(loamx_pipeline* h, uint32_t step) {
  return guard([&]() { LX_REQUIRE(h, "NULL handle"); return h->p.step(step); });
}
int loamx_pipeline_get(loamx_pipeline* h, uint32_t stream, float* transform, float* transform_sum, float* aft, int* stats8) {
  return guard([&]() {
    LX_REQUIRE(h && stream < h->p.n_streams_, "invalid stream");
    PipeStreamState& P = h->p.st[stream];
    const OdomPub& O = P.cur;   // the sweep that was registered last (odometry itself may already be one sweep ahead)
    if (transform) O.transform.get(transform);
    if (transform_sum) O.transform_sum.get(transform_sum);
    if (aft) P.aft.get(aft);
    if (stats8) {
      stats8[0] = O.stats.iterations; stats8[1] = O.stats.sel; stats8[2] = P.map_stats.iterations; stats8[3] = P.map_stats.sel;
      stats8[4] = P.map_stats.corner_q; stats8[5] = P.map_stats.surf_q; stats8[6] = P.map_stats.degenerate; stats8[7] = P.mapped ? 1 : 0;
    }
    return LOAMX_OK;
  });
}
int loamx_pipeline_download_full_res(loamx_pipeline* h, uint32_t slot, loamx_cloud* out) {
  return guard([&]() { LX_REQUIRE(h && out, "NULL argument"); return h->p.reg.download_full_res(slot, out); });
}
int loamx_pipeline_download_last_clouds(loamx_pipeline* h, uint32_t stream, loamx_cloud* last_corner, loamx_cloud* last_surf) {
  return guard([&]() {
    LX_REQUIRE(h && last_corner && last_surf, "NULL argument");
    LX_REQUIRE(stream < h->p.n_streams_, "stream index out of range");
    LX_REQUIRE(h->p.last_step.load() >= 0, "no step has run");
    check_cloud(last_corner, false);
    check_cloud(last_surf, false);
    LX_HIP(hipSetDevice(h->p.device));
    // (produced on the odometry chain's stream, behind the event the step's registration waited for: complete since step() returned;
    // their buffer is rewritten only once the chain has gone on for more steps than the look-ahead allows before the next step())
    const OdomPub& N = h->p.st[stream].cur;
    std::vector<float4> tmp(std::max(N.n_last_corner, N.n_last_surf));
    if (N.n_last_corner) LX_HIP(hipMemcpy(tmp.data(), N.last_corner, sizeof(float4) * N.n_last_corner, hipMemcpyDeviceToHost));
    const int rc = unpack_cloud(tmp.data(), N.n_last_corner, last_corner);
    if (N.n_last_surf) LX_HIP(hipMemcpy(tmp.data(), N.last_surf, sizeof(float4) * N.n_last_surf, hipMemcpyDeviceToHost));
    const int rs = unpack_cloud(tmp.data(), N.n_last_surf, last_surf);
    return rc != LOAMX_OK ? rc : rs;
  });
}
int loamx_pipeline_set_lookahead(loamx_pipeline* h, int on) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    if (!on && h->p.prefetch) h->p.park_odometry(-1);   // (every worker finishes the step it is in; the chains continue from there)
    h->p.prefetch = on != 0;
    return LOAMX_OK;
  });
}
int loamx_pipeline_drain_lookahead(loamx_pipeline* h, int* last_odometry_step) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    const int done = h->p.drain_lookahead();
    if (last_odometry_step) *last_odometry_step = done;
    return LOAMX_OK;
  });
}
int loamx_pipeline_set_timing(loamx_pipeline* h, int on) {
  return guard([&]() {
    LX_REQUIRE(h, "NULL handle");
    h->p.timing = on != 0;
    h->p.reg.set_timing(on != 0, on != 2);
    for (auto& c : h->p.chains) c->ob->set_launch_timing(on != 0 && on != 2);
    return LOAMX_OK;
  });
}
int loamx_pipeline_get_odom_launch_timing(loamx_pipeline* h, double ms4[4], uint64_t counts7[7]) {
  return guard([&]() {
    LX_REQUIRE(h && ms4 && counts7, "NULL argument");
    for (int k = 0; k < 4; k++) ms4[k] = 0.0;
    for (int k = 0; k < 7; k++) counts7[k] = 0;
    for (auto& c : h->p.chains) {
      const OdometryBatch::LaunchTotals t = c->ob->launch_totals();
      ms4[0] += t.lm_ms; ms4[1] += t.lm_noop_ms; ms4[2] += t.corr_ms; ms4[3] += t.corr_noop_ms;
      counts7[0] += t.lm_launches; counts7[1] += t.lm_noop_launches; counts7[2] += t.lm_iterations; counts7[3] += t.corr_launches;
      counts7[4] += t.corr_noop_launches; counts7[5] += t.lm_bytes; counts7[6] += t.corr_features;
    }
    return LOAMX_OK;
  });
}
int loamx_pipeline_get_timing(loamx_pipeline* h, float stage_ms[4], float reg_ms[4], uint64_t counts[4]) {
  return guard([&]() {
    LX_REQUIRE(h && stage_ms && reg_ms && counts, "NULL argument");
    for (int k = 0; k < 4; k++) stage_ms[k] = h->p.last_ms[k];
    h->p.reg.get_timing(reg_ms, counts);
    return LOAMX_OK;
  });
}
int loamx_pipeline_lookahead_depth(loamx_pipeline* h) { return h ? h->p.depth() : 0; }
void* loamx_pipeline_stream(loamx_pipeline* h) { return h ? (void*)h->p.reg.stream() : nullptr; }

}  // extern "C"

// the registered cloud of the slot-th stream registered in the last step, for the dense map (cloud_stage.hpp): it lies in the registrar's
// full-resolution buffer until the registrar's stream passes the next step's gather, so an add enqueued on that stream reads it in time
void loamx_pipeline_dense_source(loamx_pipeline* h, uint32_t slot, loamx::DenseSource& out) {
  LX_REQUIRE(h, "NULL pipeline");
  Pipeline& P = h->p;
  out = loamx::DenseSource{};
  out.stream = P.reg.stream();
  out.device = P.device;
  const uint32_t nw = P.last_full_off.empty() ? 0u : (uint32_t)P.last_full_off.size() - 1;
  if (!nw) return;
  LX_REQUIRE(slot < nw, "slot beyond the streams registered in the last step");
  out.pts = P.reg.d_full_res() + P.last_full_off[slot];
  out.n = P.last_full_off[slot + 1] - P.last_full_off[slot];
  const HTwist& aft = P.st[P.last_who[slot]].aft;
  out.origin[0] = aft.pos.x; out.origin[1] = aft.pos.y; out.origin[2] = aft.pos.z;
  out.has_cloud = true;
}
