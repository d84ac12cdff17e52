// kb_engine_int.hpp — what the translation units of the engine's host side share (round 6: kb_engine.cpp was one 2 400-line file): the engine
// object, its device / pinned buffers, a round's context, the declaration of the action's host state (ActionRun) and of the helpers.
//   kb_engine.cpp   create / destroy, buffers, timers, the closing reduction, the getters
//   kb_load.cpp     kb_session_load (host session, uploads, water-fill launch) as named steps, kb_session_reset, the one list of the state it restores
//   kb_rounds.cpp   a round's three host steps, chaining and overlap, ActionRun (the window planner, the feasibility probe, absorbing a round's
//                   answer), run_action (allocate / backfill), the round-granular API of the task-row split
//   kb_evict.cpp    the bridge between the evict machine (kb_preempt.cpp) and the device lists: kb_run_preempt / kb_run_reclaim
//   kb_matrix.cpp   kb_eval_matrix / kb_argmax_rows / kb_bench_matrix (the materialised matrix)
//
// Round structure: DESIGN.md §4 (kb_engine.cpp restates it at its top).
#pragma once
#include <hip/hip_runtime.h>

#include <sched.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/kb_engine.h"
#include "kb_device.h"
#include "kb_host.hpp"
#include "kb_waterfill.hpp"
#include "kb_preempt.hpp"

using namespace kb;

#define HIP_OK(expr)                                                                                      \
  do {                                                                                                    \
    hipError_t _e = (expr);                                                                               \
    if (_e != hipSuccess) throw EngineError(KB_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

namespace kbe {

inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;   // the size asked for last
  size_t cap = 0;     // what is allocated: a session of the same size (the Go action loads one every cycle) or a smaller one reuses it —
                      // hipFree synchronises the device and hipMalloc is not cheap either
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    cap = 0;
  }
  void swap(DevBuf &o) { std::swap(p, o.p); std::swap(bytes, o.bytes); std::swap(cap, o.cap); }
  void alloc(size_t n) {
    n = n ? n : 16;
    if (p && n <= cap) { bytes = n; return; }
    release();
    bytes = cap = n;
    HIP_OK(hipMalloc(&p, cap));
  }
  template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
  void copy_of(const DevBuf &src, hipStream_t s) {   // this := src, device to device on s, nothing waited for
    alloc(src.bytes);
    HIP_OK(hipMemcpyAsync(p, src.p, src.bytes, hipMemcpyDeviceToDevice, s));
  }
};

// grow-only pinned host array: the per-round staging buffers (window rows in, decision records out) are copied with
// hipMemcpyAsync every round, which only is asynchronous (and cheap to issue) from page-locked memory
template <typename T> struct Pinned {
  T *p = nullptr;
  size_t n = 0;
  unsigned flags = hipHostMallocDefault;
  Pinned() = default;
  Pinned(const Pinned &) = delete;
  Pinned &operator=(const Pinned &) = delete;
  ~Pinned() { if (p) (void)hipHostFree(p); }
  void resize(size_t m) {
    if (m <= n) return;
    T *q = nullptr;
    HIP_OK(hipHostMalloc((void **)&q, sizeof(T) * m, flags));
    if (p) { std::memcpy(q, p, sizeof(T) * n); (void)hipHostFree(p); }
    p = q;
    n = m;
  }
  T *data() { return p; }
  const T *data() const { return p; }
  size_t size() const { return n; }
  T &operator[](size_t i) { return p[i]; }
  const T &operator[](size_t i) const { return p[i]; }
};

// kb_session_load's staging: ONE pinned area, grow-only like the device buffers, in which every host-to-device source of a load is
// assembled (padding included) and from which it is copied asynchronously.  Round 4 copied from pageable memory — the caller's snapshot,
// std::vectors of this file —: the runtime pins such a source on the fly (or stages it, blocking) at every call, a per-call cost of
// tens to hundreds of microseconds with a long tail, about thirty times per load, and upload_padded synchronised the stream behind each
// of its eight temporaries.  A block stays valid until the next load resets the area, and a load ends behind a stream synchronisation.
// Sources of 8 MiB and more that outlive the load (the task vectors of a million-task session: Uploader::copy_persistent) skip the area: one pin
// per call is cheaper than the extra pass over them.
struct PinnedArena {
  struct Block { unsigned char *p; size_t cap; };
  std::vector<Block> blocks;
  size_t cur = 0, off = 0;
  PinnedArena() = default;
  PinnedArena(const PinnedArena &) = delete;
  PinnedArena &operator=(const PinnedArena &) = delete;
  ~PinnedArena() { for (Block &b : blocks) (void)hipHostFree(b.p); }
  void reset() { cur = 0; off = 0; }
  void *take(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    while (cur < blocks.size() && off + bytes > blocks[cur].cap) { cur++; off = 0; }
    if (cur == blocks.size()) {
      Block b{nullptr, std::max<size_t>(bytes, (size_t)8 << 20)};
      HIP_OK(hipHostMalloc((void **)&b.p, b.cap, hipHostMallocDefault));
      blocks.push_back(b);
      off = 0;
    }
    void *p = blocks[cur].p + off;
    off += bytes;
    return p;
  }
  size_t bytes_held() const { size_t t = 0; for (const Block &b : blocks) t += b.cap; return t; }
};
constexpr size_t kStageMaxBytes = (size_t)8 << 20;

// What an upload hands back: the device copy, typed as its source, so that a KbDev view is bound on the line of its upload.  It converts to a
// pointer to any element type of the same size, signedness and kind (the ABI's int64_t / uint64_t arrays are KbDev's long long / unsigned long long).
template <typename T> struct DevPtr {
  T *p;
  template <typename U, typename = std::enable_if_t<sizeof(U) == sizeof(T) && std::is_signed<U>::value == std::is_signed<T>::value &&
                                                    std::is_floating_point<U>::value == std::is_floating_point<T>::value>>
  operator U *() const { return reinterpret_cast<U *>(p); }
};

struct Uploader {
  PinnedArena &arena;
  hipStream_t s;
  Uploader(PinnedArena &a, hipStream_t st) : arena(a), s(st) {}
  // b := n elements the caller writes through the returned pointer BEFORE the next take / copy (the copy is queued by commit(), which takes that pointer)
  template <typename T> T *stage(DevBuf &b, size_t n) {
    b.alloc(n * sizeof(T));
    pending_dst = b.p; pending_bytes = n * sizeof(T);
    return reinterpret_cast<T *>(arena.take(pending_bytes ? pending_bytes : 16));
  }
  template <typename T> DevPtr<T> commit(T *staged) {
    if (pending_bytes) HIP_OK(hipMemcpyAsync(pending_dst, staged, pending_bytes, hipMemcpyHostToDevice, s));
    pending_bytes = 0;
    return {reinterpret_cast<T *>(pending_dst)};
  }
  // any source: copied into the area first (the source may die before the load's synchronisation: block-scoped temporaries)
  template <typename T> DevPtr<T> copy(DevBuf &b, const T *src, size_t n) {
    T *p = stage<T>(b, n);
    if (n) std::memcpy(p, src, n * sizeof(T));
    return commit(p);
  }
  // a source that outlives the load's synchronisation (the caller's snapshot, the host session's vectors): from 8 MiB on straight from where it
  // lies — the runtime pins it for the transfer; one pin per call is cheaper than an extra pass over a million-task vector
  template <typename T> DevPtr<T> copy_persistent(DevBuf &b, const T *src, size_t n) {
    if (n * sizeof(T) < kStageMaxBytes) return copy(b, src, n);
    b.alloc(n * sizeof(T));
    HIP_OK(hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
    return {b.as<T>()};
  }
  // rows of a [rows][n] host matrix into a padded [max(rows, 1)][np] device matrix (the pad, and the one row of a matrix without rows: `fill`)
  template <typename T> DevPtr<T> padded(DevBuf &b, const T *src, size_t rows, size_t n, size_t np, T fill = T(0)) {
    T *p = stage<T>(b, std::max<size_t>(rows, 1) * np);
    if (!rows) std::fill(p, p + np, fill);
    for (size_t r = 0; r < rows; r++) {
      if (n) std::memcpy(p + r * np, src + r * n, n * sizeof(T));
      std::fill(p + r * np + n, p + (r + 1) * np, fill);
    }
    return commit(p);
  }
 private:
  void *pending_dst = nullptr;
  size_t pending_bytes = 0;
};

struct Timer {   // HIP-event pair on the engine stream
  hipEvent_t a = nullptr, b = nullptr;
  void init() {
    HIP_OK(hipEventCreate(&a));
    HIP_OK(hipEventCreate(&b));
  }
  void destroy() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    a = b = nullptr;
  }
};

}  // namespace kbe
using namespace kbe;

struct MgState;
void mg_free(MgState *m);
void mg_reset(MgState *m);

struct kb_engine {
  std::string err;
  int device = 0;
  uint32_t window = 256, commit_batch = 0, flags = 0;   // 256: measured optimum on the 100k x 10k snapshots (small dirty sets vs per-round cost)
  Policy pol;
  hipStream_t stream = nullptr, own_stream = nullptr;   // stream: the one in use (own_stream unless kb_engine_use_stream gave another)
  bool loaded = false;
  bool tainted = false;   // an evict action failed after it had touched device / host state: kb_run_* answer KB_E_STATE until kb_session_load / kb_session_reset
  HostSession hs;
  KbDev dev{};
  kb_stats stats{};
  uint64_t round_no = 0;

  // session buffers
  DevBuf b_idle, b_rel, b_nzc, b_nzm, b_podcnt, b_acpu, b_amem, b_maxpods, b_ncls, b_nmask, b_invac, b_invam;
  uint64_t k5_walks = 0, k5_rescans = 0, k5_demand = 0, k5_slots = 0;   // commit kernel counters (KB_K5_STATS)
  double k5_trace[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double tl_repair_tag = 0;   // KB_K5_STATS: ms between the start of a repair launch and the moment its first workgroup had seen its list's tag
  uint32_t eff_window = 0;   // window actually used for this session (bounded by the commit kernel's LDS budget)
  // Which commit kernel a round runs on: the selection kernel (kb_commit_sel.hip), backfill rounds included; KB_COMMIT_KERNEL=run|select pins
  // one of the two — they compute the same decisions, and every -m gpu case runs under each (the run kernel, kb_commit.hip, is the plain
  // serial restatement the selection is held to).  Round 3's batch kernel (speculation across shapes) and the per-round rules that chose
  // between kernels lost to plain selection on every configuration (profiles/round4/call30_pinned_kernels) and are gone: HISTORY.md.
  int commit_kernel = KB_COMMIT_SELECT, commit_pin = -1;
  double dirty_share = 0.0;   // share of rows won by a node the round had already changed (exponential average; a statistic)
  uint64_t rounds_run = 0, rounds_sel = 0;
  uint64_t sel_stat[4] = {0, 0, 0, 0};   // selection kernel: runs with every pick a clean first placement / committed by shots; shots cut short by a table's end; shots
  uint32_t shape_cap = KB_K5_MAX_SHAPES;   // distinct shapes a window may hold (each keeps its candidate list in the commit kernel's LDS); ActionRun::admit_shape keeps to it
  const double *t_fit = nullptr;   // backfill's view of t_init (BestEffort rows: Resreq cpu / memory), == b_tinit when they agree
  bool idle_below_eps = false;
  DevBuf b_tfit;
  DevBuf b_tinit, b_tres, b_tnzc, b_tnzm, b_tcls, b_tactive, b_tresmask, b_tjob, b_tstatus, b_tnode, b_tbind, b_tcounted, b_jallocated, b_compat, b_crows, b_aff, b_affcls;
  // pristine copies for kb_session_reset, one per entry of kb_load.cpp's for_each_live: THE list of the buffers an action changes on the device
  // (the load's snapshot and the reset's restore both walk it; a new live buffer is one line there and nothing here)
  std::unique_ptr<DevBuf[]> p_live;
  // inter-pod (anti)affinity tables (kb_interpod)
  DevBuf b_ip_cdom, b_ip_ccnt, b_ip_ctot, b_ip_tinc, b_ip_tforbid, b_ip_treq, b_ip_tself, b_ip_tsubj, b_ip_tchk, b_ip_pdom, b_ip_pbound, b_ip_punb, b_ip_tcinc,
      b_ip_tsig, b_ip_sigw, b_ip_z, b_ip_scnt, b_ip_shist;
  DevBuf b_ports, b_twant, b_tconf;   // host ports (only when the snapshot carries any)
  DevBuf b_ports_x, b_twant_x, b_tconf_x;   // their words behind the first (kb_snapshot.port_words > 1 and some pod reaches there)
  DevBuf b_jbegin, b_jmin, b_jqueue, b_total, b_deserved, b_desmask, b_jalloc, b_jshare, b_qalloc, b_qshare, b_jready;
  uint32_t total_mask = 0;
  // round buffers
  DevBuf b_desc;
  Pinned<unsigned long long> h_listkeys;  // one complete candidate list of an evict action's preemptor shape (D2H target)
  Pinned<unsigned char> h_evict;          // an evict action's entry / exit staging: node state and task table through ONE pinned block, one synchronisation each way
  DevBuf b_scatter;                       // packed node records of upload_live_nodes
  Pinned<unsigned long long> h_scatter;
  DevBuf b_sscore, b_smask, b_xslot, b_xorder, b_xchunks;   // per-shape rows, row->shape map, rows in shape order and its chunk table (kb_eval_matrix / kb_bench_matrix)
  std::vector<uint32_t> h_xorder;
  std::vector<KbXChunk> h_xchunks;
  size_t xs_cap = 0, xslot_cap = 0;
  DevBuf b_mrows, b_same, b_score, b_maskw, b_keys;
  // Overlapped candidate lists: the matrix and arg-max launches of a chained round run on a second stream
  // beside its predecessor's commit kernel, into buffers of their own (matrix rows, stale lists per staging half, one `ready` word per
  // list, a scratch block for their time stamps); kb_launch_repair on the first stream turns the stale lists into the round's lists
  hipStream_t stream_b = nullptr;
  DevBuf b_score2, b_maskw2, b_stale, b_ready, b_task_rows, b_lready;   // b_lready: one word per repaired list and staging half (KbRound::lists_ready)
  bool fuse_repair = true;   // the selection kernel's launch carries its round's repair workgroups (KB_FUSE_REPAIR=0: the launch of its own in front of it)
  Pinned<unsigned long long> h_cand_out;   // per staging half: the output-block words the second stream's launches stamp (start of the matrix launch, start of the arg-max launch)
  unsigned long long *d_cand_out = nullptr;
  uint32_t mat2_cap = 0;
  size_t stale_cap = 0;
  bool overlap = true;             // KB_OVERLAP=0: every round on the plain path (matrix -> arg-max -> commit on one stream)
  uint64_t overlapped_rounds = 0, overlap_faults = 0;
  bool device_waterfill = true;    // proportion's water-fill runs as a launch at kb_session_load (kb_waterfill.hip); KB_DEVICE_WATERFILL=0: the host loop of kb_session.cpp (A/B)
  uint32_t waterfill_passes = 0;
  DevBuf b_wf_queues, b_wf_state;
  DevBuf b_win, b_out;   // per-round upload / download blocks (see h_win / h_out)
  DevBuf b_chain;        // KbRound::chain: tag of the last round that committed its whole window
  // feasibility probe at speculation breaks (ActionRun::probe_launch / probe_collect): one representative task per feasibility shape still alive.
  // Rows in and flags out live in mapped pinned memory the kernel reads and writes directly (like h_win / h_out): the probe is ONE stream
  // operation — it was copy -> memset -> kernel -> copy, ~4.5 us each with a gap behind each, around a kernel of 8.6 us
  Pinned<uint32_t> h_probe_alive, h_probe_rows;
  uint32_t *d_probe_alive = nullptr, *d_probe_rows = nullptr;   // their device addresses (re-read when kb_session_load grew them)
  bool probe_enabled = true;          // KB_PROBE=0 disables
  uint64_t probes = 0, probe_deaths = 0;
  int commit_kernel_of[2] = {0, 0};   // the commit kernel launched for the round in each staging half
  uint32_t win_cap = 0, mat_cap = 0;
  size_t keys_cap = 0;
  Pinned<uint32_t> h_rows, h_slot, h_mrows;   // h_rows: kb_matrix.cpp's row range (a round's rows are its ActionRun's: Window)
  std::vector<uint32_t> h_decnode, h_deckind;
  Pinned<uint32_t> h_win;             // per-round upload  [rows | slots | mrows] at fixed offsets of KB_K5_MAX_WINDOW
  Pinned<unsigned long long> h_out;   // per-round download: KB_OUT_HDR header words (kb_device.h) + decision records
  const uint32_t *d_hwin = nullptr;       // device view of h_win
  unsigned long long *d_hout = nullptr;   // device view of h_out (fast rounds: the commit kernel writes it directly)
  bool fast_rounds = true;            // host spins on h_out[KB_OUT_SEQ] instead of synchronising the stream every round
  bool chain_rounds = true;           // queue the next speculated round behind the running one (KbRound::chain); KB_CHAIN_ROUNDS=0 disables
  unsigned long long seq = 0;
  double wall_khz = 100000.0;         // rate of the device's constant wall clock
  std::vector<uint8_t> h_same;
  std::vector<uint32_t> shape_stamp, shape_slot_of;   // per row-shape id: round stamp and slot inside the current round
  uint32_t stamp = 0;
  std::vector<Timer> ev;          // event pool for per-launch timing
  PinnedArena load_arena;         // kb_session_load's staging area (above)
  Pinned<unsigned char> h_fin;    // pinned D2H target of run_finalize (seven results in one block, copied out after ONE synchronisation)
  // the host mirrors of the device reduction as of kb_session_load: kb_session_reset restores them instead of reducing the restored
  // (identical) state again
  struct FinalMirror { std::vector<double> job_alloc, job_share, queue_alloc, queue_share; std::vector<int32_t> job_ready; std::vector<uint8_t> t_status; std::vector<uint32_t> t_node; bool valid = false; } fin0;
  // where the host's wall time of a cycle goes outside the device rounds (KB_K5_STATS=1 prints it): reset, the action's start up to its
  // first launch, the speculation breaks (from a stopped round's answer to the re-planned launch), the closing reduction, round waits
  bool async_pending = false;   // kb_session_reset queued device-to-device copies on `stream` and returned without waiting: whoever touches the
                                // buffers outside that stream (null-stream copies of the getters and of the evict actions, a stream switch) waits first
  // "a Pending task carries a NodeName" is looked for in front of an allocate / backfill only when it can have appeared: once per loaded
  // session (load_clean remembers that the load-time state passed; kb_session_reset returns to that state) and after every evict action
  // (a discarded statement is the one thing inside a session that creates such a task)
  bool stale_checked = false, pristine = true, load_clean = false;
  double tl_reset = 0, tl_begin = 0, tl_break = 0, tl_finish = 0, tl_wait = 0, tl_backfill = 0;
  double tl_begin_parts[3] = {0, 0, 0};   // of tl_begin: the order machine's set-up, the first feasibility probe, the first plan (the rest: buffers, the first launch)
  double tl_break_parts[3] = {0, 0, 0};   // of tl_break: the probe's launch + absorbing the answer (roll-back + replay) beside it, waiting for the probe, the re-plan (the rest: the skipped round, the launch)
  std::vector<kb_decision> decisions_all;   // decisions of the last multi-GPU round sequence
  std::vector<uint32_t> evictions;          // committed evictions of the session's preempt actions, in cache.Evict order

  // multi-GPU round state (kb_round_*), defined below
  struct MgState *mg = nullptr;
  std::unique_ptr<PreemptMachine> evict_machine;   // kb_evict.cpp: kept for the engine's life (grow-only tables, like the device buffers)

  ~kb_engine() {
    mg_free(mg);
    for (auto &t : ev) t.destroy();
    if (own_stream) (void)hipStreamDestroy(own_stream);
    if (stream_b) (void)hipStreamDestroy(stream_b);
  }
};

extern thread_local std::string g_create_err;

namespace kbe {

// ---- buffers, timers, the closing reduction (kb_engine.cpp)
void ensure_window_buffers(kb_engine *e, uint32_t rows);
void ensure_ip_scratch(kb_engine *e, size_t rows);
void ensure_matrix_buffers(kb_engine *e, uint32_t mrows, uint32_t L);
Timer &get_timer(kb_engine *e, size_t i);
void quiesce(kb_engine *e);
void run_finalize(kb_engine *e, const std::function<void()> &after_sync = nullptr);
int guarded(kb_engine *e, const std::function<void()> &fn);

// ---- rounds (kb_rounds.cpp)
KbRound make_round(kb_engine *e, uint32_t n_rows, uint32_t n_mrows, uint32_t L, int fit_mode, bool backfill, uint32_t buf = 0);
uint32_t assign_shapes(kb_engine *e, const uint32_t *rows, uint32_t n);
// ---- one device round, in three host steps so the multi-GPU path can interleave its collectives ----
struct RoundCtx {
  KbRound r{};
  KbDev d{};
  uint32_t n = 0, ns = 0, L = 0;
  bool backfill = false;
  bool direct = false;           // the kernels read the window from the pinned staging block (no copy command)
  uint32_t buf = 0;              // which half of the pinned upload / download blocks the round uses (chained rounds alternate)
  unsigned long long seq = 0;    // the sequence number its commit kernel publishes
  bool overlapped = false;       // its candidate lists were built on the second stream and repaired (round_candidates_overlapped)
};
RoundCtx round_prepare(kb_engine *e, const uint32_t *rows, uint32_t n, int fit_mode, bool backfill, bool gather_in_matrix = false, uint32_t buf = 0,
                       uint32_t chain_expect = 0);
void round_candidates(kb_engine *e, const RoundCtx &c, uint32_t m0, uint32_t m1, unsigned long long *keys);
void ensure_overlap_buffers(kb_engine *e, uint32_t mrows, uint32_t stale_L);
void round_candidates_overlapped(kb_engine *e, RoundCtx &c, uint32_t n_prev, unsigned long long *keys);
void round_commit(kb_engine *e, const RoundCtx &c, unsigned long long *keys, double *delta, uint32_t own0, uint32_t own1);
void round_collect(kb_engine *e, const RoundCtx &c, bool had_candidates, uint32_t &n_done, uint32_t &reason);
void check_aggregates(kb_engine *e, const OrderMachine &om);

// One planned window of an action and where it stands in run_action's pipeline
struct Window {
  std::vector<uint32_t> rows;   // task ids, eff_window entries (ActionRun::begin)
  uint32_t n = 0;               // ... of which the planner filled this many
  uint64_t pops = 0;            // what the order machine popped for them (tasks of dead shapes included)
  bool planned = false;         // a speculated slot holds a window (n == 0: the order machine ran dry)
  bool launched = false;        // its round is on the device: running (the current slot) or queued behind the running one (the next slot)
  RoundCtx ctx;                 // ... that round
  void set(uint32_t n_, uint64_t pops_) { n = n_; pops = pops_; planned = true; launched = false; }
};

// Host side of one action as a resumable object (bodies: kb_rounds.cpp): plan() fills the current window, absorb() digests the device's answer
// (confirm, or roll back + replay on a mis-speculated round), finish() runs the gang/share reduction.  run_action drives it for
// kb_run_allocate / kb_run_backfill, kb_round_* a round at a time through MgState.
struct ActionRun {
  uint32_t action = 0;   // 0 allocate, 1 backfill
  bool bf_need_pred = false;
  std::vector<int> bf_podcnt;
  std::vector<unsigned long long> bf_ports, bf_ports_x;   // word 0 [NP]; the words behind it [port_xw][NP]
  OrderMachine om;
  std::vector<uint8_t> dead;   // per feasibility shape (mark_dead, the probe); backfill marks none
  std::vector<kb_decision> decs;
  std::vector<uint32_t> bf_list;
  size_t bf_pos = 0;
  uint64_t popped = 0;
  Window cur, next, next2;   // the window the device works on (or is about to), the one speculated behind it, and the one behind that
  std::vector<uint32_t> plan_stamp;   // per row-shape id: stamp of the window being planned
  uint32_t plan_epoch = 0;
  std::vector<uint32_t> probe_list;  // feasibility shapes the probe looks at (the ones still alive)
  uint32_t probe_calls = 0, probe_S = 0;   // probe_S: rows of the probe in flight (0: none)
  double host_ms = 0, t_start = 0;
  bool active = false;

  // starts the action: the order machine (allocate) or the BestEffort task list (backfill), no window planned, no shape dead
  void begin(kb_engine *e, uint32_t act);
  // feasibility shape x and every shape it dominates are dead for the rest of the action
  void mark_dead(const HostSession &hs, uint32_t x);
  // a window holds at most e->shape_cap distinct task shapes (one lane of the commit kernel's main wave each)
  void new_window() { plan_epoch++; }
  bool admit_shape(const kb_engine *e, uint32_t shape, uint32_t &nshapes);
  // what the planner does with task t when the window being planned holds n rows of nshapes shapes: the admission rule, stated once
  enum class Admit { Dead, Next, Join, Alone };
  Admit admit(const kb_engine *e, uint32_t t, uint32_t n, uint32_t &nshapes);
  // w := up to eff_window admitted tasks from the order machine, each reported as Allocated
  void fill(kb_engine *e, Window &w);
  // cur := the next window, behind a fresh roll-back point (allocate) or from bf_pos on (backfill); returns its row count, 0: the action is complete
  uint32_t plan(kb_engine *e);
  // next (`second`: next2) := the window behind the last one planned, behind a roll-back point of its own; returns its row count
  uint32_t plan_ahead(kb_engine *e, bool second = false);
  // the window in flight is confirmed: next becomes cur and next2 moves up; the slots rotate, no row is copied
  void promote();
  // the plugin predicates of task t (predicates.go:127,181-190 and the static class table) against the pod counts / ports
  // backfill started from: a superset of the nodes that pass at any later point of the action
  bool passed_predicates_at_start(kb_engine *e, uint32_t t) const;
  // the feasibility probe: every shape still alive without a node in the current state is marked dead.  In two halves around the host's work on
  // a break's answer; probe_abandon() when that work throws between them (the kernel must not outlive the call: it writes into h_probe_alive)
  void probe_launch(kb_engine *e);
  void probe_collect(kb_engine *e);
  void probe_abandon(kb_engine *e) { if (probe_S) { (void)hipStreamSynchronize(e->stream); probe_S = 0; } }
  void probe_dead_shapes(kb_engine *e) { probe_launch(e); probe_collect(e); }
  // the answer (n_done rows, reason) to cur's round: its decisions join decs; a break rolls the order machine back to the round's start, replays
  // the confirmed prefix and feeds the true outcome of the row that broke.  absorb() = absorb_round() + the placed pods' host-port words behind the first
  void absorb(kb_engine *e, uint32_t n_done, uint32_t reason);
  void absorb_round(kb_engine *e, uint32_t n_done, uint32_t reason);
  // the closing reduction (when anything was decided), the aggregate cross-check, the action's share of kb_stats
  void finish(kb_engine *e);
};

}  // namespace kbe

// The node state at the start of a round of the task-row split (kb_round_*): the reduced deltas are applied to it and checked against it
struct NodeStart {
  DevBuf idle, rel, nzc, nzm, podcnt;
  void take(kb_engine *e) {   // five device-to-device copies of the live arrays on e->stream
    idle.copy_of(e->b_idle, e->stream); rel.copy_of(e->b_rel, e->stream); nzc.copy_of(e->b_nzc, e->stream); nzm.copy_of(e->b_nzm, e->stream); podcnt.copy_of(e->b_podcnt, e->stream);
  }
  KbNodeCopy view() const { return KbNodeCopy{idle.as<double>(), rel.as<double>(), nzc.as<long long>(), nzm.as<long long>(), podcnt.as<int>()}; }
  void swap(NodeStart &o) { idle.swap(o.idle); rel.swap(o.rel); nzc.swap(o.nzc); nzm.swap(o.nzm); podcnt.swap(o.podcnt); }
};

struct MgState {
  ActionRun run;   // run.cur.ctx is the round between kb_round_begin and kb_round_apply
  bool in_round = false, committed = false, had_candidates = false;
  uint32_t n_done = 0, reason = 0;
  std::vector<kb_decision> last_decs;
  // node state at the start of the round and of the one BEFORE it: the deferred cross-check (kb_round_check) compares that round's reduced deltas
  // against the two, one round late; a device counter of differing values that lives for the action, the rounds begun in it
  NodeStart cur, prev;
  DevBuf chk_counter;
  uint32_t rounds_begun = 0;
  bool chk_valid = false;   // chk_counter belongs to an action begun since the last load / reset
};
