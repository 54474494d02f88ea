// tsdf_capi.cpp — extern "C" boundary of libtsdf_hip.so (declared in include/tsdf_hip.h).
//
// One tsdf_ctx = one HIP device + one non-blocking stream + the brick hash table, brick pool and
// batch work buffers, all allocated once at create (no allocation on the integrate path).  The
// host-pointer integrate packs the caller's PointCloud2-style records (any point_step/xyz_offset,
// f32 or f64 xyz) into one of two pinned staging buffers, copies them into the device staging
// area of the pending batch and returns; the batch is launched when max_batch scans are pending
// or when any other call needs the field (see "Batching" in the header).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/tsdf_hip.h"
#include "../../include/tsdf_hip_deskew.h"
#include "../../include/tsdf_hip_coarsen.h"
#include "../../include/tsdf_hip_columns.h"
#include "../../include/tsdf_hip_esdf.h"
#include "../../include/tsdf_hip_frontier.h"
#include "../../include/tsdf_hip_merge.h"
#include "../../include/tsdf_hip_mesh.h"
#include "../../include/tsdf_hip_prune.h"
#include "../../include/tsdf_hip_raycast.h"
#include "../../include/tsdf_hip_sample.h"
#include "../../include/tsdf_mc_tables.h"
#include "brick_key.h"
#include "coarsen_plan.h"
#include "ctx_plan.h"
#include "columns_plan.h"
#include "esdf_plan.h"
#include "frontier_plan.h"
#include "host_pack.h"
#include "merge_plan.h"
#include "mesh_plan.h"
#include "os_headers.h"
#include "pack_pool.h"
#include "prune_plan.h"
#include "tsdf_device.h"

using namespace tsdf;

static_assert(TSDF_MAX_BATCH == MAX_BATCH, "header and device batch limits differ");
static_assert(TSDF_TILE_WORDS == TILE_WORDS && TSDF_MAX_WORLD == MAX_WORLD, "border tile layout differs");
static_assert(TSDF_MC_TABLES == MC_TABLES, "marching-cubes table count differs");
static_assert(BRICK_KEY_BIAS == BRICK_COORD_BIAS, "host and device brick keys differ");

namespace {

// Diagnostic host timing of launch() sections (TSDF_HOST_TIMING=1: averages printed at destroy).
// launch()'s slots, by the number the stderr line prints them under (2 and 11: unused, 0.00):
enum HtSlot {
    HT_PRE = 0, HT_WAITS = 1, HT_FRONT = 3, HT_COMPACT = 4, HT_BACK = 5, HT_INTEGRATE = 6,
    HT_FINISH = 7, HT_RING_WAIT = 8, HT_RING_COPY = 9, HT_UPLOAD = 10
};
struct HostTiming {
    bool on = std::getenv("TSDF_HOST_TIMING") != nullptr;
    double acc[12] = {};
    uint64_t n = 0;
    std::chrono::steady_clock::time_point t;
    void start() { if (on) t = std::chrono::steady_clock::now(); }
    void lap(int k) {
        if (!on) return;
        const auto u = std::chrono::steady_clock::now();
        acc[k] += std::chrono::duration<double, std::micro>(u - t).count();
        t = u;
    }
    ~HostTiming() {
        if (!on || !n) return;
        std::fprintf(stderr, "host launch timing (us/batch over %llu):", (unsigned long long)n);
        for (int k = 0; k < 12; k++) std::fprintf(stderr, " %d:%.2f", k, acc[k] / n);
        std::fprintf(stderr, "\n");
    }
};

struct EventTimer final : KernelTimer {
    struct Rec { int kind; uint64_t batch; hipEvent_t a, b; bool own_a; };
    uint64_t cur_batch = 0;  // the batch being launched (set by launch())
    bool per_batch = false;  // keep per-batch times for the metrics log
    std::vector<std::pair<uint64_t, std::array<double, KIND_N>>> batch_ms;
    std::vector<hipEvent_t> free_ev;
    std::vector<Rec> pending;
    hipEvent_t open_ev[KIND_N] = {};
    bool open_own[KIND_N] = {};  // open_ev[k] is not also the end of an earlier record
    uint32_t every_mask = ~0u;   // kinds timed on every batch (tsdf_set_profiling_period)
    uint32_t period = 1;         // the other kinds: every period-th batch
    bool want(int kind) const { return ((every_mask >> kind) & 1u) || cur_batch % period == 0; }
    double ms[KIND_N] = {};
    uint64_t launches[KIND_N] = {};

    hipEvent_t get() {
        if (free_ev.empty()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            return e;
        }
        hipEvent_t e = free_ev.back();
        free_ev.pop_back();
        return e;
    }
    void begin(int kind, hipStream_t st) override {
        open_ev[kind] = get();
        open_own[kind] = true;
        if (open_ev[kind]) (void)hipEventRecord(open_ev[kind], st);
    }
    void end(int kind, hipStream_t st) override {
        hipEvent_t e = get();
        if (!e || !open_ev[kind]) return;
        (void)hipEventRecord(e, st);
        pending.push_back({kind, cur_batch, open_ev[kind], e, open_own[kind]});
        open_ev[kind] = nullptr;
    }
    // events the kernel launch itself records (its dispatch packet's timestamps: KTime)
    KTime timing(int kind) {
        hipEvent_t a = get(), b = get();
        if (!a || !b) return {};
        pending.push_back({kind, cur_batch, a, b, true});
        return {a, b};
    }
    // end `done` and begin `open` with ONE event, for kernels launched back to back on one stream
    // (every timing event is a queue barrier with a timestamp: ~4 us each per batch)
    void next(int done, int open, hipStream_t st) {
        hipEvent_t e = get();
        if (!e || !open_ev[done]) return begin(open, st);
        (void)hipEventRecord(e, st);
        pending.push_back({done, cur_batch, open_ev[done], e, open_own[done]});
        open_ev[done] = nullptr;
        open_ev[open] = e;
        open_own[open] = false;
    }
    // call only after the stream drained
    void harvest() {
        for (auto& r : pending) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
                ms[r.kind] += t;
                launches[r.kind]++;
                if (per_batch) {
                    if (batch_ms.empty() || batch_ms.back().first != r.batch)
                        batch_ms.push_back({r.batch, std::array<double, KIND_N>{}});
                    batch_ms.back().second[r.kind] += t;
                }
            }
            if (r.own_a) free_ev.push_back(r.a);  // else it is an earlier record's b
            free_ev.push_back(r.b);
        }
        pending.clear();
    }
    void reset() {
        std::fill(ms, ms + KIND_N, 0.0);
        std::fill(launches, launches + KIND_N, 0);
    }
    ~EventTimer() override {
        for (auto& r : pending) {
            if (r.own_a) (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
        for (auto e : free_ev) (void)hipEventDestroy(e);
    }
};

uint64_t next_pow2(uint64_t v) {
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// Sector k of n starts at the pseudo-angle of yaw0 + 2 pi k / n (include/tsdf_hip.h
// tsdf_sector_of); the oracle computes the same bounds with the same operations.
float sector_start(double yaw0, uint32_t k, uint32_t n) {
    const double th = yaw0 + 6.283185307179586476925286766559 * (double)k / (double)n;
    return pseudo_angle((float)std::cos(th), (float)std::sin(th));
}

void sector_bounds(double yaw0, uint32_t sector, uint32_t n, RayConst& R) {
    R.sec_on = n > 1 ? 1 : 0;
    if (!R.sec_on) return;
    R.sec_lo = sector_start(yaw0, sector, n);
    R.sec_hi = sector_start(yaw0, (sector + 1) % n, n);
    R.sec_wrap = R.sec_hi <= R.sec_lo ? 1 : 0;
}

// ---- the owners of a context's HIP resources -------------------------------------

// A device or pinned buffer, an event, a stream: each frees what it holds when it is destroyed,
// reset or assigned over, and an empty one frees nothing, so a half-built context tears down like
// a whole one.  They convert to the raw handle: the kernels' argument structs (Table, Pool, Work,
// MgBufs) are views filled from them (set_views).
template <class T, bool PINNED>
struct HipBuf {
    T* p = nullptr;
    HipBuf() = default;
    explicit HipBuf(T* q) : p(q) {}
    HipBuf(HipBuf&& o) noexcept : p(std::exchange(o.p, nullptr)) {}
    HipBuf& operator=(HipBuf&& o) noexcept {
        if (this != &o) reset(std::exchange(o.p, nullptr));
        return *this;
    }
    ~HipBuf() { reset(); }
    void reset(T* q = nullptr) {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = q;
    }
    // a fresh allocation of `bytes` bytes (the owner must be empty)
    hipError_t alloc_bytes(size_t bytes) {
        return PINNED ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    }
    hipError_t alloc(size_t n) { return alloc_bytes(n * sizeof(T)); }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};
template <class T> using DevBuf = HipBuf<T, false>;
template <class T> using PinBuf = HipBuf<T, true>;

// An event without timing (the contexts order streams with them; EventTimer keeps its own) and a
// non-blocking stream
template <class H, hipError_t (*MAKE)(H*, unsigned), unsigned FLAGS, hipError_t (*KILL)(H)>
struct HipHandle {
    H h = nullptr;
    HipHandle() = default;
    HipHandle(const HipHandle&) = delete;
    HipHandle& operator=(const HipHandle&) = delete;
    ~HipHandle() { if (h) (void)KILL(h); }
    hipError_t create() { return MAKE(&h, FLAGS); }
    operator H() const { return h; }
};
using Event = HipHandle<hipEvent_t, hipEventCreateWithFlags, hipEventDisableTiming, hipEventDestroy>;
using Stream = HipHandle<hipStream_t, hipStreamCreateWithFlags, hipStreamNonBlocking, hipStreamDestroy>;


// The capacity-dependent buffers: brick pool, hash table, and per batch parity the cells and the
// per-brick work lists.  The context holds the installed one; growth builds a
// second and move-assigns it over the first, which frees the old buffers.
struct Capacity {
    uint64_t max_bricks = 0, cap = 0;
    uint32_t max_active = 0;
    DevBuf<uint64_t> keys, brick_keys;
    DevBuf<uint32_t> slots, touched, cell[2];  // (u64 cells with the single walk)
    DevBuf<float> sdf, weight;
    DevBuf<uint4> active[2], active_ord[2], cagg[2];
};

// One batch parity's capacity-independent buffers: the work lists (Work), sized by the plan and,
// for fb / smp / spn, doubled on overflow (grow_list), and the merged pre-pass' set (MgBufs;
// Voxblox MergedTsdfIntegrator only, tsdf_merged.hip)
struct Lane {
    DevBuf<uint32_t> pair, blk_n, plan, spn, ord_hist, act;
    DevBuf<uint32_t> tile;  // per scan of the batch: its ray tiles' column height (k_tile_detect)
    DevBuf<uint4> blk, fb;
    DevBuf<uint2> smp;
    DevBuf<uint64_t> mg_ekey;
    DevBuf<uint32_t> mg_eidx, mg_bcnt, mg_bst, mg_bscan;
    DevBuf<float> mg_xyz, mg_w;
};

// Batch records for the kernels: a pinned host ring and its device twin (launch() copies a batch's
// n_scans + 1 records into the next slot on the batch's stream), one event per slot
struct ScanRing {
    static constexpr int N = 16;
    PinBuf<ScanRec> host;
    DevBuf<ScanRec> dev;
    const ScanRec* host_dev = nullptr;  // `host` as the device addresses it (k_upload)
    // ring progress: k_upload of launch q stores q + 1 here once it has read its slot
    PinBuf<unsigned long long> done;
    unsigned long long* done_dev = nullptr;
    Event ev[N];
    uint64_t next = 0;

    hipError_t create() {
        hipError_t e = host.alloc((size_t)N * (MAX_BATCH + 1));
        if (e == hipSuccess) e = dev.alloc((size_t)N * (MAX_BATCH + 1));
        void* dp = nullptr;
        if (e == hipSuccess) e = hipHostGetDevicePointer(&dp, host, 0);
        host_dev = static_cast<const ScanRec*>(dp);
        if (e == hipSuccess) e = done.alloc_bytes(64);
        if (e == hipSuccess) *done = 0;
        if (e == hipSuccess) e = hipHostGetDevicePointer(&dp, done, 0);
        done_dev = static_cast<unsigned long long*>(dp);
        for (int k = 0; k < N && e == hipSuccess; k++) e = ev[k].create();
        return e;
    }
};

}  // namespace

struct tsdf_ctx {
    tsdf_params p{};
    int device = -1;
    Stream stream;
    RayConst R{};
    // what the kernels take: views of the owners below (set_views)
    Table T{};
    Pool Pl{};
    Work W2[2]{};
    MgBufs mg[2];
    DevBuf<Globals> G;
    uint64_t max_points = 0;  // per scan
    uint32_t max_batch = 0;
    CtxPlan plan;  // one batch's sizes (ctx_plan.h), as created
    uint32_t max_fb = 0, max_smp = 0, max_spn = 0;  // the growable lists' entries now (grow_list)
    // batches of at most small_ns scans take k_integrate_small (TSDF_SMALL_NS; 0: never; measured
    // break-even with k_integrate at 6 scans)
    int small_ns = 5;
    // batches of at most count_wide k_count blocks (about 4 full scans: too few workgroups of 256
    // lanes to fill the chip) run k_count with 1024-lane workgroups (TSDF_COUNT_WIDE; 0: never)
    uint32_t count_wide = 512;
    // TSDF_COUNT_PAIRED=1: larger batches run k_count with two blocks per 512-lane workgroup
    // (bit-exact, ~29% fewer cell atomics, but measured slower: DESIGN.md §10, round 4)
    bool count_paired = false;
    // TSDF_RAY_TILES: the walk kernels' blocks as 32 x 32 ray tiles of the scan instead of 1024
    // consecutive rays (ray_tile.h).  -1 (unset): scans whose points k_tile_detect finds to be
    // intact columns; 0: never; 64 / 128 / 256: every scan, with this column height.  Off for
    // sector contexts, the Merged pre-pass and the single walk.
    int ray_tiles = -1;
    // host-pointer path: pinned double buffer per scan; the pending batch's points are staged in
    // stage2[pend_stage]
    PinBuf<float> h_stage[2];
    Event stage_done[2];
    int stage_cur = 0;
    // Batch pipeline: batch b runs on bst[b & 1] with its own work buffers (lane, W2), per-scan
    // cells (K.cell) and device staging (stage2), so batch b + 1's count / compact / place overlap
    // batch b's place / integrate.  Cross-batch order: the table above launch() and DESIGN.md §5.
    Stream bst[2];
    Capacity K;  // the installed capacity
    Lane lane[2];
    DevBuf<float> stage2[2];
    Event ev_main;
    Event ev_compact[2];
    // the end of the last batch of each parity: the ring event of that batch's slot (one marker
    // per batch; every marker in the stream costs the GPU a few microseconds)
    hipEvent_t ev_integ[2] = {nullptr, nullptr};
    BatchDesc pend{};  // pending host scans (points in stage2[pend_stage])
    // Device staging ownership (independent of batch parity, which replays can shift): the pending
    // batch's buffer, and per buffer the last batch that read it (its id and completion event).
    int pend_stage = 0;
    int last_stage = 1;  // the buffer of the most recently launched host batch
    uint64_t stage_reader[2] = {~0ull, ~0ull};
    Event stage_ev[2];
    ScanRing ring;
    HostTiming ht;
    uint64_t batch_id = 0;
    uint64_t n_scans = 0, n_batches = 0, n_points_in = 0;
    EventTimer* timer = nullptr;
    std::string err;
    // Capacity growth: batches launched since the last check, replayable from their
    // still-valid input (caller device memory until tsdf_sync; host scans in stage2 until the
    // staging of batch id + 2, where a checkpoint runs first).
    struct Logged { uint64_t id; const float* xyz; BatchDesc D; };
    std::vector<Logged> log;
    bool can_grow = false;  // G->retry: overflowed batches are skipped and replayed
    bool in_replay = false;
    uint32_t ovf_refused = 0;  // OVF_* of batches re-run committing what fits, for tsdf_sync
    // metrics log (tsdf_set_metrics_log): one JSON line per finished batch
    FILE* metrics = nullptr;
    uint64_t metrics_next = 0;  // the next batch id to report
    struct BatchInfo { uint64_t id; uint32_t scans; uint64_t points; };
    std::vector<BatchInfo> metrics_info;  // host-side facts of the batches not yet reported
    PackPool* pack = nullptr;  // host staging threads (tsdf_integrate of strided records)
    // tsdf_integrate_sectors' packed scan (xyz, then the sector per point) when this context
    // leads the split: cache-resident between its two passes
    std::vector<float> split_xyz;
    std::vector<int8_t> split_sec;
    HostTiming split_ht;  // TSDF_HOST_TIMING: prep, classify, scatter, copies + queue (us/scan)
    uint64_t n_grows = 0, n_replayed = 0;
    // Voxblox MergedTsdfIntegrator (tsdf_params.voxblox_method): the bundling pre-pass runs first
    bool merged = false;
    // TSDF_SECTOR_RULE_INDEX sharding (ABI v10): the context takes points [share_lo, share_hi) of
    // every cloud (idx_share); the kernels' azimuth filter is off (R.sec_on = 0)
    bool idx_rule = false;
    // tsdf_create_sharded: the contexts whose device memory this one reaches directly (peer access
    // or the same device); tsdf_integrate_sectors' fan-out: its copy-done event (this device)
    uint64_t peer_mask = 0;
    Event bc_ev;
    // tsdf_integrate_sectors' fan-out, batch-granular: a follower's pending points [fan_lo, fan_hi)
    // are still in its leader's staging buffer fan_buf (same offsets: the contexts' batches run in
    // lockstep) and are copied in ONE device-to-device copy before the follower's batch launches
    // (fan_copy); the leader keeps its followers, so it never reuses a buffer they still read
    tsdf_ctx* fan_src = nullptr;
    const float* fan_buf = nullptr;
    uint64_t fan_lo = 0, fan_hi = 0;
    std::vector<tsdf_ctx*> fan_followers;
    // border-reduce transaction (ABI v9): the pool slots the open reduce's pack sent
    // (reset at commit) and, per merge, the received bricks' pre-merge tiles (written back at
    // abort).  While a reduce is open the context takes no scan and no import.
    bool brd_open = false;
    DevBuf<uint32_t> brd_sent;
    uint64_t brd_n_sent = 0;
    std::vector<std::pair<DevBuf<uint32_t>, uint64_t>> brd_backup;
    // tsdf_align_terms_device's workgroup partials and their sum (launch_align), allocated at the
    // first call
    DevBuf<double> align_part;
};

// A context with an open border reduce refuses new mass until the reduce is committed or aborted
// (a commit resets the sent bricks: mass integrated into them meanwhile would be lost).
static bool border_busy(tsdf_ctx* c);

// Weight cap of the weighted-mean merges (import, border reduce): Voxblox's max_weight, else none
static float merge_cap(const tsdf_ctx* c) {
    return c->p.semantics == TSDF_SEM_VOXBLOX ? c->p.max_weight : INFINITY;
}

static int fail(tsdf_ctx* c, int code, const char* fmt, ...) {
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return code;
}

#define HIPCHK(c, expr)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((c), TSDF_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));      \
    } while (0)

static int check_and_replay(tsdf_ctx* c);
static int drain_all(tsdf_ctx* c);
static int emit_metrics(tsdf_ctx* c);

// Before launch seq rewrites its host ring slot: launch seq - N (the slot's previous user) must
// have read it (its k_upload raised the progress word to seq - N + 1).  Waits like an event
// synchronize (spin, then yield), and checks the batch streams for errors while it waits.
static int ring_wait(tsdf_ctx* c, uint64_t seq) {
    if (seq < (uint64_t)ScanRing::N) return TSDF_OK;
    const unsigned long long need = seq - ScanRing::N + 1;
    for (uint64_t i = 0;; i++) {
        if (__atomic_load_n(c->ring.done.p, __ATOMIC_ACQUIRE) >= need) return TSDF_OK;
        if (i < 64) continue;
        std::this_thread::yield();
        if ((i & 1023) == 0) {
            bool idle = true;
            for (int q = 0; q < 2; q++) {
                const hipError_t e = hipStreamQuery(c->bst[q]);
                if (e == hipErrorNotReady) idle = false;
                else if (e != hipSuccess) HIPCHK(c, e);
            }
            if (idle && __atomic_load_n(c->ring.done.p, __ATOMIC_ACQUIRE) < need)
                return fail(c, TSDF_EHIP, "scan-record ring: upload %llu never completed",
                            (unsigned long long)(need - 1));
        }
    }
}

// ---- launch: one batch through the pipeline ---------------------------------------

// Cross-batch order.  Batch b runs on stream bst[b & 1] (serial: every batch on bst[0], where
// stream order is the whole rule) and orders itself against batch b - 1 on the other stream with
// two events of b - 1: `compact` (ev_compact: its table `touched` words are consumed, so b's front
// end may mark bricks) and `end` (ev_integ: its k_finish ran, so b may fuse into the same bricks).
//
//   pipeline    wait before front | before back | before integrate   ev_compact of b recorded
//   0 serial           -          |      -      |        -           never
//   1 overlap       compact       |      -      |       end          after k_compact
//   2 lean          compact       |     end     |        -           after the back end
//
// 1: b's front end runs beside b - 1's back end and integrate.  2: only b's front end and compact
// overlap b - 1's integrate; the back end always runs alone, and b + 1's front end starts after it.
// The waits and records in launch() carry the row numbers they belong to.

// Launch one batch (desc offsets relative to d_xyz); fills the workgroup prefix of D.
static int launch(tsdf_ctx* c, const float* d_xyz, BatchDesc& D) {
    if (D.n_scans == 0) return TSDF_OK;
    c->ht.start();
    // -- checkpoints: the device ring of batch records would wrap (metrics), or the replay log
    // grows without bound (device-pointer batches stay replayable until a check)
    const bool ring_full = c->metrics && c->batch_id - c->metrics_next >= METRIC_RING - 8;
    if (!c->in_replay && (ring_full || (c->can_grow && c->log.size() >= 1024))) {
        int rc = drain_all(c);
        if (!rc) rc = check_and_replay(c);
        if (!rc && ring_full) rc = emit_metrics(c);
        if (rc) return rc;
    }
    // -- block prefix: RPB rays per workgroup, one scan per workgroup
    D.s[0].blk = 0;
    for (uint32_t s = 0; s < D.n_scans; s++)
        D.s[s + 1].blk = D.s[s].blk + (D.s[s + 1].off - D.s[s].off + RPB - 1) / RPB;
    D.n_blocks = D.s[D.n_scans].blk;
    if (D.n_blocks > c->plan.max_blocks)
        return fail(c, TSDF_EINVAL, "batch needs %u workgroups > %u", D.n_blocks, c->plan.max_blocks);
    const int par = (int)(c->batch_id & 1);
    c->ht.lap(HT_PRE);
    // serial batches share one stream (stream order replaces the cross-stream waits); pipelined
    // batches alternate between two
    const bool cross = c->p.pipeline != 0, lean = c->p.pipeline == 2;
    hipStream_t st = c->bst[cross ? par : 0];
    Table T = c->T;
    T.cell = c->K.cell[par];
    const Work& W = c->W2[par];
    const bool prev = cross && c->batch_id > 0;  // a previous batch on the other stream
    EventTimer* tm = c->timer;
    if (tm) tm->cur_batch = c->batch_id;
    if (c->metrics) c->metrics_info.push_back({c->batch_id, D.n_scans, D.s[D.n_scans].off});
    // -- waits: staging uploads, imports, ... (an idle context stream has nothing to order against)
    if (hipStreamQuery(c->stream) != hipSuccess) {
        HIPCHK(c, hipEventRecord(c->ev_main, c->stream));
        HIPCHK(c, hipStreamWaitEvent(st, c->ev_main, 0));
    }
    // -- the batch's scan records into its host ring slot (reused once the slot's upload ran)
    ScanRing& ring = c->ring;
    const uint64_t seq = ring.next++;
    const int slot = (int)(seq % ScanRing::N);
    if (const int rc = ring_wait(c, seq)) return rc;
    c->ht.lap(HT_RING_WAIT);
    const size_t at = (size_t)slot * (MAX_BATCH + 1);
    ScanRec* ds = ring.dev + at;
    std::memcpy(ring.host + at, D.s, (D.n_scans + 1) * sizeof(ScanRec));
    c->ht.lap(HT_RING_COPY);
    // -- ray tiles: which scans are intact columns.  k_tile_detect needs only the points and the
    // scan records, which it reads from the host slot, so it runs ahead of the wait on the previous
    // batch, beside that batch's kernels.  (The upload stays behind the wait: ahead of it, k_count
    // started level with the previous batch's k_integrate instead of ~10 us after it, and
    // k_integrate, whose grid is sized to own the chip, ran 0.58-0.70 ms beside it instead of
    // 0.38 -- DESIGN.md §10.)
    const bool tiles = c->ray_tiles != 0 && !c->R.sec_on && !c->idx_rule && !c->merged &&
                       !c->plan.fused && D.n_blocks != 0;
    uint32_t* const d_tile = tiles ? c->lane[par].tile.p : nullptr;
    if (tiles)
        HIPCHK(c, launch_tile_detect(d_xyz, BatchRef{D.n_scans, D.n_blocks, ring.host_dev + at, nullptr},
                                     d_tile, c->ray_tiles > 0 ? (uint32_t)c->ray_tiles : 0u, st));
    if (prev) HIPCHK(c, hipStreamWaitEvent(st, c->ev_compact[par ^ 1], 0));  // before front: 1, 2
    c->ht.lap(HT_WAITS);
    // -- ring upload: the records -> the device ring slot
    HIPCHK(c, launch_upload(ring.host_dev + at, ds, (uint32_t)((D.n_scans + 1) * sizeof(ScanRec)),
                            ring.done_dev, seq + 1, st));
    c->ht.lap(HT_UPLOAD);
    const BatchRef B{D.n_scans, D.n_blocks, ds, d_tile};
    // -- pre-pass (MergedTsdfIntegrator): the batch's points bundled per (scan, voxel) first; the
    // walk kernels then read one ray per bundle, in the slot of its first point (tsdf_merged.hip)
    RayConst R = c->R;
    const float* d_rays = d_xyz;
    if (c->merged && D.n_blocks) {
        HIPCHK(c, launch_mg_prepass(d_xyz, B, D.n_blocks, D.s[D.n_scans].off, c->R, c->mg[par],
                                    &c->G->ctr[par].ovf, st));
        d_rays = c->mg[par].xyz_out;
        R.ray_w = c->mg[par].w_out;
    }
    // -- front end and compact.  A small batch (a live node's 1-8 scans) fuses wave-per-brick, in
    // table order (not k_compact's size order)
    const bool small = !c->plan.fused && D.n_scans <= (uint32_t)c->small_ns;
    const int k_front = c->plan.fused ? KIND_WALK : KIND_COUNT;
    const int k_back = c->plan.fused ? KIND_SPANS : KIND_PLACE;
    // per-kernel times: the two-walk kernels record their own dispatch timestamps (KTime, no
    // marker packets); the single walk's stages are bracketed by marker events
    auto kt = [&](int kind) { return tm && !c->plan.fused && tm->want(kind) ? tm->timing(kind) : KTime{}; };
    if (D.n_blocks) {
        if (tm && c->plan.fused) tm->begin(k_front, st);
        if (c->R.sec_on) HIPCHK(c, launch_sector_flags(d_rays, B, R, W, c->G, par, st));
        if (c->plan.fused) HIPCHK(c, launch_walk(d_rays, B, R, T, W, c->G, par, c->plan.nstep, st));
        else HIPCHK(c, launch_count(d_rays, B, R, T, W, c->G, par, st, kt(KIND_COUNT),
                                    !c->R.sec_on && D.n_blocks <= c->count_wide,
                                    !c->R.sec_on && c->count_paired));
        c->ht.lap(HT_FRONT);
        if (tm && c->plan.fused) tm->next(k_front, KIND_COMPACT, st);
        HIPCHK(c, launch_compact(B, T, W, c->G, par, c->plan.fused, st, kt(KIND_COMPACT)));
        c->ht.lap(HT_COMPACT);
    } else {  // no compaction: the record's pool count is taken here instead
        HIPCHK(c, launch_pool_mark(c->G, par, st));
    }
    if (cross && !lean) HIPCHK(c, hipEventRecord(c->ev_compact[par], st));  // after compact: 1
    // -- back end
    if (prev && lean) HIPCHK(c, hipStreamWaitEvent(st, c->ev_integ[par ^ 1], 0));  // before back: 2
    if (D.n_blocks) {
        if (tm && c->plan.fused) tm->next(KIND_COMPACT, k_back, st);
        if (c->plan.fused) HIPCHK(c, launch_spans(B, c->R, T, W, c->G, par, c->plan.nstep, st));
        else HIPCHK(c, launch_place(d_rays, B, R, T, W, c->G, par, st, kt(KIND_PLACE)));
        c->ht.lap(HT_BACK);
        if (tm && c->plan.fused) tm->end(k_back, st);
    }
    if (lean) HIPCHK(c, hipEventRecord(c->ev_compact[par], st));  // after back: 2
    // -- integrate
    if (prev && !lean) HIPCHK(c, hipStreamWaitEvent(st, c->ev_integ[par ^ 1], 0));  // before integrate: 1
    if (D.n_blocks) {
        if (tm && c->plan.fused) tm->begin(KIND_INTEGRATE, st);
        if (small) {
            HIPCHK(c, launch_integrate_small(B, c->R, T, W, c->Pl, c->G, par, st, kt(KIND_INTEGRATE)));
        } else {
            Work Wi = W;
            Wi.active = W.active_ord;  // largest bricks first (k_compact's size order)
            HIPCHK(c, launch_integrate(B, c->R, T, Wi, c->Pl, c->G, par, c->plan.fused, c->max_batch > 64, st,
                                       kt(KIND_INTEGRATE)));
        }
        if (tm && c->plan.fused) tm->end(KIND_INTEGRATE, st);
        c->ht.lap(HT_INTEGRATE);
    }
    // -- finish and the host's books
    HIPCHK(c, launch_finish(c->G, par, (uint32_t)c->batch_id, B, st));
    if (cross) {  // the batch's end: the other stream's next batches wait on it
        HIPCHK(c, hipEventRecord(ring.ev[slot], st));
        c->ev_integ[par] = ring.ev[slot];
    }
    if (c->can_grow) c->log.push_back({c->batch_id, d_xyz, D});
    for (int k = 0; k < 2; k++)  // a host batch: its staging buffer's last reader
        if (d_xyz == c->stage2[k]) {
            c->stage_reader[k] = c->batch_id;
            HIPCHK(c, hipEventRecord(c->stage_ev[k], st));
        }
    c->ht.lap(HT_FINISH);
    c->ht.n++;
    c->batch_id++;
    c->n_batches++;
    c->n_scans += D.n_scans;
    if (tm && tm->pending.size() > 8192) {
        HIPCHK(c, hipStreamSynchronize(c->bst[0]));
        HIPCHK(c, hipStreamSynchronize(c->bst[1]));
        tm->harvest();
    }
    return TSDF_OK;
}

// The context stream waits for every launched batch (read-outs, imports, sync).
static int join(tsdf_ctx* c) {
    if (c->batch_id == 0) return TSDF_OK;
    if (!c->p.pipeline) {  // serial batches: one stream, no per-batch marker; one now
        HIPCHK(c, hipEventRecord(c->ev_main, c->bst[0]));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_main, 0));
        return TSDF_OK;
    }
    for (int q = 0; q < 2; q++)
        if (c->batch_id > (uint64_t)q) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_integ[q], 0));
    return TSDF_OK;
}

// A fan-out follower's pending points, still in its leader's staging, copied into its own staging
// (device to device, xGMI between GPUs) after the leader's H2D copies; the leader's stream then
// waits for the copy, so the leader never rewrites that region first.  Leaves the current device
// as it found it.
static int fan_copy_range(tsdf_ctx* c, tsdf_ctx* s, float* dst, const float* src, uint64_t bytes) {
    int dev = 0;
    HIPCHK(c, hipGetDevice(&dev));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamWaitEvent(c->stream, s->bc_ev, 0));  // the leader's H2D copies so far
    HIPCHK(c, c->device == s->device
                  ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream)
                  : hipMemcpyPeerAsync(dst, c->device, src, s->device, bytes, c->stream));
    if (!c->bc_ev) HIPCHK(c, c->bc_ev.create());
    HIPCHK(c, hipEventRecord(c->bc_ev, c->stream));
    HIPCHK(s, hipSetDevice(s->device));
    HIPCHK(s, hipStreamWaitEvent(s->stream, c->bc_ev, 0));
    HIPCHK(c, hipSetDevice(dev));
    return TSDF_OK;
}

static int fan_copy(tsdf_ctx* c) {
    if (!c->fan_src || !c->fan_buf || c->fan_hi <= c->fan_lo) {
        c->fan_lo = c->fan_hi;
        return TSDF_OK;
    }
    const int rc = fan_copy_range(c, c->fan_src, c->stage2[c->pend_stage] + 3 * c->fan_lo,
                                  c->fan_buf + 3 * c->fan_lo, (c->fan_hi - c->fan_lo) * 12);
    c->fan_lo = c->fan_hi;
    return rc;
}

// Launch the queued host scans (integrate paths: no join, so batches keep overlapping).
static int flush(tsdf_ctx* c) {
    if (c->pend.n_scans == 0) return TSDF_OK;
    if (c->fan_src) {  // a fan-out follower: its points first
        const int rc = fan_copy(c);
        if (rc) return rc;
    }
    // the buffer the pending scans were staged into; a replay that runs inside launch() (metrics
    // drain, log bound) re-reads only logged batches, none of which uses this buffer any more
    const int rc = launch(c, c->stage2[c->pend_stage], c->pend);
    c->last_stage = c->pend_stage;
    c->pend.n_scans = 0;
    c->pend.s[0].off = 0;
    return rc;
}

// flush + make the context stream wait for every batch (read-out, import, sync paths)
static int settle(tsdf_ctx* c) {
    const int rc = flush(c);
    return rc ? rc : join(c);
}

// ---- capacity: brick pool, hash table and per-brick work lists -----------------

// Allocate (and clear: empty table, zero cells) the capacity-dependent buffers for max_bricks bricks;
// the pool's contents are the caller's.  Allocation failure is TSDF_ENOMEM; K frees what it got.
static int alloc_capacity(tsdf_ctx* c, uint64_t max_bricks, Capacity& K) {
    K = Capacity{};
    K.max_bricks = max_bricks;
    K.cap = next_pow2(2 * max_bricks);
    K.max_active = (uint32_t)std::min<uint64_t>(K.cap, c->plan.slots);
    const size_t cells = K.cap * c->plan.cell_stride * (c->plan.fused ? sizeof(uint64_t) : sizeof(uint32_t));
    hipError_t e = K.keys.alloc(K.cap);
    if (e == hipSuccess) e = K.slots.alloc(K.cap);
    if (e == hipSuccess) e = K.touched.alloc(K.cap);
    if (e == hipSuccess) e = K.brick_keys.alloc(max_bricks);
    if (e == hipSuccess) e = K.sdf.alloc(max_bricks * BRICK_VOX);
    if (e == hipSuccess) e = K.weight.alloc(max_bricks * BRICK_VOX);
    for (int q = 0; q < 2 && e == hipSuccess; q++) {
        e = K.cell[q].alloc_bytes(cells);
        if (e == hipSuccess) e = K.active[q].alloc(K.max_active);
        if (e == hipSuccess) e = K.active_ord[q].alloc(K.max_active);
        if (e == hipSuccess) e = K.cagg[q].alloc(compact_chunks(K.cap) * 2);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, TSDF_ENOMEM, "device allocation for %llu bricks failed",
                    (unsigned long long)max_bricks);
    }
    e = launch_fill_u64(K.keys, EMPTY_KEY, K.cap, c->stream);
    if (e == hipSuccess) e = launch_fill_u32(K.slots, UNASSIGNED, K.cap, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(K.touched, 0, K.cap * sizeof(uint32_t), c->stream);
    for (int q = 0; q < 2 && e == hipSuccess; q++) e = hipMemsetAsync(K.cell[q], 0, cells, c->stream);
    if (e != hipSuccess) return fail(c, TSDF_EHIP, "capacity init: %s", hipGetErrorString(e));
    return TSDF_OK;
}

// The kernels' argument structs, filled from the owners (c->K, c->lane): after create, after a
// new capacity is installed and after a list grew.  T.cell is the parity-0 cells; launch() passes
// a Table with its parity's.
static void set_views(tsdf_ctx* c) {
    const Capacity& K = c->K;
    c->T = Table{K.keys, K.slots, K.touched, K.cell[0], K.brick_keys, K.cap - 1,
                 (uint32_t)K.max_bricks, c->plan.cell_stride};
    c->Pl = Pool{K.sdf, K.weight};
    const uint64_t mg_cap = c->merged ? c->plan.batch_points : 0;
    for (int q = 0; q < 2; q++) {
        const Lane& L = c->lane[q];
        c->W2[q] = Work{L.pair, L.blk, L.blk_n, L.plan, L.fb, L.smp, K.active[q], K.active_ord[q],
                        L.ord_hist, K.cagg[q], L.act, L.spn, c->plan.maxp,
                        K.max_active, c->max_fb, c->max_smp, c->max_spn};
        c->mg[q] = MgBufs{L.mg_xyz, L.mg_w, mg_cap, L.mg_ekey, L.mg_eidx, L.mg_bcnt, L.mg_bst,
                          L.mg_bscan, mg_cap ? mg_buckets_max(mg_cap) : 0};
    }
}

// ---- the host's protocol with Globals (tsdf_device.h) --------------------------------------------

// The check word: Globals' first five fields, read in one copy; the clears span adjacent fields,
// and the reset after a grow (everything before tot_vox) takes the check word and both counters
struct GlobalsCheck { uint32_t pool_count, overflow, failed, retry, fail_id; };
static_assert(offsetof(Globals, pool_count) == 0 && offsetof(Globals, overflow) == 4 &&
              offsetof(Globals, failed) == 8 && offsetof(Globals, retry) == 12 &&
              offsetof(Globals, fail_id) == 16 && offsetof(Globals, ctr) < offsetof(Globals, tot_vox),
              "the host reads and clears Globals' head by these offsets");
// Zero `words` adjacent u32 fields from `first` on
static hipError_t globals_clear(uint32_t* first, int words) {
    const uint32_t z[3] = {0u, 0u, 0u};
    return hipMemcpy(first, z, 4 * words, hipMemcpyHostToDevice);
}

// Grow the pool (and table, cells, lists) to hold at least `need` bricks: x2 or more, capped by
// max_bricks_hard.  Every batch must be complete.  The pool keeps its bricks (same slots); the
// table is rebuilt from the slot -> key map.  TSDF_ENOMEM: no growth possible.
static int grow_capacity(tsdf_ctx* c, uint64_t need) {
    const uint64_t old = c->T.max_bricks;
    uint64_t nb = std::max<uint64_t>(2 * old, need + need / 4);
    if (c->p.max_bricks_hard) nb = std::min<uint64_t>(nb, c->p.max_bricks_hard);
    nb = std::min<uint64_t>(nb, 0xFFFFFFEFull);
    if (nb <= old) return fail(c, TSDF_ENOMEM, "brick pool at its hard limit (%llu bricks)",
                               (unsigned long long)old);
    uint32_t pc = 0;
    HIPCHK(c, hipMemcpy(&pc, &c->G->pool_count, 4, hipMemcpyDeviceToHost));
    const uint64_t valid = std::min<uint64_t>(pc, old);
    Capacity K;  // (freed with this scope if it is not installed)
    int rc = alloc_capacity(c, nb, K);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    if (valid) {
        e = hipMemcpyAsync(K.sdf, c->Pl.sdf, valid * BRICK_VOX * 4, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(K.weight, c->Pl.weight, valid * BRICK_VOX * 4, hipMemcpyDeviceToDevice,
                               c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(K.brick_keys, c->T.brick_keys, valid * 8, hipMemcpyDeviceToDevice,
                               c->stream);
    }
    if (e == hipSuccess) e = launch_fill(K.sdf + valid * BRICK_VOX, c->R.bg, (nb - valid) * BRICK_VOX, c->stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(K.weight + valid * BRICK_VOX, 0, (nb - valid) * BRICK_VOX * 4, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // the old pool is read before the free
    if (e != hipSuccess) return fail(c, TSDF_EHIP, "grow: %s", hipGetErrorString(e));
    c->K = std::move(K);  // installed: the old buffers are freed
    set_views(c);
    HIPCHK(c, launch_rehash(c->T, (uint32_t)valid, c->G, c->stream));
    // the failed batches' counters and flags go; the pool keeps its valid bricks; retry stays on
    const uint32_t pcv = (uint32_t)valid, retry = 1u;
    HIPCHK(c, hipMemsetAsync(c->G, 0, offsetof(Globals, tot_vox), c->stream));
    HIPCHK(c, hipMemcpyAsync(&c->G->pool_count, &pcv, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(&c->G->retry, &retry, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->n_grows++;
    return TSDF_OK;
}

// Double one of the work lists in both batch parities, up to `limit` entries of `bytes` each.
// `counted`: the growth shows in tsdf_get_stats' n_grows (the fallback pairs' never has).
template <class T>
static int grow_list(tsdf_ctx* c, DevBuf<T> Lane::*list, uint32_t tsdf_ctx::*max, uint64_t limit,
                     size_t bytes, const char* what, bool counted) {
    const uint64_t n = std::min<uint64_t>(2ull * (c->*max), limit);
    if (n <= c->*max) return fail(c, TSDF_ENOMEM, "%s at its limit", what);
    DevBuf<T> f[2];
    hipError_t e = f[0].alloc_bytes(n * bytes);
    if (e == hipSuccess) e = f[1].alloc_bytes(n * bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, TSDF_ENOMEM, "%s allocation failed", what);
    }
    for (int q = 0; q < 2; q++) c->lane[q].*list = std::move(f[q]);  // frees the old list
    c->*max = (uint32_t)n;
    set_views(c);
    if (counted) c->n_grows++;
    return TSDF_OK;
}

// Every launched batch complete: the context stream waits for them and drains.
static int drain_all(tsdf_ctx* c) {
    int rc = join(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TSDF_OK;
}

// Replay logged batches in order (their inputs are still valid); every batch complete on return.
static int replay(tsdf_ctx* c, const tsdf_ctx::Logged* first, size_t n) {
    int rc = TSDF_OK;
    c->in_replay = true;
    for (size_t j = 0; j < n && !rc; j++) {
        tsdf_ctx::Logged L = first[j];
        c->n_scans -= L.D.n_scans;
        c->n_batches--;
        c->n_replayed++;
        rc = launch(c, L.xyz, L.D);
    }
    c->in_replay = false;
    return rc ? rc : drain_all(c);
}

// With every batch complete: if a batch overflowed, grow the capacity it lacked and re-run the
// batches from it (their inputs are still valid), until a round succeeds.  Without growth (hard
// limit, or a non-growable overflow) the batches are re-run committing what fits, and tsdf_sync
// reports the overflow.  A Merged batch with more distinct keys in a bucket than its LDS table
// holds (OVF_MG) lacks no capacity of the context: that batch alone is re-run committing what fits
// and reported by tsdf_sync; the context keeps growing for the batches after it.
static int check_and_replay(tsdf_ctx* c) {
    for (int round = 0; round < 64; round++) {
        GlobalsCheck g;
        HIPCHK(c, hipMemcpy(&g, c->G, sizeof g, hipMemcpyDeviceToHost));
        if (!g.failed) {
            c->log.clear();
            return TSDF_OK;
        }
        if (!c->can_grow) {  // committed anyway (G->retry = 0): the overflow stays for tsdf_sync
            HIPCHK(c, globals_clear(&c->G->failed, 1));
            c->log.clear();
            return TSDF_OK;
        }
        // the replay: from the first failed batch on, in order
        size_t first = 0;
        while (first < c->log.size() && (uint32_t)c->log[first].id != g.fail_id) first++;
        if (first == c->log.size()) first = 0;
        std::vector<tsdf_ctx::Logged> rep(c->log.begin() + first, c->log.end());
        c->log.clear();
        if (g.overflow == OVF_MG && !rep.empty()) {
            // nothing to grow (every growable flag of an earlier round was cleared with its
            // growth, so the first failed batch raised OVF_MG and nothing else): that batch with
            // retry off, its flags kept on the host for tsdf_sync, then the others with retry on
            HIPCHK(c, globals_clear(&c->G->overflow, 3));  // overflow, failed, retry
            int rc = replay(c, rep.data(), 1);
            if (rc) return rc;
            uint32_t ovf = 0;
            HIPCHK(c, hipMemcpy(&ovf, &c->G->overflow, sizeof ovf, hipMemcpyDeviceToHost));
            c->ovf_refused |= ovf;
            const uint32_t on[3] = {0u, 0u, 1u};  // overflow, failed, retry
            HIPCHK(c, hipMemcpy(&c->G->overflow, on, sizeof on, hipMemcpyHostToDevice));
            c->log.clear();
            rc = replay(c, rep.data() + 1, rep.size() - 1);
            if (rc) return rc;
            continue;
        }
        int rc = TSDF_ENOMEM;
        // pair slots per ray are a geometric bound: not a capacity to grow
        if (!(g.overflow & OVF_PAIRS)) {
            rc = TSDF_OK;
            if (g.overflow & (OVF_TABLE | OVF_POOL | OVF_ACTIVE))
                rc = grow_capacity(c, std::max<uint64_t>(g.pool_count, c->T.max_bricks + 1));
            // fallback pairs: up to the 26-bit index space (never counted in n_grows); samples: up
            // to the 32-bit sample index (single walk: the span record's 30-bit sample position)
            if (rc == TSDF_OK && (g.overflow & OVF_FB))
                rc = grow_list(c, &Lane::fb, &tsdf_ctx::max_fb, 1ull << 26, sizeof(uint4),
                               "fallback pair list", false);
            if (rc == TSDF_OK && (g.overflow & OVF_SMP))
                rc = grow_list(c, &Lane::smp, &tsdf_ctx::max_smp,
                               c->plan.fused ? (1ull << 30) : 0xFFFFFFF0ull, smp_bytes(c->R.sem),
                               "sample list", true);
            if (rc == TSDF_OK && (g.overflow & OVF_SPN))
                rc = grow_list(c, &Lane::spn, &tsdf_ctx::max_spn, 0xFFFFFFF0ull, sizeof(uint32_t),
                               "span list", true);
            if (rc == TSDF_EHIP) return rc;
        }
        if (rc != TSDF_OK) {  // cannot grow: commit what fits from now on
            c->can_grow = false;
            HIPCHK(c, globals_clear(&c->G->failed, 2));  // failed, retry
        } else {  // grown: the replay re-raises whatever still does not fit
            HIPCHK(c, globals_clear(&c->G->overflow, 2));  // overflow, failed
        }
        rc = replay(c, rep.data(), rep.size());
        if (rc) return rc;
    }
    return fail(c, TSDF_ENOMEM, "capacity growth did not converge");
}

// Metrics log: one JSON line per finished batch, from the device ring of batch records (k_finish)
// and the host's facts (points) and kernel times (profiling on).  Called with every batch done.
static int emit_metrics(tsdf_ctx* c) {
    if (!c->metrics) return TSDF_OK;
    if (c->timer) c->timer->harvest();
    const uint64_t end = c->batch_id;
    if (end == c->metrics_next) return TSDF_OK;
    std::vector<BatchRecord> ring(METRIC_RING);
    HIPCHK(c, hipMemcpy(ring.data(), c->G->ring, sizeof(BatchRecord) * METRIC_RING,
                        hipMemcpyDeviceToHost));
    size_t ti = 0;
    for (uint64_t b = std::max<uint64_t>(c->metrics_next, end > METRIC_RING ? end - METRIC_RING : 0);
         b < end; b++) {
        const BatchRecord& r = ring[b % METRIC_RING];
        if (r.batch_id != (uint32_t)b) continue;  // not written (ring wrapped)
        uint32_t scans = 0;
        uint64_t points = 0;
        for (auto& i : c->metrics_info)
            if (i.id == b) { scans = i.scans; points = i.points; }
        const double bytes = 12.0 * (double)r.rays + 16.0 * (double)r.vox;  // SURVEY §8d B_scan
        fprintf(c->metrics,
                "{\"batch\": %llu, \"scans\": %u, \"points\": %llu, \"rays\": %llu, \"pairs\": %llu, "
                "\"voxel_updates\": %llu, \"dirty_voxels\": %llu, \"active_bricks\": %u, "
                "\"new_bricks\": %u, \"bricks\": %u, \"overflow\": %u, \"committed\": %s, "
                "\"tiled_scans\": %u, \"algorithmic_bytes\": %.0f",
                (unsigned long long)b, scans, (unsigned long long)points,
                (unsigned long long)r.rays, (unsigned long long)r.pairs, (unsigned long long)r.vox,
                (unsigned long long)r.dirty, r.n_active, r.n_new,
                std::min<uint32_t>(r.pool_count, c->T.max_bricks), r.ovf,
                r.committed ? "true" : "false", r.tiled, bytes);
        const std::array<double, KIND_N>* ms = nullptr;
        if (c->timer) {
            auto& bm = c->timer->batch_ms;
            while (ti < bm.size() && bm[ti].first < b) ti++;
            if (ti < bm.size() && bm[ti].first == b) ms = &bm[ti].second;
        }
        if (ms) {
            double path = 0;
            for (int k = 0; k < KIND_N; k++) path += (*ms)[k];
            if (c->plan.fused)
                fprintf(c->metrics,
                        ", \"kernel_ms\": {\"walk\": %.5f, \"compact\": %.5f, \"spans\": %.5f, "
                        "\"integrate\": %.5f}",
                        (*ms)[KIND_WALK], (*ms)[KIND_COMPACT], (*ms)[KIND_SPANS], (*ms)[KIND_INTEGRATE]);
            else
                fprintf(c->metrics,
                        ", \"kernel_ms\": {\"count\": %.5f, \"compact\": %.5f, \"place\": %.5f, "
                        "\"integrate\": %.5f}",
                        (*ms)[KIND_COUNT], (*ms)[KIND_COMPACT], (*ms)[KIND_PLACE], (*ms)[KIND_INTEGRATE]);
            fprintf(c->metrics, ", \"path_ms\": %.5f, \"gbs\": %.2f", path,
                    path > 0 ? bytes / (path * 1e-3) / 1e9 : 0.0);
        }
        fprintf(c->metrics, "}\n");
    }
    fflush(c->metrics);
    c->metrics_next = end;
    c->metrics_info.clear();
    if (c->timer) c->timer->batch_ms.clear();
    return TSDF_OK;
}

// Marching-cubes case table, generated (the same construction as the oracle's
// mc_build): per cube face the sign-change edges are paired into segments (ambiguous faces pair the
// crossings around their inside corners, so neighbouring cubes agree), each directed with the
// face's inside corners (S < 0) on its right seen from outside; the segments chain into cycles,
// fanned into triangles.  Corner c = (c & 1, c >> 1 & 1, c >> 2 & 1); edges axis-major.
struct McTable {
    uint8_t tab[256][32];  // [case][0] = triangles, then 3 edge ids each
    uint8_t edge[12][2];   // edge -> (a, b), b = a | axis bit
};

// lorensen: the classic table's ambiguity rule instead (Lorensen & Cline's complement symmetry;
// TSDF_MC_LORENSEN_RULE, a restatement of the published table's topology): an ambiguous face pairs its crossings
// around the inside corners when at most 4 corners of the cube are inside, around the outside
// corners otherwise; the two cubes sharing a face can then disagree (the classic cracks).
static McTable build_mc_table(bool lorensen) {
    McTable M{};
    int ne = 0;
    for (int d = 0; d < 3; d++)
        for (int base = 0; base < 8; base++)
            if (!(base & (1 << d))) {
                M.edge[ne][0] = (uint8_t)base;
                M.edge[ne][1] = (uint8_t)(base | (1 << d));
                ne++;
            }
    auto edge_of = [&](int a, int b) {
        for (int e = 0; e < 12; e++)
            if ((M.edge[e][0] == a && M.edge[e][1] == b) || (M.edge[e][0] == b && M.edge[e][1] == a))
                return e;
        return -1;
    };
    for (int k = 0; k < 256; k++) {
        int next[12];
        std::fill(next, next + 12, -1);
        for (int d = 0; d < 3; d++) {
            const int u = (d + 1) % 3, w = (d + 2) % 3;
            for (int side = 0; side < 2; side++) {
                // face corners counter-clockwise seen from outside (outward normal (2 side - 1) e_d)
                const int ou[4] = {0, 1, 1, 0}, ow[4] = {0, 0, 1, 1};
                int q[4], in[4];
                for (int i = 0; i < 4; i++) {
                    const int cu = side ? ou[i] : ow[i], cw = side ? ow[i] : ou[i];
                    q[i] = (side << d) | (cu << u) | (cw << w);
                    in[i] = (k >> q[i]) & 1;
                }
                int cr[4], ncr = 0;
                for (int i = 0; i < 4; i++)
                    if (in[i] != in[(i + 1) & 3]) cr[ncr++] = i;
                std::vector<std::pair<int, int>> pairs;
                if (ncr == 2) pairs.push_back({cr[0], cr[1]});
                if (ncr == 4) {
                    // around the inside corners (generated; Lorensen with <= 4 inside corners), else
                    // around the outside ones
                    const bool around_in = !lorensen || __builtin_popcount((unsigned)k) <= 4;
                    if (in[0] == (around_in ? 1 : 0)) pairs = {{3, 0}, {1, 2}};
                    else pairs = {{0, 1}, {2, 3}};
                }
                for (auto [i, j] : pairs) {
                    const int ei = edge_of(q[i], q[(i + 1) & 3]), ej = edge_of(q[j], q[(j + 1) & 3]);
                    // the corners q[i+1 .. j] are on the right of the segment i -> j
                    if (in[(i + 1) & 3]) next[ei] = ej;
                    else next[ej] = ei;
                }
            }
        }
        bool used[12] = {};
        int nt = 0;
        for (int e0 = 0; e0 < 12; e0++) {
            if (next[e0] < 0 || used[e0]) continue;
            int poly[12], n = 0;
            for (int e = e0; !used[e] && n < 12; e = next[e]) {
                used[e] = true;
                poly[n++] = e;
            }
            for (int m = 1; m + 1 < n; m++) {
                M.tab[k][1 + 3 * nt] = (uint8_t)poly[0];
                M.tab[k][2 + 3 * nt] = (uint8_t)poly[m];
                M.tab[k][3 + 3 * nt] = (uint8_t)poly[m + 1];
                nt++;
            }
        }
        M.tab[k][0] = (uint8_t)nt;
    }
    return M;
}

// TSDF_MC_LORENSEN: the published table (include/tsdf_mc_tables.h, VDBFusion's), renumbered into
// this library's corners and edges: Bourke vertex v -> corner kV[v], edge e -> edge kE[e]; the
// triangles keep their order and winding.
static McTable literal_mc_table() {
    McTable M = build_mc_table(false);  // the edge list
    static const int kV[8] = {0, 1, 3, 2, 4, 5, 7, 6};
    static const int kE[12] = {0, 5, 1, 4, 2, 7, 3, 6, 8, 9, 11, 10};
    for (int b = 0; b < 256; b++) {
        int k = 0;
        for (int v = 0; v < 8; v++)
            if (b >> v & 1) k |= 1 << kV[v];
        int nt = 0;
        for (int i = 0; i < 15 && tsdf_mc_tri_table[b][i] >= 0; i += 3, nt++)
            for (int j = 0; j < 3; j++) M.tab[k][1 + 3 * nt + j] = (uint8_t)kE[tsdf_mc_tri_table[b][i + j]];
        M.tab[k][0] = (uint8_t)nt;
    }
    return M;
}

static const McTable& mc_table(int which = TSDF_MC_GENERATED) {
    static const McTable G = build_mc_table(false), L = literal_mc_table(), R = build_mc_table(true);
    return which == TSDF_MC_LORENSEN ? L : which == TSDF_MC_LORENSEN_RULE ? R : G;
}

extern "C" {

void tsdf_default_params(tsdf_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->voxel_size = 0.05;
    p->sdf_trunc = 0.15;
    p->space_carving = 0;
    p->weight_mode = TSDF_WEIGHT_CONSTANT;
    p->min_range = 0.0;
    p->max_range = INFINITY;
    p->max_bricks = 1u << 20;
    p->max_points = 1u << 18;
    p->max_pairs = 0;
    p->device_id = 0;
    p->brick_side = TSDF_BRICK_SIDE;
    p->max_batch = 32;
    p->semantics = TSDF_SEM_VDBFUSION_F64;  // ABI v8: the mode matching VDBFusion exactly
    p->voxblox_method = TSDF_VB_SIMPLE;
    p->sector_input = TSDF_SECTOR_INPUT_FANOUT;
    p->sector_rule = TSDF_SECTOR_RULE_INDEX;  // ABI v10: SURVEY §8e's contiguous column sectors
    p->allow_clear = 1;  // voxblox TsdfIntegratorBase::Config defaults
    p->use_weight_dropoff = 1;
    p->max_weight = 10000.0f;
    p->depth_weight = 1;  // voxblox use_const_weight = false (upstream's default)
}

int tsdf_abi_version(void) { return TSDF_ABI_VERSION; }

const char* tsdf_last_error(const tsdf_ctx* c) { return c ? c->err.c_str() : "null context"; }

// In order: the fan-out links go, the pending work settles, the streams drain, and the context's
// owners free what they hold (a half-built context's empty owners free nothing).
void tsdf_destroy(tsdf_ctx* c) {
    if (!c) return;
    // fan-out links (tsdf_integrate_sectors): a leader hands its followers their pending points
    // before its staging goes; a follower leaves its leader's list
    for (tsdf_ctx* f : c->fan_followers) {
        (void)fan_copy(f);
        f->fan_src = nullptr;
        f->fan_buf = nullptr;
    }
    c->fan_followers.clear();
    if (c->fan_src) {
        auto& v = c->fan_src->fan_followers;
        v.erase(std::remove(v.begin(), v.end(), c), v.end());
    }
    if (c->device >= 0) {
        (void)hipSetDevice(c->device);
        if (c->stream) {
            (void)settle(c);
            (void)hipStreamSynchronize(c->stream);
            for (int q = 0; q < 2; q++)
                if (c->bst[q]) (void)hipStreamSynchronize(c->bst[q]);
        }
    }
    if (c->metrics) fclose(c->metrics);
    delete c->timer;
    delete c->pack;
    delete c;  // the owners free what they hold
}

// The ray model's constants, derived from the params
static RayConst ray_const(const tsdf_params& p, int band_vox) {
    RayConst R{};
    R.vs = (float)p.voxel_size;
    R.inv_vs = 1.0f / R.vs;
    R.tau = (float)p.sdf_trunc;
    R.min_range = (float)p.min_range;
    R.max_range = (float)p.max_range;
    R.carving = p.space_carving ? 1 : 0;
    R.tau2_lo = (float)(((double)R.tau * (1.0 - 0x1p-20)) * ((double)R.tau * (1.0 - 0x1p-20)));
    R.tau2_hi = (float)(((double)R.tau * (1.0 + 0x1p-20)) * ((double)R.tau * (1.0 + 0x1p-20)));
    // internal sem 3: Voxblox with per-sample weights (the 1/z^2 weight, stored by k_place; the
    // merged integrator's bundles, which carry summed weights)
    R.depth_w = p.semantics == TSDF_SEM_VOXBLOX && p.depth_weight ? 1 : 0;
    R.sem = plan_sem(p);
    // (ray_w stays null: set per launch to the pre-pass output, merged)
    R.allow_clear = p.allow_clear ? 1 : 0;
    R.dropoff = p.use_weight_dropoff ? 1 : 0;
    R.max_weight = p.max_weight;
    R.w0_cap = p.max_weight > 0.0f && p.max_weight < TSDF_W0_CAP ? p.max_weight : TSDF_W0_CAP;
    R.bg = p.semantics == TSDF_SEM_VOXBLOX ? 0.0f : R.tau;
    R.tau_m_vs = R.tau - R.vs;
    // TSDF_SECTOR_RULE_INDEX: the context takes an index share; the kernels' azimuth filter is off
    if (!(p.n_sectors > 1 && p.sector_rule == TSDF_SECTOR_RULE_INDEX))
        sector_bounds(p.sector_yaw0, p.sector, p.n_sectors, R);
    const double vs_d = (double)R.vs;  // VDBVolume keeps voxel_size as float
    R.hvs_d = vs_d * 0.5;              // exact
    R.inv_s_d = 1.0 / vs_d;
    R.gate_d2 = gate_threshold(R.tau);
    R.band_vox = band_vox;
    return R;
}

// Three steps: the ray constants, the sizing plan (ctx_plan.h), the allocations.
static int create_impl(tsdf_ctx* c, const tsdf_params* p) {
    c->p = *p;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(c, TSDF_ENODEV, "no HIP device available");
    if (p->device_id < 0 || p->device_id >= ndev)
        return fail(c, TSDF_EINVAL, "device_id %d out of range (%d devices)", p->device_id, ndev);
    c->device = p->device_id;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->stream.create());
    for (int q = 0; q < 2; q++) {
        HIPCHK(c, c->bst[q].create());
        HIPCHK(c, c->ev_compact[q].create());
        HIPCHK(c, c->stage_ev[q].create());
    }
    HIPCHK(c, c->ev_main.create());

    c->plan = ctx_plan(*p, PlanConsts{RPB, MAX_BATCH, WLK_THREADS, SPAN, VOX_LIMIT});
    if (!c->plan.refusal.empty()) return fail(c, TSDF_EINVAL, "%s", c->plan.refusal.c_str());
    c->R = ray_const(*p, c->plan.band_vox);
    c->merged = plan_merged(*p);
    c->idx_rule = p->n_sectors > 1 && p->sector_rule == TSDF_SECTOR_RULE_INDEX;
    c->max_points = p->max_points;
    c->max_batch = p->max_batch;
    c->max_fb = c->plan.max_fb;
    c->max_smp = c->plan.max_smp;
    c->max_spn = c->plan.max_spn;

    for (int q = 0; q < 2; q++) {  // one set per batch parity (capacity-independent part)
        Lane& L = c->lane[q];
        HIPCHK(c, L.pair.alloc(c->plan.fused ? 4 : c->plan.slots));
        HIPCHK(c, L.blk.alloc((size_t)c->plan.max_blocks * 2 * HCAP));
        HIPCHK(c, L.blk_n.alloc((size_t)c->plan.max_blocks * 2));
        HIPCHK(c, L.plan.alloc((size_t)c->plan.max_blocks * 2 * PLAN_STRIDE));
        HIPCHK(c, L.fb.alloc(c->max_fb));
        HIPCHK(c, L.smp.alloc_bytes((size_t)c->max_smp * smp_bytes(c->R.sem)));
        HIPCHK(c, L.spn.alloc(c->max_spn));
        // (slice, size class) histogram, then first positions (k_compact; zero between batches)
        HIPCHK(c, L.ord_hist.alloc(2 * 64 * 32));
        HIPCHK(c, hipMemset(L.ord_hist, 0, 2 * 64 * 32 * sizeof(uint32_t)));
        HIPCHK(c, L.act.alloc(c->plan.max_blocks));
        HIPCHK(c, L.tile.alloc(c->max_batch));
        HIPCHK(c, c->stage2[q].alloc(c->plan.batch_points * 3));
        if (c->merged) {  // the bundling pre-pass: one set per parity, batch_points entries
            const uint64_t n = c->plan.batch_points, nb = mg_buckets_max(n);
            HIPCHK(c, L.mg_ekey.alloc(n));
            HIPCHK(c, L.mg_eidx.alloc(n));
            HIPCHK(c, L.mg_bcnt.alloc(MG_REPLICAS * nb));
            HIPCHK(c, hipMemset(L.mg_bcnt, 0, 4 * MG_REPLICAS * nb));  // zero between batches
            HIPCHK(c, L.mg_bst.alloc(nb + 1));
            HIPCHK(c, L.mg_bscan.alloc(nb));
            HIPCHK(c, L.mg_xyz.alloc(n * 3));
            HIPCHK(c, L.mg_w.alloc(n));
        }
    }
    HIPCHK(c, c->G.alloc(1));
    if (const char* e = std::getenv("TSDF_SMALL_NS")) c->small_ns = std::max(0, std::min(8, std::atoi(e)));
    if (const char* e = std::getenv("TSDF_COUNT_WIDE")) c->count_wide = (uint32_t)std::max(0, std::atoi(e));
    if (const char* e = std::getenv("TSDF_COUNT_PAIRED")) c->count_paired = std::atoi(e) != 0;
    if (const char* e = std::getenv("TSDF_RAY_TILES")) {
        const int h = std::atoi(e);
        c->ray_tiles = h == 64 || h == 128 || h == 256 ? h : 0;
    }
    // host staging threads: 3 workers + the caller (TSDF_PACK_THREADS overrides; 1 = none)
    int nt = 4;
    if (const char* e = std::getenv("TSDF_PACK_THREADS")) nt = std::max(1, std::atoi(e));
    nt = std::min<int>(nt, (int)std::max(1u, std::thread::hardware_concurrency()));
    if (nt > 1) {
        try {
            c->pack = new PackPool(nt - 1);
        } catch (...) {  // no threads: the caller's thread stages alone
            c->pack = nullptr;
        }
    }
    HIPCHK(c, c->ring.create());
    HIPCHK(c, hipMemsetAsync(c->G, 0, sizeof(Globals), c->stream));
    // the brick pool, hash table and per-brick work lists (grown later by grow_capacity)
    Capacity K;
    if (const int rc = alloc_capacity(c, p->max_bricks, K)) return rc;
    HIPCHK(c, launch_fill(K.sdf, c->R.bg, p->max_bricks * BRICK_VOX, c->stream));
    HIPCHK(c, hipMemsetAsync(K.weight, 0, p->max_bricks * BRICK_VOX * sizeof(float), c->stream));
    c->K = std::move(K);  // installed
    set_views(c);
    for (int i = 0; i < 2; i++) {
        HIPCHK(c, c->h_stage[i].alloc(c->max_points * 3));
        HIPCHK(c, c->stage_done[i].create());
    }
    c->can_grow = p->max_bricks_hard == 0 || p->max_bricks_hard > p->max_bricks;
    const uint32_t retry = c->can_grow ? 1u : 0u;
    HIPCHK(c, hipMemcpyAsync(&c->G->retry, &retry, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    static uint8_t all[TSDF_MC_TABLES][256][32];
    for (int t = 0; t < TSDF_MC_TABLES; t++) std::memcpy(all[t], mc_table(t).tab, sizeof all[t]);
    HIPCHK(c, upload_mc_table(all, mc_table().edge));
    return TSDF_OK;
}

int tsdf_create(const tsdf_params* p, tsdf_ctx** out) {
    if (!p || !out) return TSDF_EINVAL;
    *out = nullptr;
    if (!params_valid(*p)) return TSDF_EINVAL;
    tsdf_ctx* c = new (std::nothrow) tsdf_ctx();
    if (!c) return TSDF_ENOMEM;
    const int rc = create_impl(c, p);
    if (rc != TSDF_OK) {
        fprintf(stderr, "tsdf_create: %s\n", c->err.c_str());
        tsdf_destroy(c);
        return rc;
    }
    *out = c;
    return TSDF_OK;
}

// A scan's ray origin and sensor z axis (the world frame's z axis unless a pose gives it)
struct ScanPose {
    double o[3];
    float z[3];
};

// An origin without an orientation: the zero axis tells the walk to use Voxblox's constant weight
// (the 1/z^2 weight needs the sensor axis, which only the pose entry points carry)
static ScanPose pose_of_origin(const double o[3]) {
    return ScanPose{{o[0], o[1], o[2]}, {0.0f, 0.0f, 0.0f}};
}

// pose = (x, y, z, qx, qy, qz, qw): the z axis is the third column of the rotation of the
// normalised quaternion, computed in double and rounded to float (the oracle does the same)
static ScanPose pose_of(const double q[7]) {
    ScanPose P = pose_of_origin(q);
    const double n = std::sqrt(q[3] * q[3] + q[4] * q[4] + q[5] * q[5] + q[6] * q[6]);
    const double x = q[3] / n, y = q[4] / n, z = q[5] / n, w = q[6] / n;
    P.z[0] = (float)(2.0 * (x * z + w * y));
    P.z[1] = (float)(2.0 * (y * z - w * x));
    P.z[2] = (float)(1.0 - 2.0 * (x * x + y * y));
    return P;
}

static void set_pose(BatchDesc& D, uint32_t s, const ScanPose& P) {
    D.s[s].ox = (float)P.o[0];
    D.s[s].oy = (float)P.o[1];
    D.s[s].oz = (float)P.o[2];
    D.s[s].odx = P.o[0];
    D.s[s].ody = P.o[1];
    D.s[s].odz = P.o[2];
    D.s[s].zx = P.z[0];
    D.s[s].zy = P.z[1];
    D.s[s].zz = P.z[2];
}

// A caller's row-major 3x4 pose as the kernels take it (a null pose: unused, zeros)
static OsPose os_pose(const double pose[12]) {
    OsPose P{};
    if (pose)
        for (int k = 0; k < 12; k++) P.m[k] = (float)pose[k];
    return P;
}

// The pending batch's device staging buffer (host and single device scans are queued there).  A
// new pending batch takes the buffer the last launched host batch did not use; that buffer's
// previous reader must be complete and, with growth possible, committed: an overflowed batch is
// re-run from its logged input, so that input stays until then.
static int pend_stage_buffer(tsdf_ctx* c) {
    if (c->pend.n_scans != 0) return TSDF_OK;
    const int k = c->last_stage ^ 1;
    for (tsdf_ctx* f : c->fan_followers)  // fan-out followers still reading buffer k copy first
        if (f->fan_buf == c->stage2[k] && f->fan_hi > f->fan_lo) {
            const int rc = fan_copy(f);
            if (rc) return rc;
        }
    if (c->stage_reader[k] != ~0ull) {
        if (c->can_grow) {
            HIPCHK(c, hipEventSynchronize(c->stage_ev[k]));
            uint32_t failed = 0;
            HIPCHK(c, hipMemcpy(&failed, &c->G->failed, 4, hipMemcpyDeviceToHost));
            if (failed) {  // replays re-read stage2[k]: it is written only after them
                int rc = drain_all(c);
                if (!rc) rc = check_and_replay(c);
                if (rc) return rc;
            } else {  // every batch up to stage2[k]'s reader committed
                const uint64_t done = c->stage_reader[k];
                size_t j = 0;
                while (j < c->log.size() && c->log[j].id <= done) j++;
                c->log.erase(c->log.begin(), c->log.begin() + j);
            }
        }
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->stage_ev[k], 0));
    }
    c->pend_stage = k;
    return TSDF_OK;
}

// Append a staged scan of n points seen from pose P to the pending batch; launch it when full.
static int pend_push(tsdf_ctx* c, uint64_t n, const ScanPose& P) {
    BatchDesc& D = c->pend;
    const uint32_t s = D.n_scans;
    set_pose(D, s, P);
    D.s[s].xoff = 0;  // staged scans are contiguous
    D.s[s + 1].off = D.s[s].off + (uint32_t)n;
    D.n_scans = s + 1;
    c->n_points_in += n;
    if (D.n_scans == c->max_batch) return flush(c);
    return TSDF_OK;
}

// Room for a scan of n points in the pending batch (flushing it first if needed).
static int pend_room(tsdf_ctx* c, uint64_t n) {
    if (c->pend.n_scans == c->max_batch || c->pend.s[c->pend.n_scans].off + n > c->plan.batch_points)
        return flush(c);
    return TSDF_OK;
}

// TSDF_SECTOR_RULE_INDEX (ABI v10): sector k of N holds points
// [floor(k n / N), floor((k + 1) n / N)) of an n-point cloud -- contiguous column ranges of the
// spin for DLIO's time-sorted cloud (odom.cc:635-636).  The oracle's idx_share is the same.
static void idx_share(const tsdf_ctx* c, uint64_t n, uint64_t& lo, uint64_t& hi) {
    if (!c->idx_rule) {
        lo = 0;
        hi = n;
        return;
    }
    const unsigned __int128 N = c->p.n_sectors, k = c->p.sector;
    lo = (uint64_t)((unsigned __int128)n * k / N);
    hi = (uint64_t)((unsigned __int128)n * (k + 1) / N);
}

// ---- host-pointer input: a packer (host_pack.h pack_xyz), a scheduler (run_parts
// over the contexts' staging pools) and a stager (stage_acquire / stage_commit) ------------------

// The argument rules the host-pointer entry points share
static RecordView records_of(const void* pts, uint32_t point_step, uint32_t xyz_offset,
                             int32_t xyz_is_f64) {
    return RecordView{static_cast<const char*>(pts), point_step, xyz_offset, xyz_is_f64 != 0};
}

static int check_layout(tsdf_ctx* c, const RecordView& V) {
    return V.layout_ok() ? TSDF_OK : fail(c, TSDF_EINVAL, "point_step/xyz_offset inconsistent");
}

// pose = (x, y, z, qx, qy, qz, qw): the quaternion need not be normalised, only finite and nonzero
static bool quat_ok(const double pose[7]) {
    const double qn = pose[3] * pose[3] + pose[4] * pose[4] + pose[5] * pose[5] + pose[6] * pose[6];
    return qn > 0.0 && std::isfinite(qn);
}

// A free pinned staging buffer (*hb, at *h) for a scan of n points: room in the pending batch
// (launching it first if needed), then the buffer whose previous copy to the device is complete.
static int stage_acquire(tsdf_ctx* c, uint64_t n, int* hb, float** h) {
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = pend_room(c, n);
    if (rc) return rc;
    *hb = c->stage_cur;
    c->stage_cur ^= 1;
    HIPCHK(c, hipEventSynchronize(c->stage_done[*hb]));
    *h = c->h_stage[*hb];
    return TSDF_OK;
}

// The n points packed into h (stage_acquire's buffer hb) go to the device and join the pending
// batch as a scan seen from P, on the current device.
static int stage_commit(tsdf_ctx* c, int hb, const float* h, uint64_t n, const ScanPose& P) {
    const int rc = pend_stage_buffer(c);
    if (rc) return rc;
    if (n)
        HIPCHK(c, hipMemcpyAsync(c->stage2[c->pend_stage] + 3 * (uint64_t)c->pend.s[c->pend.n_scans].off,
                                 h, n * 12, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->stage_done[hb], c->stream));
    return pend_push(c, n, P);
}

static int integrate_impl(tsdf_ctx* c, RecordView V, uint64_t n, const ScanPose& P) {
    if (border_busy(c)) return TSDF_EINVAL;
    if (const int rc = check_layout(c, V)) return rc;
    {  // the context's share of the cloud (all of it unless index-sharded)
        uint64_t lo, hi;
        idx_share(c, n, lo, hi);
        if (V.base) V.base += lo * V.point_step;
        n = hi - lo;
    }
    if (n > c->max_points)
        return fail(c, TSDF_EINVAL, "scan of %llu points exceeds max_points %llu",
                    (unsigned long long)n, (unsigned long long)c->max_points);
    int hb;
    float* h;
    if (const int rc = stage_acquire(c, n, &hb, &h)) return rc;
    // on the context's own staging threads; packed fp32 is one memcpy, on the calling thread
    run_parts(&c->pack, V.packed_f32() ? 0 : 1, n,
              [&](int, uint64_t i0, uint64_t i1) { pack_xyz(V, i0, i1, h + 3 * i0); });
    return stage_commit(c, hb, h, n, P);
}

int tsdf_integrate(tsdf_ctx* c, const void* pts, uint64_t n, uint32_t point_step,
                   uint32_t xyz_offset, int32_t xyz_is_f64, const double origin[3]) {
    if (!c) return TSDF_EINVAL;
    if ((!pts && n) || !origin) return fail(c, TSDF_EINVAL, "null argument");
    return integrate_impl(c, records_of(pts, point_step, xyz_offset, xyz_is_f64), n,
                          pose_of_origin(origin));
}

int tsdf_integrate_pose(tsdf_ctx* c, const void* pts, uint64_t n, uint32_t point_step,
                        uint32_t xyz_offset, int32_t xyz_is_f64, const double pose[7]) {
    if (!c) return TSDF_EINVAL;
    if ((!pts && n) || !pose) return fail(c, TSDF_EINVAL, "null argument");
    if (!quat_ok(pose)) return fail(c, TSDF_EINVAL, "pose quaternion is zero");
    return integrate_impl(c, records_of(pts, point_step, xyz_offset, xyz_is_f64), n, pose_of(pose));
}

}  // extern "C"

// ---- tsdf_integrate_sectors: one host cloud for N sector-sharded contexts ----------------------

// The ctxs / n rule every multi-context entry point starts with
static bool ctxs_ok(tsdf_ctx* const* ctxs, uint32_t n) {
    if (!ctxs || n == 0 || n > TSDF_MAX_WORLD) return false;
    for (uint32_t k = 0; k < n; k++)
        if (!ctxs[k]) return false;
    return true;
}

// The error text of a multi-context call is read from ctxs[0] (the Python wrapper, the node).
// mirror: the caller knows that context k failed, and its text replaces ctxs[0]'s.  Call it on the
// thread that owns the call.  first_error (border reduce, sharded mesh: the failing context is not
// tracked through their steps) copies the first other context's text, and only when ctxs[0] holds
// none at all, so a text left in ctxs[0] by an earlier call wins there.
static int mirror(tsdf_ctx* const* ctxs, uint32_t k, int rc) {
    if (rc && k) ctxs[0]->err = ctxs[k]->err;
    return rc;
}
static int first_error(tsdf_ctx* const* ctxs, uint32_t n, int rc) {
    for (uint32_t k = 1; k < n && ctxs[0]->err.empty(); k++) ctxs[0]->err = ctxs[k]->err;
    return rc;
}

// stage_commit of one of a sectors call's contexts: on its device first
static int stage_commit_on(tsdf_ctx* c, int hb, const float* h, uint64_t n, const ScanPose& P) {
    HIPCHK(c, hipSetDevice(c->device));
    return stage_commit(c, hb, h, n, P);
}

// The contexts' staging pools, for run_parts (a context without threads has none)
static void pools_of(tsdf_ctx* const* ctxs, uint32_t n, PackPool** pools) {
    for (uint32_t k = 0; k < n; k++) pools[k] = ctxs[k]->pack;
}

// tsdf_integrate_sectors without a host split (tsdf_params.sector_input FANOUT / H2D): the cloud
// is packed ONCE into ctxs[0]'s pinned buffer hx (on every context's staging threads), and every
// context receives all of it -- its kernels drop the other sectors' rays (R.sec_on), so the fields
// are those of the split, bit for bit.
//   FANOUT: one H2D copy into ctxs[0]'s staging (the leader); the other contexts (followers) take
//           the scan into their pending batch and copy the batch's points from the leader's staging
//           in ONE device-to-device copy before they launch it (fan_copy: hipMemcpyPeerAsync, xGMI
//           with peer access, tsdf_create_sharded) -- O(1) API calls per follower per scan.
//   H2D:    every context copies hx over its own PCIe link; ctxs[0]'s stream waits for them all
//           before it records hx's reuse event.
// One follower's leg: the scan's n points, at offset off0 of the leader c0's staging buffer buf0
// (device) and in hx (host), join c's pending batch.
static int broadcast_follower(tsdf_ctx* c, tsdf_ctx* c0, float* buf0, uint64_t off0,
                              const float* hx, uint64_t n, const ScanPose& P, bool fanout) {
    HIPCHK(c, hipSetDevice(c->device));
    int rc = pend_stage_buffer(c);
    if (rc) return rc;
    const uint64_t off = c->pend.s[c->pend.n_scans].off;
    if (fanout) {
        // batch-granular: extend the follower's uncopied range when it continues in the same
        // leader buffer at the same offset (lockstep batches), else copy what it holds first
        if (c->fan_src != c0 || c->fan_buf != buf0 || c->fan_hi != off || off != off0) {
            rc = fan_copy(c);
            if (rc) return rc;
            if (c->fan_src && c->fan_src != c0) {  // a new leader
                auto& v = c->fan_src->fan_followers;
                v.erase(std::remove(v.begin(), v.end(), c), v.end());
            }
            if (std::find(c0->fan_followers.begin(), c0->fan_followers.end(), c) ==
                c0->fan_followers.end())
                c0->fan_followers.push_back(c);
            c->fan_src = c0;
            c->fan_buf = buf0;
            c->fan_lo = c->fan_hi = off;
            if (off != off0) {  // out of lockstep: this scan alone, now
                c->fan_buf = nullptr;  // nothing pending; the next scan starts afresh
                if (n) {
                    rc = fan_copy_range(c, c0, c->stage2[c->pend_stage] + 3 * off, buf0 + 3 * off0,
                                        n * 12);
                    if (rc) return rc;
                }
            }
        }
        if (c->fan_buf) c->fan_hi = off + n;
    } else if (n) {
        // H2D: this context's own PCIe copy of hx; the leader must not reuse hx first
        HIPCHK(c, hipMemcpyAsync(c->stage2[c->pend_stage] + 3 * off, hx, n * 12,
                                 hipMemcpyHostToDevice, c->stream));
        if (!c->bc_ev) HIPCHK(c, c->bc_ev.create());
        HIPCHK(c, hipEventRecord(c->bc_ev, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c0->stream, c->bc_ev, 0));  // (reported by c: see mirror)
    }
    return pend_push(c, n, P);  // a full batch launches here (fan-out: after its copy)
}

static int sectors_broadcast(tsdf_ctx* const* ctxs, uint32_t n_ctx, const RecordView& V,
                             uint64_t n, const ScanPose& P, float* hx, int hb0, bool fanout) {
    tsdf_ctx* c0 = ctxs[0];
    // every context's staging threads pack a share of the points
    PackPool* pools[TSDF_MAX_WORLD];
    pools_of(ctxs, n_ctx, pools);
    run_parts(pools, n_ctx, n,
              [&](int, uint64_t i0, uint64_t i1) { pack_xyz(V, i0, i1, hx + 3 * i0); });
    c0->split_ht.lap(1);  // TSDF_HOST_TIMING: 0 prep, 1 pack, 2 copies + queue
    // the leader's H2D copy first
    HIPCHK(c0, hipSetDevice(c0->device));
    if (const int rc = pend_stage_buffer(c0)) return rc;
    const uint64_t off0 = c0->pend.s[c0->pend.n_scans].off;
    float* buf0 = c0->stage2[c0->pend_stage];
    if (n) HIPCHK(c0, hipMemcpyAsync(buf0 + 3 * off0, hx, n * 12, hipMemcpyHostToDevice, c0->stream));
    if (!c0->bc_ev) HIPCHK(c0, c0->bc_ev.create());
    HIPCHK(c0, hipEventRecord(c0->bc_ev, c0->stream));
    for (uint32_t k = 1; k < n_ctx; k++)
        if (const int rc = mirror(ctxs, k, broadcast_follower(ctxs[k], c0, buf0, off0, hx, n, P, fanout)))
            return rc;
    HIPCHK(c0, hipSetDevice(c0->device));
    HIPCHK(c0, hipEventRecord(c0->stage_done[hb0], c0->stream));
    if (const int rc = pend_push(c0, n, P)) return rc;
    c0->split_ht.lap(2);
    return TSDF_OK;
}

// tsdf_integrate_sectors under TSDF_SECTOR_RULE_INDEX: context k receives points [lo_k, hi_k)
// (idx_share).  The packing is one parallel pass on the staging threads of the first few contexts
// (each part of the cloud to the pinned buffers of the contexts whose shares it covers), then per
// context one H2D copy of its share and the scan joins its pending batch.
static int sectors_shares(tsdf_ctx* const* ctxs, uint32_t n_ctx, const RecordView& V, uint64_t n,
                          const ScanPose& P) {
    tsdf_ctx* c0 = ctxs[0];
    HostTiming& ht = c0->split_ht;
    ht.start();
    uint64_t lo[TSDF_MAX_WORLD + 1];
    for (uint32_t k = 0; k < n_ctx; k++) {
        uint64_t l, h;
        idx_share(ctxs[k], n, l, h);
        lo[k] = l;
        if (h - l > ctxs[k]->max_points)
            return fail(c0, TSDF_EINVAL, "share of %llu points exceeds max_points of context %u",
                        (unsigned long long)(h - l), k);
    }
    lo[n_ctx] = n;
    float* h[TSDF_MAX_WORLD];
    int hb[TSDF_MAX_WORLD];
    for (uint32_t k = 0; k < n_ctx; k++)  // room in every pending batch, a free pinned buffer
        if (const int rc = mirror(ctxs, k, stage_acquire(ctxs[k], lo[k + 1] - lo[k], &hb[k], &h[k])))
            return rc;
    ht.lap(0);
    // the staging pools of the first few contexts only: every pool's workers spin ~100 us after a
    // job, so N pools' workers (4 N threads) would crowd the calling thread off a 16-CPU share
    // (TSDF_SECTOR_PACK_POOLS, default 2: 8 threads)
    static const uint32_t max_pools = [] {
        const char* e = std::getenv("TSDF_SECTOR_PACK_POOLS");
        return e ? (uint32_t)std::max(1, std::atoi(e)) : 2u;
    }();
    PackPool* pools[TSDF_MAX_WORLD];
    const uint32_t np = std::min(n_ctx, max_pools);
    pools_of(ctxs, np, pools);
    run_parts(pools, np, n,
              [&](int, uint64_t i0, uint64_t i1) { pack_shares(V, i0, i1, lo, n_ctx, h); });
    ht.lap(1);
    for (uint32_t k = 0; k < n_ctx; k++)
        if (const int rc = mirror(ctxs, k, stage_commit_on(ctxs[k], hb[k], h[k], lo[k + 1] - lo[k], P)))
            return rc;
    HIPCHK(c0, hipSetDevice(c0->device));
    ht.lap(3);
    ht.n++;
    return TSDF_OK;
}

// The sectors call proper, by the contexts' sector_rule and sector_input.  The host split (world
// rule): every point is classified once (the kernels' in_sector rule on each
// context's bounds) and packed into its context's pinned staging; each context then copies only
// its sector's points to its GPU, so a scan crosses PCIe once in total, split over the N links.
static int sectors_impl(tsdf_ctx* const* ctxs, uint32_t n_ctx, const RecordView& V, uint64_t n,
                        const ScanPose& P) {
    tsdf_ctx* c0 = ctxs[0];
    if (!V.base && n) return fail(c0, TSDF_EINVAL, "null argument");
    if (const int rc = check_layout(c0, V)) return rc;
    for (uint32_t k = 0; k < n_ctx; k++)
        if (border_busy(ctxs[k])) return mirror(ctxs, k, TSDF_EINVAL);
    // TSDF_SECTOR_RULE_INDEX (ABI v10): context k's share is a contiguous index range of the
    // cloud, whatever sector_input says: one pass over the cloud, no classification, no fan-out
    // (a Merged context bundles its share)
    if (n_ctx > 1 && c0->idx_rule) return sectors_shares(ctxs, n_ctx, V, n, P);
    for (uint32_t k = 0; k < n_ctx; k++) {
        const tsdf_ctx* c = ctxs[k];
        if (n > c->max_points)  // a context may receive every point
            return fail(c0, TSDF_EINVAL, "scan of %llu points exceeds max_points of context %u",
                        (unsigned long long)n, k);
    }
    const float ox = (float)P.o[0], oy = (float)P.o[1];
    HostTiming& ht = c0->split_ht;
    ht.start();
    // room in every pending batch, and each context's free pinned buffer
    float* h[TSDF_MAX_WORLD];
    int hb[TSDF_MAX_WORLD];
    for (uint32_t k = 0; k < n_ctx; k++)
        if (const int rc = mirror(ctxs, k, stage_acquire(ctxs[k], n, &hb[k], &h[k]))) return rc;
    int mode = n_ctx > 1 ? c0->p.sector_input : TSDF_SECTOR_INPUT_SPLIT;
    // MergedTsdfIntegrator bundles the whole scan's points before the sector filter: a host split
    // would bundle each sector's points apart
    if (mode == TSDF_SECTOR_INPUT_SPLIT && n_ctx > 1 && c0->merged) mode = TSDF_SECTOR_INPUT_FANOUT;
    if (mode == TSDF_SECTOR_INPUT_FANOUT || mode == TSDF_SECTOR_INPUT_H2D) {
        ht.lap(0);
        if (const int rc = sectors_broadcast(ctxs, n_ctx, V, n, P, h[0], hb[0],
                                             mode == TSDF_SECTOR_INPUT_FANOUT))
            return rc;
        ht.lap(3);
        ht.n++;
        return TSDF_OK;
    }
    // Two passes over point chunks, on the staging threads of ALL the contexts (each GPU's host
    // share): (1) read the records once, pack xyz into c0's scratch and classify each point
    // (host_pack.h sector_of_angle: one pseudo-angle and N compares), counting per (part, sector);
    // (2) copy the packed points, still in cache, to their sector's pinned buffer at the part's
    // prefix (the parts keep the input order within a sector).
    const bool sharded = n_ctx > 1 && c0->R.sec_on;
    float u[TSDF_MAX_WORLD];  // the sector starts, ascending from context r0's
    uint32_t r0 = 0;
    if (sharded) {
        for (uint32_t k = 1; k < n_ctx; k++)
            if (ctxs[k]->R.sec_lo < ctxs[r0]->R.sec_lo) r0 = k;
        for (uint32_t j = 0; j < n_ctx; j++) {
            u[j] = ctxs[(r0 + j) % n_ctx]->R.sec_lo;
            if (j && !(u[j] > u[j - 1]))
                return fail(c0, TSDF_EINVAL, "sector starts of the contexts are not distinct");
        }
    }
    PackPool* pools[TSDF_MAX_WORLD];
    pools_of(ctxs, n_ctx, pools);
    const int parts = part_count(pools, n_ctx, n);
    if (c0->split_xyz.size() < 3 * n) {
        c0->split_xyz.resize(3 * n);
        c0->split_sec.resize(n);
    }
    float* xyz = c0->split_xyz.data();
    int8_t* sec = c0->split_sec.data();
    std::vector<uint64_t> cnt((size_t)parts * n_ctx, 0), at((size_t)parts * n_ctx, 0);
    auto classify = [&](int part, uint64_t i0, uint64_t i1) {
        pack_xyz(V, i0, i1, xyz + 3 * i0);
        uint64_t cl[TSDF_MAX_WORLD] = {};  // local counts (the parts' rows share cache lines)
        for (uint64_t i = i0; i < i1; i++) {
            const float* v = xyz + 3 * i;
            const int k = sharded ? sector_of_angle(pseudo_angle(v[0] - ox, v[1] - oy), u, r0, n_ctx)
                                  : 0;
            sec[i] = (int8_t)k;
            if (k >= 0) cl[k]++;
        }
        for (uint32_t k = 0; k < n_ctx; k++) cnt[(size_t)part * n_ctx + k] = cl[k];
    };
    auto scatter = [&](int part, uint64_t i0, uint64_t i1) {
        float* dst[TSDF_MAX_WORLD];
        for (uint32_t k = 0; k < n_ctx; k++) dst[k] = h[k] + 3 * at[(size_t)part * n_ctx + k];
        for (uint64_t i = i0; i < i1; i++) {
            const int k = sec[i];
            if (k < 0) continue;
            std::memcpy(dst[k], xyz + 3 * i, 12);
            dst[k] += 3;
        }
    };
    ht.lap(0);
    run_parts(pools, n_ctx, n, classify);
    ht.lap(1);
    std::vector<uint64_t> tot(n_ctx, 0);
    for (uint32_t k = 0; k < n_ctx; k++)
        for (int q = 0; q < parts; q++) {
            at[(size_t)q * n_ctx + k] = tot[k];
            tot[k] += cnt[(size_t)q * n_ctx + k];
        }
    run_parts(pools, n_ctx, n, scatter);
    ht.lap(2);
    // each context: its sector's points to its GPU, into its pending batch -- the contexts are
    // independent, so the staging threads issue them side by side (the copy and launch API calls
    // cost ~10 us each on the host)
    int crc[TSDF_MAX_WORLD] = {};
    auto push_ctx = [&](uint32_t k) { return stage_commit_on(ctxs[k], hb[k], h[k], tot[k], P); };
    const int cparts = c0->pack && n_ctx > 1 ? std::min<int>(c0->pack->parts(), (int)n_ctx) : 1;
    if (cparts > 1) {
        c0->pack->run([&](int part) {
            if (part >= cparts) return;
            for (uint32_t k = (uint32_t)part; k < n_ctx; k += (uint32_t)cparts) crc[k] = push_ctx(k);
        });
    } else {
        for (uint32_t k = 0; k < n_ctx; k++) crc[k] = push_ctx(k);
    }
    for (uint32_t k = 0; k < n_ctx; k++)
        if (crc[k]) return mirror(ctxs, k, crc[k]);
    ht.lap(3);
    ht.n++;
    return TSDF_OK;
}

// The ctxs / n_ctx rule of the sectors entry points: n_ctx contexts, context k sector k of n_ctx
// with the same sector_yaw0 and sector_rule (one context: not sharded)
static int check_sector_ctxs(tsdf_ctx* const* ctxs, uint32_t n_ctx) {
    if (!ctxs_ok(ctxs, n_ctx)) return TSDF_EINVAL;
    const tsdf_ctx* c0 = ctxs[0];
    for (uint32_t k = 0; k < n_ctx; k++) {
        const tsdf_ctx* c = ctxs[k];
        const bool sharded = n_ctx == 1 ? c->p.n_sectors <= 1 : c->p.n_sectors == n_ctx;
        if (!sharded || (n_ctx > 1 && (c->p.sector != k || c->p.sector_yaw0 != c0->p.sector_yaw0 ||
                                       c->p.sector_rule != c0->p.sector_rule)))
            return fail(ctxs[0], TSDF_EINVAL,
                        "context %u is not sector %u of %u (same sector_yaw0 and sector_rule)", k, k,
                        n_ctx);
    }
    return TSDF_OK;
}

extern "C" {

int tsdf_integrate_sectors(tsdf_ctx* const* ctxs, uint32_t n_ctx, const void* pts, uint64_t n,
                           uint32_t point_step, uint32_t xyz_offset, int32_t xyz_is_f64,
                           const double pose[7]) {
    const int rc = check_sector_ctxs(ctxs, n_ctx);
    if (rc) return rc;
    if (!pose) return fail(ctxs[0], TSDF_EINVAL, "null argument");
    if (!quat_ok(pose)) return fail(ctxs[0], TSDF_EINVAL, "pose quaternion is zero");
    return sectors_impl(ctxs, n_ctx, records_of(pts, point_step, xyz_offset, xyz_is_f64), n,
                        pose_of(pose));
}

// ABI v9: the sectors path with a bare origin keeps tsdf_integrate's "no orientation"
// (Voxblox's constant weight), so the sharded field equals the unsharded one for every semantics
int tsdf_integrate_sectors_origin(tsdf_ctx* const* ctxs, uint32_t n_ctx, const void* pts,
                                  uint64_t n, uint32_t point_step, uint32_t xyz_offset,
                                  int32_t xyz_is_f64, const double origin[3]) {
    const int rc = check_sector_ctxs(ctxs, n_ctx);
    if (rc) return rc;
    if (!origin) return fail(ctxs[0], TSDF_EINVAL, "null argument");
    return sectors_impl(ctxs, n_ctx, records_of(pts, point_step, xyz_offset, xyz_is_f64), n,
                        pose_of_origin(origin));
}

// origins: 3 doubles per scan (pose_stride 3) or poses: 7 per scan (pose_stride 7)
static int batch_device_impl(tsdf_ctx* c, const float* d_xyz, const uint64_t* offs,
                             uint32_t n_scans, const double* origins, int pose_stride) {
    if (!c) return TSDF_EINVAL;
    if (border_busy(c)) return TSDF_EINVAL;
    if (!offs || !origins || (!d_xyz && n_scans)) return fail(c, TSDF_EINVAL, "null argument");
    for (uint32_t s = 0; s < n_scans; s++) {
        if (offs[s + 1] < offs[s]) return fail(c, TSDF_EINVAL, "scan_offsets not monotone");
        if (offs[s + 1] - offs[s] > c->max_points)
            return fail(c, TSDF_EINVAL, "scan %u of %llu points exceeds max_points %llu", s,
                        (unsigned long long)(offs[s + 1] - offs[s]),
                        (unsigned long long)c->max_points);
    }
    HIPCHK(c, hipSetDevice(c->device));
    int rc = flush(c);
    if (rc) return rc;
    // Each scan's share (all of it unless index-sharded: then only [lo, hi) of it is read, and the
    // shares of a batch's scans are not contiguous -- ScanRec.xoff = the gap before each share)
    uint32_t s = 0;
    while (s < n_scans) {
        BatchDesc D;
        D.n_scans = 0;
        D.s[0].off = 0;
        uint64_t lo, hi;
        idx_share(c, offs[s + 1] - offs[s], lo, hi);
        const uint64_t b0 = offs[s] + lo;
        while (s < n_scans && D.n_scans < c->max_batch) {
            idx_share(c, offs[s + 1] - offs[s], lo, hi);
            const uint64_t x0 = offs[s] + lo - b0, nb = D.s[D.n_scans].off + (hi - lo);
            if (nb > c->plan.batch_points || x0 + (hi - lo) > 0xFFFFFFFFull) break;
            const double* q = origins + (uint64_t)pose_stride * s;
            set_pose(D, D.n_scans, pose_stride == 7 ? pose_of(q) : pose_of_origin(q));
            D.s[D.n_scans].xoff = (uint32_t)(x0 - D.s[D.n_scans].off);
            D.s[D.n_scans + 1].off = (uint32_t)nb;
            D.n_scans++;
            s++;
        }
        rc = launch(c, d_xyz + 3 * b0, D);
        if (rc) return rc;
        c->n_points_in += D.s[D.n_scans].off;
    }
    return TSDF_OK;
}

int tsdf_integrate_batch_device(tsdf_ctx* c, const float* d_xyz, const uint64_t* offs,
                                uint32_t n_scans, const double* origins) {
    return batch_device_impl(c, d_xyz, offs, n_scans, origins, 3);
}

int tsdf_integrate_batch_device_pose(tsdf_ctx* c, const float* d_xyz, const uint64_t* offs,
                                     uint32_t n_scans, const double* poses) {
    if (c && poses)
        for (uint32_t s = 0; s < n_scans; s++)
            if (!quat_ok(poses + 7 * (uint64_t)s))
                return fail(c, TSDF_EINVAL, "pose %u: quaternion is zero", s);
    return batch_device_impl(c, d_xyz, offs, n_scans, poses, 7);
}

// A single device scan joins the pending batch like a host scan: its points are copied into the
// pending batch's device staging before the call returns, so the caller's buffer is free at once
// (and a capacity replay re-reads the library's copy, not the caller's memory).
int tsdf_integrate_device(tsdf_ctx* c, const float* d_xyz, uint64_t n, const double origin[3]) {
    if (!c) return TSDF_EINVAL;
    if (border_busy(c)) return TSDF_EINVAL;
    if ((!d_xyz && n) || !origin) return fail(c, TSDF_EINVAL, "null argument");
    {  // the context's share of the scan (all of it unless index-sharded)
        uint64_t lo, hi;
        idx_share(c, n, lo, hi);
        if (d_xyz) d_xyz += 3 * lo;
        n = hi - lo;
    }
    if (n > c->max_points)
        return fail(c, TSDF_EINVAL, "scan of %llu points exceeds max_points %llu",
                    (unsigned long long)n, (unsigned long long)c->max_points);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = pend_room(c, n);
    if (!rc) rc = pend_stage_buffer(c);
    if (rc) return rc;
    if (n) {
        HIPCHK(c, hipMemcpyAsync(c->stage2[c->pend_stage] + 3 * (uint64_t)c->pend.s[c->pend.n_scans].off,
                                 d_xyz, n * 12, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return pend_push(c, n, pose_of_origin(origin));
}

// flush + drain, ignoring (but keeping) the overflow flag for read-out calls
static int drain(tsdf_ctx* c) {
    HIPCHK(c, hipSetDevice(c->device));
    int rc = settle(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rc = check_and_replay(c);
    if (rc) return rc;
    if (c->timer) c->timer->harvest();
    return emit_metrics(c);
}

int tsdf_sync(tsdf_ctx* c) {
    if (!c) return TSDF_EINVAL;
    const int rc = drain(c);
    if (rc) return rc;
    uint32_t ovf = 0;
    HIPCHK(c, hipMemcpy(&ovf, &c->G->overflow, sizeof ovf, hipMemcpyDeviceToHost));
    const uint32_t dev = ovf;
    ovf |= c->ovf_refused;  // batches check_and_replay re-ran committing what fits
    c->ovf_refused = 0;
    if (ovf) {
        if (dev) HIPCHK(c, hipMemset(&c->G->overflow, 0, sizeof ovf));
        if (ovf & ERR_MERGE_KEY)
            return fail(c, TSDF_EINVAL, "border merge: a tile's brick is not held by this context");
        return fail(c, TSDF_ENOMEM, "capacity overflow (%s%s%s%s%s%s%s%s): updates were dropped",
                    (ovf & OVF_TABLE) ? "hash table full; " : "",
                    (ovf & OVF_POOL) ? "brick pool exhausted; " : "",
                    (ovf & OVF_PAIRS) ? "ray brick-pair slots exceeded; " : "",
                    (ovf & OVF_ACTIVE) ? "active-brick list full; " : "",
                    (ovf & OVF_SMP) ? "sample list full; " : "",
                    (ovf & OVF_FB) ? "fallback pair list full; " : "",
                    (ovf & OVF_SPN) ? "span list full; " : "",
                    (ovf & OVF_MG) ? "merged integrator: more distinct voxels in one bucket of a "
                                     "scan than its table holds, their points were not bundled; "
                                   : "");
    }
    return TSDF_OK;
}

}  // extern "C"

// ---- read-out and exchange: what the calls below share -------------------------------------------

// A call's temporary device memory: allocated on a context's device, freed there at scope end,
// whichever way the call returns.  take() hands a buffer over to a longer-lived owner (the border
// transaction's brd_sent and brd_backup, freed by tsdf_border_commit_device).
struct Scratch {
    std::vector<std::pair<int, void*>> held;  // (device, buffer)
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    // n elements on c's device (at least 16 bytes, so never a null pointer)
    template <class T>
    hipError_t get(tsdf_ctx* c, T** p, size_t n) {
        void* q = nullptr;
        hipError_t e = hipSetDevice(c->device);
        if (e == hipSuccess) e = hipMalloc(&q, std::max<size_t>(n * sizeof(T), 16));
        if (e == hipSuccess) held.push_back({c->device, q});
        *p = e == hipSuccess ? static_cast<T*>(q) : nullptr;
        return e;
    }
    // the same as a status code, the text in c (for the calls that go on to roll back)
    template <class T>
    int get_or_fail(tsdf_ctx* c, T** p, size_t n) {
        HIPCHK(c, get(c, p, n));
        return TSDF_OK;
    }
    template <class T>
    T* take(T* p) {
        held.erase(std::find_if(held.begin(), held.end(), [p](const auto& q) { return q.second == p; }));
        return p;
    }
    ~Scratch() {
        for (auto& q : held) {
            (void)hipSetDevice(q.first);
            (void)hipFree(q.second);
        }
    }
};

// The caller's current device, restored at scope end: the multi-context calls switch devices.
struct DeviceGuard {
    int dev = -1;
    DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
    ~DeviceGuard() { if (dev >= 0) (void)hipSetDevice(dev); }
};

// Bytes from context src's device buffer to context dst's: an xGMI peer copy, or a device copy
// when both share a GPU.
static hipError_t copy_between(tsdf_ctx* dst, void* d_dst, tsdf_ctx* src, const void* d_src,
                               size_t bytes) {
    if (!bytes) return hipSuccess;
    return src->device == dst->device ? hipMemcpy(d_dst, d_src, bytes, hipMemcpyDeviceToDevice)
                                      : hipMemcpyPeer(d_dst, dst->device, d_src, src->device, bytes);
}

extern "C" {

int tsdf_query_dense(tsdf_ctx* c, const int64_t lo[3], const int64_t hi[3], float* sdf,
                     float* weight) {
    if (!c) return TSDF_EINVAL;
    if (!lo || !hi) return fail(c, TSDF_EINVAL, "null argument");
    int dims[3];
    for (int a = 0; a < 3; a++) {
        if (hi[a] < lo[a]) return fail(c, TSDF_EINVAL, "hi < lo");
        // (the extent as unsigned: hi - lo of int64 bounds may exceed the int64 range)
        const uint64_t ext = (uint64_t)hi[a] - (uint64_t)lo[a];
        if (ext >= (1ull << 31)) return fail(c, TSDF_EINVAL, "query extent >= 2^31 voxels");
        dims[a] = (int)ext;
    }
    uint64_t total = 0;  // (dims[0] dims[1] < 2^62; the third factor may overflow)
    if (__builtin_mul_overflow((uint64_t)dims[0] * (uint64_t)dims[1], (uint64_t)dims[2], &total) ||
        total >= (1ull << 40))
        return fail(c, TSDF_EINVAL, "query box >= 2^40 voxels");
    int rc = drain(c);
    if (rc) return rc;
    if (!total) return TSDF_OK;
    Scratch tmp;
    float *ds = nullptr, *dw = nullptr;
    HIPCHK(c, tmp.get(c, &ds, total));
    HIPCHK(c, tmp.get(c, &dw, total));
    HIPCHK(c, launch_query_dense(c->T, c->Pl, lo, dims, c->R.bg, ds, dw, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (sdf) HIPCHK(c, hipMemcpy(sdf, ds, total * 4, hipMemcpyDeviceToHost));
    if (weight) HIPCHK(c, hipMemcpy(weight, dw, total * 4, hipMemcpyDeviceToHost));
    return TSDF_OK;
}

// ---- sparse map queries (include/tsdf_hip_sample.h) ---------------------------------------------

// The argument rules the sampling and raycast entry points share, in the order they are reported:
// mode, min_weight, then the caller's own refusal (`own`, a text or null: raycast's lattice rules),
// then the context's state.
static int map_query_args(tsdf_ctx* c, const char* what, const char* doing, int32_t mode,
                          float min_weight, const char* own) {
    if (mode != TSDF_SAMPLE_NEAREST && mode != TSDF_SAMPLE_TRILINEAR)
        return fail(c, TSDF_EINVAL, "%s: mode must be TSDF_SAMPLE_NEAREST or _TRILINEAR", what);
    if (!(min_weight >= 0.0f)) return fail(c, TSDF_EINVAL, "%s: min_weight is negative or NaN", what);
    if (own) return fail(c, TSDF_EINVAL, "%s: %s", what, own);
    if (c->p.n_sectors > 1)
        return fail(c, TSDF_EINVAL, "%s: the context holds one sector shard of the map "
                                    "(n_sectors > 1); %s a sharded field is not supported", what, doing);
    if (border_busy(c)) return TSDF_EINVAL;
    return TSDF_OK;
}

static int sample_args(tsdf_ctx* c, int32_t mode, float min_weight) {
    return map_query_args(c, "sample", "sampling", mode, min_weight, nullptr);
}

int tsdf_sample_device(tsdf_ctx* c, const float* d_xyz, uint64_t n, int32_t mode, float min_weight,
                       float* d_sdf, float* d_weight, float* d_grad, uint8_t* d_valid) {
    if (!c) return TSDF_EINVAL;
    int rc = sample_args(c, mode, min_weight);
    if (rc) return rc;
    if (n && (!d_xyz || !d_sdf || !d_weight || !d_valid))
        return fail(c, TSDF_EINVAL, "sample: null buffer");
    if (!n) return TSDF_OK;
    rc = drain(c);
    if (rc) return rc;
    HIPCHK(c, launch_sample(c->T, c->Pl, c->R, d_xyz, n, mode, min_weight, d_sdf, d_weight, d_grad,
                            d_valid, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TSDF_OK;
}

int tsdf_sample(tsdf_ctx* c, const void* pts, uint64_t n, uint32_t point_step, uint32_t xyz_offset,
                int32_t xyz_is_f64, int32_t mode, float min_weight, float* sdf, float* weight,
                float* grad, uint8_t* valid) {
    if (!c) return TSDF_EINVAL;
    int rc = sample_args(c, mode, min_weight);
    if (rc) return rc;
    const RecordView V = records_of(pts, point_step, xyz_offset, xyz_is_f64);
    rc = check_layout(c, V);
    if (rc) return rc;
    if (n && (!pts || !sdf || !weight || !valid)) return fail(c, TSDF_EINVAL, "sample: null buffer");
    if (!n) return TSDF_OK;
    rc = drain(c);
    if (rc) return rc;
    // pieces of at most max_points: packed fp32 points up, (sdf, weight, grad, valid) down
    const uint64_t piece = std::min<uint64_t>(n, std::max<uint64_t>(c->max_points, 1));
    Scratch tmp;
    float* d = nullptr;  // xyz (3), sdf, weight, grad (3) per point, then the valid bytes
    HIPCHK(c, tmp.get(c, &d, 8 * piece + (piece + 3) / 4));
    float *dx = d, *ds = d + 3 * piece, *dw = d + 4 * piece, *dg = d + 5 * piece;
    uint8_t* dv = reinterpret_cast<uint8_t*>(d + 8 * piece);
    std::vector<float> h(3 * piece);
    for (uint64_t i0 = 0; i0 < n; i0 += piece) {
        const uint64_t m = std::min(piece, n - i0);
        pack_xyz(V, i0, i0 + m, h.data());
        HIPCHK(c, hipMemcpyAsync(dx, h.data(), m * 12, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_sample(c->T, c->Pl, c->R, dx, m, mode, min_weight, ds, dw,
                                grad ? dg : nullptr, dv, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(sdf + i0, ds, m * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(weight + i0, dw, m * 4, hipMemcpyDeviceToHost));
        if (grad) HIPCHK(c, hipMemcpy(grad + 3 * i0, dg, m * 12, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(valid + i0, dv, m, hipMemcpyDeviceToHost));
    }
    return TSDF_OK;
}

int tsdf_align_terms_device(tsdf_ctx* c, const float* d_xyz, uint64_t n, const double pose[12],
                            float min_weight, double out[TSDF_ALIGN_WORDS]) {
    if (!c) return TSDF_EINVAL;
    int rc = sample_args(c, TSDF_SAMPLE_TRILINEAR, min_weight);
    if (rc) return rc;
    if (!pose || !out || (n && !d_xyz)) return fail(c, TSDF_EINVAL, "align_terms: null argument");
    std::fill(out, out + TSDF_ALIGN_WORDS, 0.0);
    if (!n) return TSDF_OK;
    rc = drain(c);
    if (rc) return rc;
    constexpr size_t words = ((size_t)ALIGN_MAX_WG + 1) * ALIGN_PART;
    if (!c->align_part) HIPCHK(c, c->align_part.alloc(words));
    const OsPose P = os_pose(pose);
    HIPCHK(c, launch_align(c->T, c->Pl, c->R, d_xyz, n, P, min_weight, c->align_part, c->stream));
    double r[29];  // H's upper triangle row-major, b, sum r^2, the valid count
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(r, c->align_part + (size_t)ALIGN_MAX_WG * ALIGN_PART, sizeof r,
                        hipMemcpyDeviceToHost));
    int k = 0;
    for (int a = 0; a < 6; a++)
        for (int b = a; b < 6; b++, k++) out[6 * a + b] = out[6 * b + a] = r[k];
    for (int a = 0; a < 6; a++) out[36 + a] = r[21 + a];
    out[42] = r[27];
    out[43] = r[28];
    return TSDF_OK;
}

// ---- raycast (include/tsdf_hip_raycast.h) -------------------------------------------------------

// The number of lattice samples: the k with t_min + (float)k * step <= t_max, in the kernel's fp32
// expression.  Every step of it is monotone in k, so the k that pass form a prefix and a bisection
// counts them; the count is capped at RAYCAST_MAX_SAMPLES.
static uint32_t raycast_samples(float t_min, float t_max, float step) {
    const auto in = [&](uint32_t k) {
        const float t = t_min + (float)k * step;
        return t <= t_max;
    };
    if (!in(0)) return 0;
    uint32_t lo = 0, hi = RAYCAST_MAX_SAMPLES;  // in(lo); hi is past the cap
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (in(mid)) lo = mid;
        else hi = mid;
    }
    return lo + 1;
}

// the argument rules both raycast entry points share (the buffers apart)
static int raycast_args(tsdf_ctx* c, float t_min, float t_max, float step, int32_t mode,
                        float min_weight) {
    const char* own = nullptr;  // the lattice rules, the first that fails
    if (!std::isfinite(t_min) || !std::isfinite(t_max) || !std::isfinite(step))
        own = "t_min, t_max and step must be finite";
    else if (!(step > 0.0f)) own = "step must be positive";
    else if (t_min < 0.0f || t_max < t_min) own = "need 0 <= t_min <= t_max";
    else if (((double)t_max - (double)t_min) / (double)step >= (double)RAYCAST_MAX_SAMPLES)
        own = "(t_max - t_min) / step must stay below 2^20 samples";
    return map_query_args(c, "raycast", "raycasting", mode, min_weight, own);
}

int tsdf_raycast_device(tsdf_ctx* c, const float* d_org, const float* d_dir, uint64_t n,
                        const double pose[12], float t_min, float t_max, float step, int32_t mode,
                        float min_weight, float* d_depth, float* d_normal, uint8_t* d_hit) {
    if (!c) return TSDF_EINVAL;
    int rc = raycast_args(c, t_min, t_max, step, mode, min_weight);
    if (rc) return rc;
    if (n && (!d_org || !d_dir || !d_depth || !d_hit))
        return fail(c, TSDF_EINVAL, "raycast: null buffer");
    if (!n) return TSDF_OK;
    rc = drain(c);
    if (rc) return rc;
    const OsPose P = os_pose(pose);
    HIPCHK(c, launch_raycast(c->T, c->Pl, c->R, d_org, d_dir, n, pose ? &P : nullptr, t_min, step,
                             raycast_samples(t_min, t_max, step), mode, min_weight, d_depth,
                             d_normal, d_hit, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TSDF_OK;
}

int tsdf_raycast(tsdf_ctx* c, const float* org, const float* dir, uint64_t n, const double pose[12],
                 float t_min, float t_max, float step, int32_t mode, float min_weight, float* depth,
                 float* normal, uint8_t* hit) {
    if (!c) return TSDF_EINVAL;
    int rc = raycast_args(c, t_min, t_max, step, mode, min_weight);
    if (rc) return rc;
    if (n && (!org || !dir || !depth || !hit)) return fail(c, TSDF_EINVAL, "raycast: null buffer");
    if (!n) return TSDF_OK;
    rc = drain(c);
    if (rc) return rc;
    const OsPose P = os_pose(pose);
    const uint32_t n_k = raycast_samples(t_min, t_max, step);
    // pieces of at most max_points: (origin, direction) up, (depth, normal, hit) down
    const uint64_t piece = std::min<uint64_t>(n, std::max<uint64_t>(c->max_points, 1));
    Scratch tmp;
    float* d = nullptr;  // org (3), dir (3), depth, normal (3) per ray, then the hit bytes
    HIPCHK(c, tmp.get(c, &d, 10 * piece + (piece + 3) / 4));
    float *dorg = d, *ddir = d + 3 * piece, *dd = d + 6 * piece, *dn = d + 7 * piece;
    uint8_t* dh = reinterpret_cast<uint8_t*>(d + 10 * piece);
    for (uint64_t i0 = 0; i0 < n; i0 += piece) {
        const uint64_t m = std::min(piece, n - i0);
        HIPCHK(c, hipMemcpyAsync(dorg, org + 3 * i0, m * 12, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(ddir, dir + 3 * i0, m * 12, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_raycast(c->T, c->Pl, c->R, dorg, ddir, m, pose ? &P : nullptr, t_min, step,
                                 n_k, mode, min_weight, dd, normal ? dn : nullptr, dh, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(depth + i0, dd, m * 4, hipMemcpyDeviceToHost));
        if (normal) HIPCHK(c, hipMemcpy(normal + 3 * i0, dn, m * 12, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(hit + i0, dh, m, hipMemcpyDeviceToHost));
    }
    return TSDF_OK;
}

// ---- distance field of a box (include/tsdf_hip_esdf.h) ------------------------------------------

// The rules both entry points share (the output buffers apart), reported in the header's order; B:
// the box's extents.
static int esdf_args(tsdf_ctx* c, const int64_t lo[3], const int64_t hi[3], uint32_t radius_vox,
                     float site_band, float min_weight, EsdfBox* B) {
    if (!lo || !hi) return fail(c, TSDF_EINVAL, "esdf: null argument");
    const int a = esdf_check(lo, hi, radius_vox, site_band, min_weight, B);
    // (min_weight is map_query_args' own rule and text)
    return map_query_args(c, "esdf", "a distance field of", TSDF_SAMPLE_NEAREST, min_weight,
                          a == ESDF_ARG_WEIGHT ? nullptr : esdf_arg_text(a));
}

// The field of box B into device buffers; the scratch lives for the call.
static int esdf_run(tsdf_ctx* c, const int64_t lo[3], const EsdfBox& B, uint32_t radius_vox,
                    float site_band, float min_weight, float* d_dist, uint8_t* d_flags) {
    // one allocation: two u16 planes and the class bytes, each part 16-byte aligned
    const size_t plane = (size_t)((2 * B.total + 15) & ~(uint64_t)15);
    Scratch tmp;
    uint8_t* s = nullptr;
    if (tmp.get(c, &s, 2 * plane + (size_t)B.total) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, TSDF_ENOMEM, "esdf: scratch allocation of %llu bytes failed",
                    (unsigned long long)esdf_scratch_bytes(B.total));
    }
    uint16_t *g0 = reinterpret_cast<uint16_t*>(s), *g1 = reinterpret_cast<uint16_t*>(s + plane);
    uint8_t* cls = s + 2 * plane;
    HIPCHK(c, launch_esdf(c->T, c->Pl, lo, B.n, radius_vox, site_band, min_weight, c->R.bg, c->R.vs,
                          g0, g1, cls, d_dist, d_flags, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TSDF_OK;
}

int tsdf_esdf_dense_device(tsdf_ctx* c, const int64_t lo[3], const int64_t hi[3],
                           uint32_t radius_vox, float site_band, float min_weight, float* d_dist,
                           uint8_t* d_flags) {
    if (!c) return TSDF_EINVAL;
    EsdfBox B;
    int rc = esdf_args(c, lo, hi, radius_vox, site_band, min_weight, &B);
    if (rc) return rc;
    if (!B.total) return TSDF_OK;
    if (!d_dist) return fail(c, TSDF_EINVAL, "esdf: null buffer");
    rc = drain(c);
    if (rc) return rc;
    return esdf_run(c, lo, B, radius_vox, site_band, min_weight, d_dist, d_flags);
}

int tsdf_esdf_dense(tsdf_ctx* c, const int64_t lo[3], const int64_t hi[3], uint32_t radius_vox,
                    float site_band, float min_weight, float* dist, uint8_t* flags) {
    if (!c) return TSDF_EINVAL;
    EsdfBox B;
    int rc = esdf_args(c, lo, hi, radius_vox, site_band, min_weight, &B);
    if (rc) return rc;
    if (!B.total) return TSDF_OK;
    if (!dist) return fail(c, TSDF_EINVAL, "esdf: null buffer");
    rc = drain(c);
    if (rc) return rc;
    Scratch out;
    float* dd = nullptr;
    uint8_t* df = nullptr;
    hipError_t e = out.get(c, &dd, B.total);
    if (e == hipSuccess && flags) e = out.get(c, &df, B.total);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, TSDF_ENOMEM, "esdf: output allocation for %llu voxels failed",
                    (unsigned long long)B.total);
    }
    rc = esdf_run(c, lo, B, radius_vox, site_band, min_weight, dd, df);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(dist, dd, B.total * 4, hipMemcpyDeviceToHost));
    if (flags) HIPCHK(c, hipMemcpy(flags, df, B.total, hipMemcpyDeviceToHost));
    return TSDF_OK;
}

// ---- column maps of a box (include/tsdf_hip_columns.h) -------------------------------------------

// The rules both entry points share (the output buffers apart), reported in the header's order; B:
// the box and its brick columns.
static int columns_args(tsdf_ctx* c, const int64_t lo[3], const int64_t hi[3], float occ_band,
                        float min_weight, uint32_t min_occ, uint32_t min_free, ColBox* B) {
    if (!lo || !hi) return fail(c, TSDF_EINVAL, "columns: null argument");
    const int a = columns_check(lo, hi, occ_band, min_weight, min_occ, min_free, B);
    // (occ_band comes before min_weight; min_weight is map_query_args' own rule and text)
    if (a == COL_ARG_BAND) return fail(c, TSDF_EINVAL, "columns: %s", columns_arg_text(a));
    return map_query_args(c, "columns", "a column map of", TSDF_SAMPLE_NEAREST, min_weight,
                          a == COL_ARG_WEIGHT ? nullptr : columns_arg_text(a));
}

int tsdf_column_map_device(tsdf_ctx* c, const int64_t lo[3], const int64_t hi[3], float occ_band,
                           float min_weight, uint32_t min_occ, uint32_t min_free, float* d_elev,
                           float* d_ceil, uint16_t* d_n_occ, uint16_t* d_n_free, uint8_t* d_flags) {
    if (!c) return TSDF_EINVAL;
    ColBox B;
    int rc = columns_args(c, lo, hi, occ_band, min_weight, min_occ, min_free, &B);
    if (rc) return rc;
    if (!B.cells) return TSDF_OK;
    if (!d_elev && !d_ceil && !d_n_occ && !d_n_free && !d_flags)
        return fail(c, TSDF_EINVAL, "columns: null buffer");
    rc = drain(c);
    if (rc) return rc;
    HIPCHK(c, launch_column_map(c->T, c->Pl, lo, B, occ_band, min_weight, min_occ, min_free, c->R.bg,
                                c->R.vs, d_elev, d_ceil, d_n_occ, d_n_free, d_flags, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TSDF_OK;
}

int tsdf_column_map(tsdf_ctx* c, const int64_t lo[3], const int64_t hi[3], float occ_band,
                    float min_weight, uint32_t min_occ, uint32_t min_free, float* elev, float* ceil,
                    uint16_t* n_occ, uint16_t* n_free, uint8_t* flags) {
    if (!c) return TSDF_EINVAL;
    ColBox B;
    int rc = columns_args(c, lo, hi, occ_band, min_weight, min_occ, min_free, &B);
    if (rc) return rc;
    if (!B.cells) return TSDF_OK;
    if (!elev && !ceil && !n_occ && !n_free && !flags)
        return fail(c, TSDF_EINVAL, "columns: null buffer");
    rc = drain(c);
    if (rc) return rc;
    // the device copy of the outputs asked for
    Scratch out;
    float *de = nullptr, *dc = nullptr;
    uint16_t *dno = nullptr, *dnf = nullptr;
    uint8_t* df = nullptr;
    hipError_t e = hipSuccess;
    if (e == hipSuccess && elev) e = out.get(c, &de, B.cells);
    if (e == hipSuccess && ceil) e = out.get(c, &dc, B.cells);
    if (e == hipSuccess && n_occ) e = out.get(c, &dno, B.cells);
    if (e == hipSuccess && n_free) e = out.get(c, &dnf, B.cells);
    if (e == hipSuccess && flags) e = out.get(c, &df, B.cells);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, TSDF_ENOMEM, "columns: output allocation for %llu columns failed",
                    (unsigned long long)B.cells);
    }
    HIPCHK(c, launch_column_map(c->T, c->Pl, lo, B, occ_band, min_weight, min_occ, min_free, c->R.bg,
                                c->R.vs, de, dc, dno, dnf, df, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (elev) HIPCHK(c, hipMemcpy(elev, de, B.cells * 4, hipMemcpyDeviceToHost));
    if (ceil) HIPCHK(c, hipMemcpy(ceil, dc, B.cells * 4, hipMemcpyDeviceToHost));
    if (n_occ) HIPCHK(c, hipMemcpy(n_occ, dno, B.cells * 2, hipMemcpyDeviceToHost));
    if (n_free) HIPCHK(c, hipMemcpy(n_free, dnf, B.cells * 2, hipMemcpyDeviceToHost));
    if (flags) HIPCHK(c, hipMemcpy(flags, df, B.cells, hipMemcpyDeviceToHost));
    return TSDF_OK;
}

static int pool_bricks(tsdf_ctx* c, uint64_t* n) {
    const int rc = drain(c);
    if (rc) return rc;
    uint32_t pc = 0;
    HIPCHK(c, hipMemcpy(&pc, &c->G->pool_count, sizeof pc, hipMemcpyDeviceToHost));
    *n = std::min<uint64_t>(pc, c->T.max_bricks);
    return TSDF_OK;
}

int tsdf_num_bricks(tsdf_ctx* c, uint64_t* n) {
    if (!c || !n) return TSDF_EINVAL;
    return pool_bricks(c, n);
}

int tsdf_export_bricks(tsdf_ctx* c, int32_t* coords, float* sdf, float* weight, uint64_t cap,
                       uint64_t* n_out) {
    if (!c || !n_out) return TSDF_EINVAL;
    uint64_t nb = 0;
    int rc = pool_bricks(c, &nb);
    if (rc) return rc;
    *n_out = nb;
    if (nb > cap) return fail(c, TSDF_EOVERFLOW, "export needs %llu bricks", (unsigned long long)nb);
    if (!nb) return TSDF_OK;
    std::vector<uint64_t> keys(nb);
    std::vector<float> s, w;
    HIPCHK(c, hipMemcpy(keys.data(), c->T.brick_keys, nb * 8, hipMemcpyDeviceToHost));
    if (sdf) {
        s.resize(nb * BRICK_VOX);
        HIPCHK(c, hipMemcpy(s.data(), c->Pl.sdf, nb * BRICK_VOX * 4, hipMemcpyDeviceToHost));
    }
    if (weight) {
        w.resize(nb * BRICK_VOX);
        HIPCHK(c, hipMemcpy(w.data(), c->Pl.weight, nb * BRICK_VOX * 4, hipMemcpyDeviceToHost));
    }
    std::vector<uint64_t> order(nb);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(),
              [&](uint64_t a, uint64_t b) { return brick_key_less_zyx(keys[a], keys[b]); });
    for (uint64_t i = 0; i < nb; i++) {
        const uint64_t k = order[i];
        if (coords)
            for (int a = 0; a < 3; a++) coords[3 * i + a] = brick_key_coord(keys[k], a);
        if (sdf) std::memcpy(sdf + i * BRICK_VOX, s.data() + k * BRICK_VOX, BRICK_VOX * 4);
        if (weight) std::memcpy(weight + i * BRICK_VOX, w.data() + k * BRICK_VOX, BRICK_VOX * 4);
    }
    return TSDF_OK;
}

// Ouster packets: the layouts per UDP profile are os_layout (os_headers.h).
int tsdf_os_packet_bytes(const tsdf_os_format* fmt, uint32_t* bytes) {
    OsLayout L;
    if (!bytes || !os_layout(fmt, L)) return TSDF_EINVAL;
    *bytes = L.packet_bytes;
    return TSDF_OK;
}

int tsdf_os_decode_device(tsdf_ctx* c, const tsdf_os_format* fmt, const uint8_t* d_packets,
                          uint32_t n_packets, uint32_t* d_range, uint32_t* d_signal,
                          uint32_t* d_reflectivity, uint32_t* d_near_ir) {
    if (!c) return TSDF_EINVAL;
    OsLayout L;
    if (!os_layout(fmt, L)) return fail(c, TSDF_EINVAL, "bad Ouster packet format");
    if (n_packets && !d_packets) return fail(c, TSDF_EINVAL, "null packets");
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t* out[4] = {d_range, d_signal, d_reflectivity, d_near_ir};
    const size_t img = (size_t)L.h * L.w * sizeof(uint32_t);
    for (int k = 0; k < 4; k++)
        if (out[k]) HIPCHK(c, hipMemsetAsync(out[k], 0, img, c->stream));
    HIPCHK(c, launch_os_decode(d_packets, n_packets, L, out, c->stream));
    return TSDF_OK;
}

int tsdf_os_cartesian_device(tsdf_ctx* c, const uint32_t* d_range, uint64_t n, const float* d_dir,
                             const float* d_off, const double pose[12], float* d_xyz) {
    if (!c) return TSDF_EINVAL;
    if (n && (!d_range || !d_dir || !d_off || !d_xyz)) return fail(c, TSDF_EINVAL, "null argument");
    if (!pose) return fail(c, TSDF_EINVAL, "null pose");
    HIPCHK(c, hipSetDevice(c->device));
    const OsPose P = os_pose(pose);
    HIPCHK(c, launch_os_xyz(d_range, n, d_dir, d_off, P, d_xyz, c->stream));
    return TSDF_OK;
}

// ---- motion-compensated frames (include/tsdf_hip_deskew.h) ---------------------------------------
int tsdf_os_headers(const tsdf_os_format* fmt, const uint8_t* packets, uint32_t n_packets,
                    uint64_t* timestamp, uint32_t* status, uint16_t* measurement_id) {
    return os_headers(fmt, packets, n_packets, timestamp, status, measurement_id);
}

int tsdf_os_deskew_device(tsdf_ctx* c, const tsdf_os_format* fmt, const uint8_t* d_packets,
                          uint32_t n_packets, const float* d_dir_cm, const float* d_off_cm,
                          const float* d_col_pose, float* d_xyz, uint32_t* d_range_cm) {
    if (!c) return TSDF_EINVAL;
    OsLayout L;
    if (!os_layout(fmt, L)) return fail(c, TSDF_EINVAL, "bad Ouster packet format");
    if (!d_dir_cm || !d_off_cm || !d_col_pose || !d_xyz || (n_packets && !d_packets))
        return fail(c, TSDF_EINVAL, "null argument");
    if ((uint64_t)n_packets * L.cols_per_packet > (1ull << 20))
        return fail(c, TSDF_EINVAL, "%llu packet columns exceed 2^20",
                    (unsigned long long)n_packets * L.cols_per_packet);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)L.h * L.w;
    HIPCHK(c, hipMemsetAsync(d_xyz, 0xFF, px * 3 * sizeof(float), c->stream));
    if (d_range_cm) HIPCHK(c, hipMemsetAsync(d_range_cm, 0, px * sizeof(uint32_t), c->stream));
    HIPCHK(c, launch_os_deskew(d_packets, n_packets, L, d_dir_cm, d_off_cm, d_col_pose, d_xyz,
                               d_range_cm, c->stream));
    return TSDF_OK;
}

}  // extern "C"

// A context's halo for meshing (ABI v9): received tiles as a small hash table + pool on the
// context's device (the mesh kernels look neighbours up there first), in the caller's scratch.
struct Halo {
    Table H{};
    Pool HP{};
};

static int halo_build(tsdf_ctx* c, const uint32_t* d_halo, uint64_t n_halo, Scratch& tmp, Halo& h) {
    if (!n_halo) return TSDF_OK;
    if (!d_halo) return fail(c, TSDF_EINVAL, "null halo tiles");
    if (n_halo >= (1ull << 30)) return fail(c, TSDF_EINVAL, "too many halo tiles");
    const uint64_t cap = next_pow2(2 * n_halo);
    uint32_t* d_ovf = nullptr;
    HIPCHK(c, tmp.get(c, &h.H.keys, cap));
    HIPCHK(c, tmp.get(c, &h.H.slots, cap));
    HIPCHK(c, tmp.get(c, &h.HP.sdf, 2 * n_halo * BRICK_VOX));
    HIPCHK(c, tmp.get(c, &d_ovf, 4));
    h.H.mask = cap - 1;
    h.H.max_bricks = (uint32_t)n_halo;
    h.HP.weight = h.HP.sdf + n_halo * BRICK_VOX;
    HIPCHK(c, launch_fill_u64(h.H.keys, EMPTY_KEY, cap, c->stream));
    HIPCHK(c, hipMemsetAsync(d_ovf, 0, 16, c->stream));
    HIPCHK(c, launch_halo_build(h.H, h.HP, d_halo, (uint32_t)n_halo, d_ovf, c->stream));
    uint32_t ovf = 0;
    HIPCHK(c, hipMemcpyAsync(&ovf, d_ovf, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (ovf) return fail(c, TSDF_EINVAL, "halo: table overflow");
    return TSDF_OK;
}

// tsdf_extract_mesh_table, with optional halo tiles (device, TSDF_TILE_WORDS rows) looked up before
// the context's own table for the +x/+y/+z neighbours of its bricks
static int mesh_impl(tsdf_ctx* c, float min_weight, int32_t table, const uint32_t* d_halo,
                     uint64_t n_halo, float* tri, uint64_t cap, uint64_t* n_tri) {
    if (!c || !n_tri) return TSDF_EINVAL;
    if (table < 0 || table >= TSDF_MC_TABLES)
        return fail(c, TSDF_EINVAL, "unknown marching-cubes table %d", table);
    uint64_t nb = 0;
    int rc = pool_bricks(c, &nb);
    if (rc) return rc;
    *n_tri = 0;
    if (!nb) return TSDF_OK;
    if (nb >= 0xFFFFFFFFull) return fail(c, TSDF_EINVAL, "too many bricks");
    HIPCHK(c, hipSetDevice(c->device));
    Scratch tmp;
    Halo halo;
    rc = halo_build(c, d_halo, n_halo, tmp, halo);
    if (rc) return rc;
    // bricks in (z, y, x) order: the triangle soup's order (and the oracle's)
    std::vector<uint64_t> keys(nb);
    HIPCHK(c, hipMemcpy(keys.data(), c->T.brick_keys, nb * 8, hipMemcpyDeviceToHost));
    std::sort(keys.begin(), keys.end(), brick_key_less_zyx);
    uint64_t *dk = nullptr, *doff = nullptr;
    uint32_t* dc = nullptr;
    float* dt = nullptr;
    std::vector<uint32_t> cnt(nb);
    std::vector<uint64_t> off(nb);
    HIPCHK(c, tmp.get(c, &dk, nb));
    HIPCHK(c, tmp.get(c, &dc, nb));
    HIPCHK(c, hipMemcpyAsync(dk, keys.data(), nb * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_mesh_count(c->T, c->Pl, halo.H, halo.HP, dk, (uint32_t)nb, min_weight, table, dc,
                                c->stream));
    HIPCHK(c, hipMemcpyAsync(cnt.data(), dc, nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t total = 0;
    for (uint64_t i = 0; i < nb; i++) {
        off[i] = total;
        total += cnt[i];
    }
    *n_tri = total;
    if (tri && total > cap)
        return fail(c, TSDF_EOVERFLOW, "mesh has %llu triangles", (unsigned long long)total);
    if (!tri || !total) return TSDF_OK;
    HIPCHK(c, tmp.get(c, &doff, nb));
    HIPCHK(c, tmp.get(c, &dt, total * 9));
    HIPCHK(c, hipMemcpyAsync(doff, off.data(), nb * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_mesh_emit(c->T, c->Pl, halo.H, halo.HP, dk, (uint32_t)nb, min_weight, table,
                               c->R.vs, doff, dt, c->stream));
    HIPCHK(c, hipMemcpyAsync(tri, dt, total * 36, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TSDF_OK;
}

// ---- frontier voxels (include/tsdf_hip_frontier.h) -----------------------------------------------

// What a frontier call wants: counts only, host outputs or device outputs.
enum FrontierOut { FRONTIER_COUNT, FRONTIER_HOST, FRONTIER_DEVICE };

static int frontier_impl(tsdf_ctx* c, const int64_t* lo, const int64_t* hi, float free_band,
                         float min_weight, int32_t conn, int32_t min_unknown, int32_t* coords,
                         uint8_t* n_unknown, int8_t* dir, uint64_t cap, tsdf_frontier_counts* out,
                         FrontierOut mode) {
    if (!c) return TSDF_EINVAL;
    if (!out) return fail(c, TSDF_EINVAL, "frontier: null counts");
    MeshBox B;
    bool empty = false;
    const int a = frontier_check(lo, hi, free_band, min_weight, conn, min_unknown, &B, &empty);
    if (a != FRONTIER_ARG_OK) return fail(c, TSDF_EINVAL, "frontier: %s", frontier_arg_text(a));
    if (c->p.n_sectors > 1)
        return fail(c, TSDF_EINVAL, "frontier: the context holds one sector shard of the map "
                                    "(n_sectors > 1); the frontier of a sharded field is not "
                                    "supported");
    if (c->brd_open)
        return fail(c, TSDF_EINVAL, "frontier: a border reduce is open on this context: commit or "
                                    "abort it first (tsdf_border_commit_device)");
    uint64_t n_pool = 0;
    int rc = pool_bricks(c, &n_pool);  // flushes and drains
    if (rc) return rc;
    *out = tsdf_frontier_counts{0, 0, 0, 0};
    if (!n_pool || empty) return TSDF_OK;
    if (n_pool >= 0xFFFFFFFFull) return fail(c, TSDF_EINVAL, "frontier: too many bricks");
    HIPCHK(c, hipSetDevice(c->device));
    // the map's bricks in (z, y, x) order (the output's order), then those that intersect the box
    std::vector<uint64_t> all(n_pool), keys;
    HIPCHK(c, hipMemcpy(all.data(), c->T.brick_keys, n_pool * 8, hipMemcpyDeviceToHost));
    std::sort(all.begin(), all.end(), brick_key_less_zyx);
    for (uint64_t k : all)
        if (mesh_brick_in_box(k, B, 0)) keys.push_back(k);
    const uint64_t nb = keys.size();
    out->n_bricks = nb;
    if (!nb) return TSDF_OK;
    Scratch tmp;
    uint64_t *dk = nullptr, *doff = nullptr;
    uint32_t* dcnt = nullptr;  // frontier voxels, then free voxels
    hipError_t e = tmp.get(c, &dk, nb);
    if (e == hipSuccess) e = tmp.get(c, &dcnt, 2 * nb);
    if (e == hipSuccess) e = tmp.get(c, &doff, nb);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, TSDF_ENOMEM, "frontier: scratch allocation for %llu bricks failed",
                    (unsigned long long)nb);
    }
    std::vector<uint32_t> cnt(2 * nb);
    std::vector<uint64_t> off(nb);
    HIPCHK(c, hipMemcpyAsync(dk, keys.data(), nb * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_frontier_count(c->T, c->Pl, dk, (uint32_t)nb, B, free_band, min_weight, conn,
                                    min_unknown, dcnt, dcnt + nb, c->stream));
    HIPCHK(c, hipMemcpyAsync(cnt.data(), dcnt, 2 * nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    frontier_prefix(cnt.data(), nb, off.data(), &out->n_voxels, &out->n_frontier_bricks);
    out->n_free = frontier_sum(cnt.data() + nb, nb);
    const uint64_t nv = out->n_voxels;
    if (mode == FRONTIER_COUNT || !nv) return TSDF_OK;
    if (nv > cap)
        return fail(c, TSDF_EOVERFLOW, "frontier has %llu voxels", (unsigned long long)nv);
    if (!coords) return fail(c, TSDF_EINVAL, "frontier: null buffer");
    int32_t* dc = coords;
    uint8_t* dn = n_unknown;
    int8_t* dd = dir;
    if (mode == FRONTIER_HOST) {  // staged on the device
        e = tmp.get(c, &dc, 3 * nv);
        if (e == hipSuccess && n_unknown) e = tmp.get(c, &dn, nv);
        if (e == hipSuccess && dir) e = tmp.get(c, &dd, 3 * nv);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, TSDF_ENOMEM, "frontier: output allocation for %llu voxels failed",
                        (unsigned long long)nv);
        }
    }
    HIPCHK(c, hipMemcpyAsync(doff, off.data(), nb * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_frontier_emit(c->T, c->Pl, dk, (uint32_t)nb, B, free_band, min_weight, conn,
                                   min_unknown, dcnt, doff, dc, dn, dd, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (mode == FRONTIER_HOST) {
        HIPCHK(c, hipMemcpy(coords, dc, nv * 12, hipMemcpyDeviceToHost));
        if (n_unknown) HIPCHK(c, hipMemcpy(n_unknown, dn, nv, hipMemcpyDeviceToHost));
        if (dir) HIPCHK(c, hipMemcpy(dir, dd, nv * 3, hipMemcpyDeviceToHost));
    }
    return TSDF_OK;
}

extern "C" {

int tsdf_frontier_count(tsdf_ctx* c, const int64_t lo[3], const int64_t hi[3], float free_band,
                        float min_weight, int32_t connectivity, int32_t min_unknown,
                        tsdf_frontier_counts* out) {
    return frontier_impl(c, lo, hi, free_band, min_weight, connectivity, min_unknown, nullptr,
                         nullptr, nullptr, 0, out, FRONTIER_COUNT);
}

int tsdf_frontier_voxels(tsdf_ctx* c, const int64_t lo[3], const int64_t hi[3], float free_band,
                         float min_weight, int32_t connectivity, int32_t min_unknown,
                         int32_t* coords, uint8_t* n_unknown, int8_t* dir, uint64_t cap,
                         tsdf_frontier_counts* out) {
    return frontier_impl(c, lo, hi, free_band, min_weight, connectivity, min_unknown, coords,
                         n_unknown, dir, cap, out, FRONTIER_HOST);
}

int tsdf_frontier_voxels_device(tsdf_ctx* c, const int64_t lo[3], const int64_t hi[3],
                                float free_band, float min_weight, int32_t connectivity,
                                int32_t min_unknown, int32_t* coords, uint8_t* n_unknown,
                                int8_t* dir, uint64_t cap, tsdf_frontier_counts* out) {
    return frontier_impl(c, lo, hi, free_band, min_weight, connectivity, min_unknown, coords,
                         n_unknown, dir, cap, out, FRONTIER_DEVICE);
}

}  // extern "C"

// ---- indexed mesh (include/tsdf_hip_mesh.h) ------------------------------------------------------

// What a call of the indexed mesh wants: counts only, host outputs or device outputs.
enum MeshOut { MESH_COUNT, MESH_HOST, MESH_DEVICE };

static int mesh_indexed_impl(tsdf_ctx* c, float min_weight, int32_t table, const int64_t* lo,
                             const int64_t* hi, float* vertices, float* normals,
                             uint32_t* triangles, uint64_t cap_v, uint64_t cap_t,
                             tsdf_mesh_counts* out, MeshOut mode) {
    if (!c) return TSDF_EINVAL;
    if (!out) return fail(c, TSDF_EINVAL, "mesh: null counts");
    if (table < 0 || table >= TSDF_MC_TABLES)
        return fail(c, TSDF_EINVAL, "mesh: unknown marching-cubes table %d", table);
    MeshBox B;
    bool empty = false;
    const int a = mesh_box_check(lo, hi, &B, &empty);
    int rc = map_query_args(c, "mesh", "an indexed mesh of", TSDF_SAMPLE_NEAREST, min_weight,
                            a == MESH_ARG_OK ? nullptr : mesh_arg_text(a));
    if (rc) return rc;
    uint64_t n_pool = 0;
    rc = pool_bricks(c, &n_pool);  // flushes and drains
    if (rc) return rc;
    *out = tsdf_mesh_counts{0, 0, 0};
    if (!n_pool || empty) return TSDF_OK;
    if (n_pool >= 0xFFFFFFFFull) return fail(c, TSDF_EINVAL, "mesh: too many bricks");
    HIPCHK(c, hipSetDevice(c->device));
    // the map's bricks in (z, y, x) order (the soup's order), then those the box lists
    std::vector<uint64_t> all(n_pool), keys;
    HIPCHK(c, hipMemcpy(all.data(), c->T.brick_keys, n_pool * 8, hipMemcpyDeviceToHost));
    std::sort(all.begin(), all.end(), brick_key_less_zyx);
    out->n_bricks = mesh_list_bricks(all, B, &keys);
    const uint64_t nb = keys.size();
    if (!out->n_bricks) return TSDF_OK;
    Scratch tmp;
    uint64_t *dk = nullptr, *dtoff = nullptr;
    uint32_t *dmask = nullptr, *dcnt = nullptr, *dvbase = nullptr, *dsi = nullptr;
    hipError_t e = tmp.get(c, &dk, nb);
    if (e == hipSuccess) e = tmp.get(c, &dsi, n_pool);  // pool slot -> position in the list
    if (e == hipSuccess) e = tmp.get(c, &dmask, nb * MESH_VMASK_WORDS);
    if (e == hipSuccess) e = tmp.get(c, &dcnt, 2 * nb);  // triangles, then vertices
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, TSDF_ENOMEM, "mesh: scratch allocation for %llu bricks failed",
                    (unsigned long long)nb);
    }
    std::vector<uint32_t> cnt(2 * nb), vbase(nb);
    std::vector<uint64_t> toff(nb);
    HIPCHK(c, hipMemcpyAsync(dk, keys.data(), nb * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_mesh_mark(c->T, c->Pl, dk, (uint32_t)nb, min_weight, table, B,
                               (uint32_t)n_pool, dsi, dmask, dcnt, dcnt + nb, c->stream));
    HIPCHK(c, hipMemcpyAsync(cnt.data(), dcnt, 2 * nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t n_tri = 0, n_vert = 0;
    mesh_prefix(cnt.data(), cnt.data() + nb, nb, toff.data(), vbase.data(), &n_tri, &n_vert);
    if (n_vert >= (1ull << 32))
        return fail(c, TSDF_EINVAL, "mesh: %llu vertices do not fit 32-bit indices; mesh it in "
                                    "boxes", (unsigned long long)n_vert);
    out->n_vertices = n_vert;
    out->n_triangles = n_tri;
    if (mode == MESH_COUNT || !n_tri) return TSDF_OK;
    if (n_vert > cap_v || n_tri > cap_t)
        return fail(c, TSDF_EOVERFLOW, "mesh has %llu vertices and %llu triangles",
                    (unsigned long long)n_vert, (unsigned long long)n_tri);
    if (!vertices || !triangles) return fail(c, TSDF_EINVAL, "mesh: null buffer");
    float *dv = vertices, *dn = normals;
    uint32_t* dt = triangles;
    e = tmp.get(c, &dtoff, nb);
    if (e == hipSuccess) e = tmp.get(c, &dvbase, nb);
    if (mode == MESH_HOST) {  // staged on the device
        if (e == hipSuccess) e = tmp.get(c, &dv, 3 * n_vert);
        if (e == hipSuccess && normals) e = tmp.get(c, &dn, 3 * n_vert);
        if (e == hipSuccess) e = tmp.get(c, &dt, 3 * n_tri);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, TSDF_ENOMEM, "mesh: output allocation for %llu vertices and %llu triangles "
                                    "failed", (unsigned long long)n_vert, (unsigned long long)n_tri);
    }
    HIPCHK(c, hipMemcpyAsync(dtoff, toff.data(), nb * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dvbase, vbase.data(), nb * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_mesh_fill(c->T, c->Pl, dk, (uint32_t)nb, min_weight, table, B, c->R.vs,
                               c->R.inv_vs, (uint32_t)n_pool, dsi, dmask, dcnt, dcnt + nb, dtoff,
                               dvbase, dv, dn, dt, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (mode == MESH_HOST) {
        HIPCHK(c, hipMemcpy(vertices, dv, n_vert * 12, hipMemcpyDeviceToHost));
        if (normals) HIPCHK(c, hipMemcpy(normals, dn, n_vert * 12, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(triangles, dt, n_tri * 12, hipMemcpyDeviceToHost));
    }
    return TSDF_OK;
}

extern "C" {

int tsdf_mesh_indexed_count(tsdf_ctx* c, float min_weight, int32_t table, const int64_t lo[3],
                            const int64_t hi[3], tsdf_mesh_counts* out) {
    return mesh_indexed_impl(c, min_weight, table, lo, hi, nullptr, nullptr, nullptr, 0, 0, out,
                             MESH_COUNT);
}

int tsdf_mesh_indexed(tsdf_ctx* c, float min_weight, int32_t table, const int64_t lo[3],
                      const int64_t hi[3], float* vertices, float* normals, uint32_t* triangles,
                      uint64_t cap_vertices, uint64_t cap_triangles, tsdf_mesh_counts* out) {
    return mesh_indexed_impl(c, min_weight, table, lo, hi, vertices, normals, triangles,
                             cap_vertices, cap_triangles, out, MESH_HOST);
}

int tsdf_mesh_indexed_device(tsdf_ctx* c, float min_weight, int32_t table, const int64_t lo[3],
                             const int64_t hi[3], float* vertices, float* normals,
                             uint32_t* triangles, uint64_t cap_vertices, uint64_t cap_triangles,
                             tsdf_mesh_counts* out) {
    return mesh_indexed_impl(c, min_weight, table, lo, hi, vertices, normals, triangles,
                             cap_vertices, cap_triangles, out, MESH_DEVICE);
}

int tsdf_mc_table(uint8_t* out) {
    if (!out) return TSDF_EINVAL;
    std::memcpy(out, mc_table().tab, sizeof(mc_table().tab));
    return TSDF_OK;
}

int tsdf_mc_table_of(int32_t table, uint8_t* out) {
    if (!out || table < 0 || table >= TSDF_MC_TABLES) return TSDF_EINVAL;
    std::memcpy(out, mc_table(table).tab, sizeof(mc_table(table).tab));
    return TSDF_OK;
}

int tsdf_extract_mesh(tsdf_ctx* c, float min_weight, float* tri, uint64_t cap, uint64_t* n_tri) {
    return tsdf_extract_mesh_table(c, min_weight, TSDF_MC_GENERATED, tri, cap, n_tri);
}

int tsdf_extract_mesh_table(tsdf_ctx* c, float min_weight, int32_t table, float* tri, uint64_t cap,
                            uint64_t* n_tri) {
    return mesh_impl(c, min_weight, table, nullptr, 0, tri, cap, n_tri);
}

int tsdf_import_bricks(tsdf_ctx* c, const int32_t* coords, const float* sdf, const float* weight,
                       uint64_t n) {
    if (!c) return TSDF_EINVAL;
    if (border_busy(c)) return TSDF_EINVAL;
    if (!n) return TSDF_OK;
    if (!coords || !sdf || !weight) return fail(c, TSDF_EINVAL, "null argument");
    if (n >= 0xFFFFFFF0ull) return fail(c, TSDF_EINVAL, "too many bricks");
    {  // bricks must be unique and inside the packable range
        std::vector<uint64_t> k(n);
        for (uint64_t i = 0; i < n; i++) {
            const int32_t* b = coords + 3 * i;
            if (!brick_coord_ok(b[0]) || !brick_coord_ok(b[1]) || !brick_coord_ok(b[2]))
                return fail(c, TSDF_EINVAL, "brick coordinate out of range");
            k[i] = brick_key_pack(b[0], b[1], b[2]);
        }
        std::sort(k.begin(), k.end());
        if (std::adjacent_find(k.begin(), k.end()) != k.end())
            return fail(c, TSDF_EINVAL, "duplicate brick in import");
    }
    int rc = drain(c);
    if (rc) return rc;
    {  // room for n new bricks (import is not a replayable batch: grow first)
        uint32_t pc = 0;
        HIPCHK(c, hipMemcpy(&pc, &c->G->pool_count, 4, hipMemcpyDeviceToHost));
        if (c->can_grow && (uint64_t)pc + n > c->T.max_bricks) {
            rc = grow_capacity(c, (uint64_t)pc + n);
            if (rc == TSDF_EHIP) return rc;
        }
    }
    Scratch tmp;
    int32_t* dc = nullptr;
    float *ds = nullptr, *dw = nullptr;
    uint32_t* dt = nullptr;
    HIPCHK(c, tmp.get(c, &dc, n * 3));
    HIPCHK(c, tmp.get(c, &ds, n * BRICK_VOX));
    HIPCHK(c, tmp.get(c, &dw, n * BRICK_VOX));
    HIPCHK(c, tmp.get(c, &dt, n));
    HIPCHK(c, hipMemcpyAsync(dc, coords, n * 12, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(ds, sdf, n * BRICK_VOX * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dw, weight, n * BRICK_VOX * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_import(c->T, c->Pl, dc, (uint32_t)n, ds, dw, dt, c->G, merge_cap(c), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return tsdf_sync(c);
}

}  // extern "C"

// ---- merging a map into another under a rigid transform (include/tsdf_hip_merge.h; kernels in
// tsdf_merge.hip; the pose, the candidate search and the scratch sizes: merge_plan.h)

// One context's part of the entry rules: the state rules of the read-side calls
static int merge_ctx_state(tsdf_ctx* d, tsdf_ctx* c, const char* which) {
    if (c->p.n_sectors > 1)
        return fail(d, TSDF_EINVAL, "merge: the %s context holds one sector shard of the map "
                                    "(n_sectors > 1); merging a sharded field is not supported", which);
    if (c->brd_open)
        return fail(d, TSDF_EINVAL, "merge: a border reduce is open on the %s context: commit or "
                                    "abort it first (tsdf_border_commit_device)", which);
    return TSDF_OK;
}

static int merge_impl(tsdf_ctx* d, tsdf_ctx* s, const double* pose, int32_t mode, float min_weight,
                      tsdf_merge_stats* out, bool apply) {
    if (!d) return TSDF_EINVAL;
    if (!s) return fail(d, TSDF_EINVAL, "merge: the source context is NULL");
    if (s == d) return fail(d, TSDF_EINVAL, "merge: source and destination are the same context");
    if (!apply && !out) return fail(d, TSDF_EINVAL, "merge: null argument");
    MergeXform X;
    int rule = merge_xform(pose, mode, min_weight, (double)d->R.vs, &X);
    if (rule) return fail(d, TSDF_EINVAL, "merge: %s", merge_arg_text(rule));
    if (s->device != d->device)
        return fail(d, TSDF_EINVAL, "merge: the contexts are on different devices (%d and %d)",
                    d->device, s->device);
    rule = merge_compat(d->p.voxel_size, s->p.voxel_size, d->p.sdf_trunc, s->p.sdf_trunc,
                        d->p.semantics, s->p.semantics);
    if (rule) return fail(d, TSDF_EINVAL, "merge: %s", merge_compat_text(rule));
    int rc = merge_ctx_state(d, d, "destination");
    if (!rc) rc = merge_ctx_state(d, s, "source");
    if (rc) return rc;
    HIPCHK(d, hipSetDevice(d->device));  // (both contexts': the scratch and every launch below)
    uint64_t n_src = 0, n_dst = 0;
    rc = pool_bricks(s, &n_src);
    if (rc) return fail(d, rc, "merge: the source context failed: %s", s->err.c_str());
    rc = pool_bricks(d, &n_dst);
    if (rc) return rc;
    tsdf_merge_stats st{};
    st.src_bricks = n_src;
    if (out) *out = st;
    if (!n_src) return TSDF_OK;

    Scratch tmp;
    unsigned long long* ctr = nullptr;
    std::vector<unsigned long long> hc(MERGE_CTR_WORDS, 0);
    unsigned long long h[6] = {0, 0, 0, 0, 0, 0};
    HIPCHK(d, tmp.get(d, &ctr, MERGE_CTR_WORDS));
    HIPCHK(d, hipMemsetAsync(ctr, 0, MERGE_CTR_WORDS * 8, d->stream));
    HIPCHK(d, launch_merge_pairs(s->T.brick_keys, (uint32_t)n_src, X, mode, ctr, d->stream));
    HIPCHK(d, hipMemcpyAsync(h, ctr, 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    const uint64_t pairs = h[0];
    if (!pairs) return TSDF_OK;  // the image lies outside the index domain
    if (pairs >= MERGE_MAX_PAIRS)
        return fail(d, TSDF_ENOMEM, "merge: %llu candidate bricks", (unsigned long long)pairs);
    const uint64_t slots = merge_set_slots(pairs);
    uint64_t *set = nullptr, *list = nullptr;
    uint32_t *flag = nullptr, *tslot = nullptr;
    if (tmp.get(d, &set, slots) != hipSuccess || tmp.get(d, &list, pairs) != hipSuccess ||
        tmp.get(d, &flag, pairs) != hipSuccess || tmp.get(d, &tslot, pairs) != hipSuccess) {
        (void)hipGetLastError();
        return fail(d, TSDF_ENOMEM, "merge: no device memory for %llu bytes of scratch",
                    (unsigned long long)merge_scratch_bytes(pairs));
    }
    HIPCHK(d, launch_fill_u64(set, EMPTY_KEY, slots, d->stream));
    HIPCHK(d, launch_merge_candidates(s->T.brick_keys, (uint32_t)n_src, X, mode, set, slots, list,
                                      pairs, ctr, d->stream));
    HIPCHK(d, launch_merge_flag(d->T, d->Pl, s->T, s->Pl, s->R, X, mode, min_weight, list, pairs,
                                ctr, flag, d->stream));
    HIPCHK(d, hipMemcpyAsync(hc.data(), ctr, MERGE_CTR_WORDS * 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    h[1] = hc[1];
    for (uint32_t q = 0; q < MERGE_SHARDS; q++)  // the flag kernel's counter shards
        for (int k = 0; k < 4; k++) h[2 + k] += hc[MERGE_CTR_HEAD + q * MERGE_SHARD_WORDS + k];
    const uint64_t n_cand = h[1];
    if (n_cand > pairs || h[3] > h[2] || h[2] > n_cand || h[5] > h[4])
        return fail(d, TSDF_EHIP, "merge: inconsistent counts (%llu candidates of %llu pairs)",
                    (unsigned long long)n_cand, (unsigned long long)pairs);
    st.candidate_bricks = n_cand;
    st.touched_bricks = h[2];
    st.new_bricks = h[3];
    st.merged_voxels = h[4];
    st.overlap_voxels = h[5];
    if (out) *out = st;
    if (!apply || !st.touched_bricks) return TSDF_OK;

    // room for the new bricks before anything is written (a merge is not a replayable batch)
    const uint64_t need = n_dst + st.new_bricks;
    if (need > d->T.max_bricks) {
        if (!d->can_grow || (d->p.max_bricks_hard && need > d->p.max_bricks_hard) ||
            need > 0xFFFFFFEFull)
            return fail(d, TSDF_ENOMEM, "merge: %llu new bricks do not fit the pool (%llu of %llu "
                                        "bricks in use) and it cannot grow",
                        (unsigned long long)st.new_bricks, (unsigned long long)n_dst,
                        (unsigned long long)d->T.max_bricks);
        rc = grow_capacity(d, need);
        if (rc) return rc;
    }
    HIPCHK(d, launch_merge_apply(d->T, d->Pl, s->T, s->Pl, s->R, X, mode, min_weight, merge_cap(d),
                                 list, n_cand, flag, tslot, d->G, d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    return tsdf_sync(d);
}

extern "C" {

int tsdf_merge_count(tsdf_ctx* dst, tsdf_ctx* src, const double pose[12], int32_t mode,
                     float min_weight, tsdf_merge_stats* out) {
    return merge_impl(dst, src, pose, mode, min_weight, out, false);
}

int tsdf_merge_transformed(tsdf_ctx* dst, tsdf_ctx* src, const double pose[12], int32_t mode,
                           float min_weight, tsdf_merge_stats* out) {
    return merge_impl(dst, src, pose, mode, min_weight, out, true);
}

}  // extern "C"

// ---- coarsening a map 2:1 into a map of twice the voxel size (include/tsdf_hip_coarsen.h; kernels
// in tsdf_coarsen.hip; the rules, the index arithmetic and the scratch sizes: coarsen_plan.h;
// DESIGN.md §24)

// One context's part of the entry rules (merge_ctx_state's)
static int coarsen_ctx_state(tsdf_ctx* d, tsdf_ctx* c, const char* which) {
    if (c->p.n_sectors > 1)
        return fail(d, TSDF_EINVAL, "coarsen: the %s context holds one sector shard of the map "
                                    "(n_sectors > 1); coarsening a sharded field is not supported",
                    which);
    if (c->brd_open)
        return fail(d, TSDF_EINVAL, "coarsen: a border reduce is open on the %s context: commit or "
                                    "abort it first (tsdf_border_commit_device)", which);
    return TSDF_OK;
}

static int coarsen_impl(tsdf_ctx* d, tsdf_ctx* s, const int32_t* lo, const int32_t* hi, int32_t side,
                        uint32_t min_children, float min_weight, tsdf_coarsen_stats* out,
                        bool apply) {
    if (!d) return TSDF_EINVAL;
    if (!s) return fail(d, TSDF_EINVAL, "coarsen: the source context is NULL");
    if (s == d) return fail(d, TSDF_EINVAL, "coarsen: source and destination are the same context");
    if (!apply && !out) return fail(d, TSDF_EINVAL, "coarsen: null argument");
    int rule = coarsen_args(side, lo != nullptr, hi != nullptr, min_children, min_weight);
    if (rule) return fail(d, TSDF_EINVAL, "coarsen: %s", coarsen_arg_text(rule));
    if (s->device != d->device)
        return fail(d, TSDF_EINVAL, "coarsen: the contexts are on different devices (%d and %d)",
                    d->device, s->device);
    rule = coarsen_compat(d->p.voxel_size, s->p.voxel_size, d->p.sdf_trunc, s->p.sdf_trunc,
                          d->p.semantics, s->p.semantics);
    if (rule) return fail(d, TSDF_EINVAL, "coarsen: %s", coarsen_compat_text(rule));
    int rc = coarsen_ctx_state(d, d, "destination");
    if (!rc) rc = coarsen_ctx_state(d, s, "source");
    if (rc) return rc;
    HIPCHK(d, hipSetDevice(d->device));  // (both contexts': the scratch and every launch below)
    uint64_t n_src = 0, n_dst = 0;
    rc = pool_bricks(s, &n_src);
    if (rc) return fail(d, rc, "coarsen: the source context failed: %s", s->err.c_str());
    rc = pool_bricks(d, &n_dst);
    if (rc) return rc;
    tsdf_coarsen_stats st{};
    if (out) *out = st;
    if (!n_src) return TSDF_OK;

    CoarsenSel sel{};
    if (lo) {
        sel.has_box = 1;
        sel.side = side;
        for (int a = 0; a < 3; a++) {
            sel.lo[a] = lo[a];
            sel.hi[a] = hi[a];
        }
    }
    Scratch tmp;
    unsigned long long* ctr = nullptr;
    std::vector<unsigned long long> hc(COARSEN_CTR_WORDS, 0);
    const uint64_t slots = coarsen_set_slots(n_src);
    uint64_t *set = nullptr, *list = nullptr;
    uint32_t *flag = nullptr, *tslot = nullptr;
    if (tmp.get(d, &ctr, COARSEN_CTR_WORDS) != hipSuccess || tmp.get(d, &set, slots) != hipSuccess ||
        tmp.get(d, &list, n_src) != hipSuccess || tmp.get(d, &flag, n_src) != hipSuccess ||
        tmp.get(d, &tslot, n_src) != hipSuccess) {
        (void)hipGetLastError();
        return fail(d, TSDF_ENOMEM, "coarsen: no device memory for %llu bytes of scratch",
                    (unsigned long long)coarsen_scratch_bytes(n_src));
    }
    HIPCHK(d, hipMemsetAsync(ctr, 0, COARSEN_CTR_WORDS * 8, d->stream));
    HIPCHK(d, launch_fill_u64(set, EMPTY_KEY, slots, d->stream));
    HIPCHK(d, launch_coarsen_parents(s->T.brick_keys, (uint32_t)n_src, sel, set, slots, list, ctr,
                                     d->stream));
    // the selection's two counts: an empty selection launches nothing more, and the per-brick
    // kernels get the list's exact length
    HIPCHK(d, hipMemcpyAsync(hc.data(), ctr, 16, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    const uint64_t n_sel = hc[0], n_par = hc[1];
    if (n_sel > n_src || n_par > n_sel || (n_sel && !n_par))
        return fail(d, TSDF_EHIP, "coarsen: inconsistent counts (%llu parents of %llu bricks)",
                    (unsigned long long)n_par, (unsigned long long)n_sel);
    st.src_bricks = n_sel;
    st.parent_bricks = n_par;
    if (out) *out = st;
    if (!n_sel) return TSDF_OK;
    HIPCHK(d, launch_coarsen_flag(d->T, d->Pl, s->T, s->Pl, sel, min_children, min_weight, list,
                                  n_par, ctr, flag, d->stream));
    HIPCHK(d, hipMemcpyAsync(hc.data(), ctr, COARSEN_CTR_WORDS * 8, hipMemcpyDeviceToHost,
                             d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    for (uint32_t q = 0; q < COARSEN_SHARDS; q++)  // the flag kernel's counter shards
        for (int k = 0; k < 5; k++) h[k] += hc[COARSEN_CTR_HEAD + q * COARSEN_SHARD_WORDS + k];
    if (h[0] > n_par || h[1] > h[0] || h[3] > h[2] || h[4] < h[2] || h[4] > 8 * h[2])
        return fail(d, TSDF_EHIP, "coarsen: inconsistent counts (%llu touched of %llu parents)",
                    h[0], (unsigned long long)n_par);
    st.touched_bricks = h[0];
    st.new_bricks = h[1];
    st.coarse_voxels = h[2];
    st.overlap_voxels = h[3];
    st.child_voxels = h[4];
    if (out) *out = st;
    if (!apply || !st.touched_bricks) return TSDF_OK;

    // room for the new bricks before anything is written (as the merge does)
    const uint64_t need = n_dst + st.new_bricks;
    if (need > d->T.max_bricks) {
        if (!d->can_grow || (d->p.max_bricks_hard && need > d->p.max_bricks_hard) ||
            need > 0xFFFFFFEFull)
            return fail(d, TSDF_ENOMEM, "coarsen: %llu new bricks do not fit the pool (%llu of "
                                        "%llu bricks in use) and it cannot grow",
                        (unsigned long long)st.new_bricks, (unsigned long long)n_dst,
                        (unsigned long long)d->T.max_bricks);
        rc = grow_capacity(d, need);
        if (rc) return rc;
    }
    HIPCHK(d, launch_merge_insert(d->T, list, n_par, flag, tslot, d->G, d->stream));
    HIPCHK(d, launch_coarsen_apply(d->T, d->Pl, s->T, s->Pl, sel, min_children, min_weight,
                                   merge_cap(d), list, n_par, tslot, d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    return tsdf_sync(d);
}

extern "C" {

int tsdf_coarsen_count(tsdf_ctx* dst, tsdf_ctx* src, const int32_t lo[3], const int32_t hi[3],
                       int32_t side, uint32_t min_children, float min_weight,
                       tsdf_coarsen_stats* out) {
    return coarsen_impl(dst, src, lo, hi, side, min_children, min_weight, out, false);
}

int tsdf_coarsen_into(tsdf_ctx* dst, tsdf_ctx* src, const int32_t lo[3], const int32_t hi[3],
                      int32_t side, uint32_t min_children, float min_weight,
                      tsdf_coarsen_stats* out) {
    return coarsen_impl(dst, src, lo, hi, side, min_children, min_weight, out, true);
}

}  // extern "C"

// ---- removing bricks (include/tsdf_hip_prune.h; kernels in tsdf_prune.hip) --------

// One removal over the pool's n slots: the keep flags, their prefix and the lists it gives
// (launch_rm_scan), all in the call's scratch.
struct Removal {
    uint32_t n = 0;                        // pool slots before
    uint32_t new_count = 0, n_moves = 0;   // kept bricks; kept bricks that change slot
    uint32_t *keep = nullptr, *bsum = nullptr, *boff = nullptr, *res = nullptr, *rml = nullptr,
             *mover = nullptr;
    uint32_t removed() const { return n - new_count; }
};

static int removal_alloc(tsdf_ctx* c, Scratch& tmp, uint32_t n, Removal& M) {
    M.n = n;
    HIPCHK(c, tmp.get(c, &M.keep, n));
    HIPCHK(c, tmp.get(c, &M.bsum, rm_scan_blocks(n)));
    HIPCHK(c, tmp.get(c, &M.boff, rm_scan_blocks(n)));
    HIPCHK(c, tmp.get(c, &M.res, 2));
    HIPCHK(c, tmp.get(c, &M.rml, n));
    HIPCHK(c, tmp.get(c, &M.mover, n));
    return TSDF_OK;
}

// keep is written: rank the slots and read the counts back
static int removal_rank(tsdf_ctx* c, Removal& M) {
    uint32_t res[2] = {0u, 0u};
    HIPCHK(c, launch_rm_scan(M.keep, M.n, M.bsum, M.boff, M.res, M.rml, M.mover, c->stream));
    HIPCHK(c, hipMemcpyAsync(res, M.res, sizeof res, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    M.new_count = res[0];
    M.n_moves = res[1];
    if (M.new_count > M.n || M.n_moves > std::min(M.new_count, M.removed()))
        return fail(c, TSDF_EHIP, "removal: inconsistent ranks (%u of %u kept, %u moves)",
                    M.new_count, M.n, M.n_moves);
    return TSDF_OK;
}

// Fill the holes from the pool's tail and leave the context as the integrate path expects it.
// Nothing removed: nothing is touched.
static int removal_compact(tsdf_ctx* c, const Removal& M) {
    if (!M.removed()) return TSDF_OK;
    const Capacity& K = c->K;
    const uint64_t at = (uint64_t)M.new_count * BRICK_VOX, freed = (uint64_t)M.removed() * BRICK_VOX;
    HIPCHK(c, launch_rm_move(c->T, c->Pl, M.rml, M.mover, M.n_moves, c->stream));
    // fresh slots hold the background: tsdf_create fills the pool once and allocation (k_compact,
    // k_import_insert) hands slots out without touching their voxels
    HIPCHK(c, launch_fill(c->Pl.sdf + at, c->R.bg, freed, c->stream));
    HIPCHK(c, hipMemsetAsync(c->Pl.weight + at, 0, freed * sizeof(float), c->stream));
    // the table again from the slot -> key map, as after a capacity growth
    HIPCHK(c, launch_fill_u64(K.keys, EMPTY_KEY, K.cap, c->stream));
    HIPCHK(c, launch_fill_u32(K.slots, UNASSIGNED, K.cap, c->stream));
    // touched and cell[2] are indexed by table entry, and the entries move with the rebuild.
    // Between batches both are zero on the ordinary path: k_compact_write clears every touched
    // flag it lists (compact_list, clear = true), and k_integrate / k_integrate_small zero the
    // whole cell row of every brick of the batch's active list, committed or not.  What that
    // leaves out is a batch that overflowed a capacity that could not grow (a brick beyond the
    // active list or without a pool slot keeps its row, and TSDF_ENOMEM says that updates were
    // dropped).  A stale row under a moved entry would then corrupt another brick's sample
    // positions, so both arrays are cleared here as alloc_capacity leaves them, instead of relying
    // on every overflow path.
    const size_t cells = K.cap * c->plan.cell_stride *
                         (c->plan.fused ? sizeof(uint64_t) : sizeof(uint32_t));
    HIPCHK(c, hipMemsetAsync(K.touched, 0, K.cap * sizeof(uint32_t), c->stream));
    for (int q = 0; q < 2; q++) HIPCHK(c, hipMemsetAsync(K.cell[q], 0, cells, c->stream));
    HIPCHK(c, launch_rehash(c->T, M.new_count, c->G, c->stream));
    HIPCHK(c, hipMemcpyAsync(&c->G->pool_count, &M.new_count, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TSDF_OK;
}

// The entry checks the three calls share (those of tsdf_import_bricks) and the drained brick count
static int removal_enter(tsdf_ctx* c, const int32_t* lo, const int32_t* hi, bool box, uint64_t* nb) {
    if (border_busy(c)) return TSDF_EINVAL;
    if (box) {
        if (!lo || !hi) return fail(c, TSDF_EINVAL, "null box");
        for (int a = 0; a < 3; a++)
            if (lo[a] > hi[a]) return fail(c, TSDF_EINVAL, "box: lo > hi");
    }
    return pool_bricks(c, nb);
}

extern "C" {

int tsdf_prune(tsdf_ctx* c, float min_weight, uint64_t* n_removed) {
    if (!c) return TSDF_EINVAL;
    if (!(min_weight >= 0.0f)) return fail(c, TSDF_EINVAL, "prune: min_weight is negative or NaN");
    uint64_t nb = 0;
    int rc = removal_enter(c, nullptr, nullptr, false, &nb);
    if (rc) return rc;
    if (n_removed) *n_removed = 0;
    if (!nb) return TSDF_OK;
    Scratch tmp;
    Removal M;
    rc = removal_alloc(c, tmp, (uint32_t)nb, M);
    if (rc) return rc;
    HIPCHK(c, launch_rm_flag_prune(c->Pl, M.n, min_weight, c->R.bg, M.keep, c->stream));
    rc = removal_rank(c, M);
    if (rc) return rc;
    if (n_removed) *n_removed = M.removed();
    return removal_compact(c, M);
}

int tsdf_count_outside(tsdf_ctx* c, const int32_t lo[3], const int32_t hi[3], uint64_t* n) {
    if (!c || !n) return TSDF_EINVAL;
    uint64_t nb = 0;
    int rc = removal_enter(c, lo, hi, true, &nb);
    if (rc) return rc;
    *n = 0;
    if (!nb) return TSDF_OK;
    Scratch tmp;
    Removal M;
    rc = removal_alloc(c, tmp, (uint32_t)nb, M);
    if (rc) return rc;
    HIPCHK(c, launch_rm_flag_box(c->T, M.n, lo, hi, M.keep, c->stream));
    rc = removal_rank(c, M);
    if (rc) return rc;
    *n = M.removed();
    return TSDF_OK;
}

int tsdf_evict_outside(tsdf_ctx* c, const int32_t lo[3], const int32_t hi[3], int32_t* coords,
                       float* sdf, float* weight, uint64_t cap, uint64_t* n_out) {
    if (!c) return TSDF_EINVAL;
    uint64_t nb = 0;
    int rc = removal_enter(c, lo, hi, true, &nb);
    if (rc) return rc;
    if (n_out) *n_out = 0;
    if (!nb) return TSDF_OK;
    Scratch tmp;
    Removal M;
    rc = removal_alloc(c, tmp, (uint32_t)nb, M);
    if (rc) return rc;
    HIPCHK(c, launch_rm_flag_box(c->T, M.n, lo, hi, M.keep, c->stream));
    rc = removal_rank(c, M);
    if (rc) return rc;
    const uint64_t count = M.removed();
    if (n_out) *n_out = count;
    const bool want = coords || sdf || weight;
    if (want && count > cap)
        return fail(c, TSDF_EOVERFLOW, "evict needs %llu bricks", (unsigned long long)count);
    if (!count) return TSDF_OK;
    if (want) {  // the copy-out, before anything moves
        std::vector<uint64_t> keys(nb);
        std::vector<uint32_t> slots(count);
        HIPCHK(c, hipMemcpy(keys.data(), c->T.brick_keys, nb * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(slots.data(), M.rml, count * 4, hipMemcpyDeviceToHost));
        for (uint32_t s : slots)
            if (s >= nb) return fail(c, TSDF_EHIP, "removal: slot %u out of range", s);
        std::sort(slots.begin(), slots.end(),
                  [&](uint32_t a, uint32_t b) { return brick_key_less_zyx(keys[a], keys[b]); });
        if (coords)
            for (uint64_t i = 0; i < count; i++)
                for (int a = 0; a < 3; a++) coords[3 * i + a] = brick_key_coord(keys[slots[i]], a);
        const int arrays = (sdf ? 1 : 0) + (weight ? 1 : 0);
        if (arrays) {
            // the sorted slots take the place of the keep flags (ranked already; count <= n);
            // the pieces' size: prune_plan.h
            const uint64_t per = evict_piece_bricks(arrays);
            uint32_t* d_slots = M.keep;
            float *ds = nullptr, *dw = nullptr;
            HIPCHK(c, hipMemcpy(d_slots, slots.data(), count * 4, hipMemcpyHostToDevice));
            if (sdf) HIPCHK(c, tmp.get(c, &ds, std::min(per, count) * BRICK_VOX));
            if (weight) HIPCHK(c, tmp.get(c, &dw, std::min(per, count) * BRICK_VOX));
            for (uint64_t i0 = 0; i0 < count; i0 += per) {
                const uint64_t m = std::min(per, count - i0);
                HIPCHK(c, launch_rm_gather(c->Pl, d_slots + i0, (uint32_t)m, ds, dw, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                if (sdf)
                    HIPCHK(c, hipMemcpy(sdf + i0 * BRICK_VOX, ds, m * BRICK_VOX * 4, hipMemcpyDeviceToHost));
                if (weight)
                    HIPCHK(c, hipMemcpy(weight + i0 * BRICK_VOX, dw, m * BRICK_VOX * 4, hipMemcpyDeviceToHost));
            }
        }
    }
    return removal_compact(c, M);
}

int tsdf_get_stats(tsdf_ctx* c, tsdf_stats* out) {
    if (!c || !out) return TSDF_EINVAL;
    const int rc = drain(c);
    if (rc) return rc;
    Globals g;
    HIPCHK(c, hipMemcpy(&g, c->G, sizeof g, hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof *out);
    out->n_scans = c->n_scans;
    out->n_batches = c->n_batches;
    out->n_points_in = c->n_points_in;
    out->n_bricks = std::min<uint64_t>(g.pool_count, c->T.max_bricks);
    out->n_grows = c->n_grows;
    out->n_replayed = c->n_replayed;
    out->max_bricks = c->T.max_bricks;
    out->peer_mask = c->peer_mask;
    if (c->batch_id) {
        const Counters& L = g.last;
        out->n_active_last = L.n_active;
        for (int k = 0; k < 8; k++) {
            out->n_voxels_last += L.n_vox[k];
            out->n_pairs_last += L.n_pairs[k];
        }
    }
    for (int k = 0; k < 8; k++) {
        out->n_voxels_total += g.tot_vox[k];
        out->n_rays_total += g.tot_rays[k];
        out->n_dirty_total += g.tot_dirty[k];
    }
    if (c->timer)
        for (int k = 0; k < KIND_N; k++) {
            out->kernel_ms[k] = c->timer->ms[k];
            out->kernel_launches[k] = c->timer->launches[k];
        }
    return TSDF_OK;
}

int tsdf_reset_stats(tsdf_ctx* c) {
    if (!c) return TSDF_EINVAL;
    const int rc = drain(c);
    if (rc) return rc;
    if (c->timer) c->timer->reset();
    HIPCHK(c, hipMemset(c->G->tot_vox, 0, sizeof(c->G->tot_vox) * 4));
    c->n_points_in = 0;
    c->n_scans = 0;
    c->n_batches = 0;
    return TSDF_OK;
}

int tsdf_set_profiling(tsdf_ctx* c, int32_t on) {
    if (!c) return TSDF_EINVAL;
    const int rc = drain(c);
    if (rc) return rc;
    if (on && !c->timer) {
        c->timer = new (std::nothrow) EventTimer();
        if (c->timer) c->timer->per_batch = c->metrics != nullptr;
    }
    if (!on && c->timer) { delete c->timer; c->timer = nullptr; }
    return (on && !c->timer) ? TSDF_ENOMEM : TSDF_OK;
}

int tsdf_set_profiling_period(tsdf_ctx* c, uint32_t every_mask, uint32_t period) {
    if (!c) return TSDF_EINVAL;
    if (period == 0) return fail(c, TSDF_EINVAL, "profiling period must be >= 1");
    if (!c->timer) return fail(c, TSDF_EINVAL, "profiling is off (tsdf_set_profiling)");
    c->timer->every_mask = every_mask;
    c->timer->period = period;
    return TSDF_OK;
}

int tsdf_set_metrics_log(tsdf_ctx* c, const char* path) {
    if (!c) return TSDF_EINVAL;
    int rc = drain(c);  // report (or drop) what came before
    if (rc) return rc;
    if (c->metrics) {
        fclose(c->metrics);
        c->metrics = nullptr;
    }
    if (c->timer) c->timer->per_batch = false;
    c->metrics_info.clear();
    c->metrics_next = c->batch_id;
    if (!path || !*path) return TSDF_OK;
    c->metrics = fopen(path, "a");
    if (!c->metrics) return fail(c, TSDF_EINVAL, "cannot open metrics log %s", path);
    if (c->timer) c->timer->per_batch = true;
    return TSDF_OK;
}

int32_t tsdf_sector_of(float px, float py, const double origin[3], double yaw0,
                       uint32_t n_sectors) {
    if (!origin || n_sectors == 0) return -1;
    const float dx = px - (float)origin[0], dy = py - (float)origin[1];
    if (!(dx == dx) || !(dy == dy)) return -1;
    if (n_sectors == 1) return 0;
    // the sector whose [start, next start) holds a, cyclically
    for (uint32_t k = 0; k < n_sectors; k++) {
        RayConst R{};
        sector_bounds(yaw0, k, n_sectors, R);
        if (in_sector(R, dx, dy)) return (int32_t)k;
    }
    return -1;
}

int tsdf_select_sector(const float* xyz, uint64_t n, const double origin[3], double yaw0,
                       uint32_t sector, uint32_t n_sectors, float* out_xyz, uint64_t* n_out) {
    if (!xyz || !origin || !out_xyz || !n_out || n_sectors == 0 || sector >= n_sectors)
        return TSDF_EINVAL;
    RayConst R{};
    sector_bounds(yaw0, sector, n_sectors, R);
    const float ox = (float)origin[0], oy = (float)origin[1];
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (!in_sector(R, xyz[3 * i] - ox, xyz[3 * i + 1] - oy)) continue;
        std::memcpy(out_xyz + 3 * k, xyz + 3 * i, 12);
        k++;
    }
    *n_out = k;
    return TSDF_OK;
}

// ---- border-brick reduce (include/tsdf_hip.h; kernels in tsdf_border.hip) ----------------------

int tsdf_brick_keys_device(tsdf_ctx* c, uint64_t* d_keys, uint64_t cap, uint64_t* n_out) {
    if (!c || !n_out) return TSDF_EINVAL;
    uint64_t nb = 0;
    int rc = pool_bricks(c, &nb);
    if (rc) return rc;
    *n_out = nb;
    if (nb > cap) return fail(c, TSDF_EOVERFLOW, "brick keys need %llu entries", (unsigned long long)nb);
    if (!nb) return TSDF_OK;
    if (!d_keys) return fail(c, TSDF_EINVAL, "null key buffer");
    HIPCHK(c, hipMemcpyAsync(d_keys, c->T.brick_keys, nb * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TSDF_OK;
}

}  // extern "C"

// tsdf_border_pack_device's work.  The pool slots of the bricks it packed join the context's
// border transaction (brd_sent), for the commit's reset.
static int border_pack_impl(tsdf_ctx* c, const uint64_t* d_all_keys, const uint64_t* counts,
                            uint64_t stride, uint32_t world, uint32_t rank, uint32_t* d_send,
                            uint64_t cap_rows, uint64_t* send_counts) {
    if (!counts || !send_counts || world == 0 || world > TSDF_MAX_WORLD || rank >= world)
        return fail(c, TSDF_EINVAL, "bad world/rank or null counts");
    WorldCounts wc{};
    for (uint32_t r = 0; r < world; r++) {
        if (counts[r] > stride) return fail(c, TSDF_EINVAL, "counts[%u] > stride", r);
        wc.n[r] = counts[r];
        send_counts[r] = 0;
    }
    uint64_t nb = 0;
    int rc = pool_bricks(c, &nb);
    if (rc) return rc;
    if (!nb || rank == 0) return TSDF_OK;  // rank 0 owns everything it holds
    bool lower = false;
    for (uint32_t r = 0; r < rank; r++) lower |= wc.n[r] > 0;
    if (!lower) return TSDF_OK;
    if (!d_all_keys) return fail(c, TSDF_EINVAL, "null key buffer");
    Scratch tmp;
    uint32_t *d_owner = nullptr, *d_aux = nullptr, *d_rows = nullptr;
    uint32_t dest[MAX_WORLD] = {}, cursor[MAX_WORLD] = {};
    HIPCHK(c, tmp.get(c, &d_owner, nb));
    HIPCHK(c, tmp.get(c, &d_aux, 2 * MAX_WORLD));
    HIPCHK(c, launch_border_owner(c->T, (uint32_t)nb, d_all_keys, wc, stride, rank, d_owner, d_aux,
                                  c->stream));
    HIPCHK(c, hipMemcpyAsync(dest, d_aux, sizeof dest, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t rows = 0;
    for (uint32_t r = 0; r < world; r++) {
        cursor[r] = (uint32_t)rows;
        send_counts[r] = dest[r];
        rows += dest[r];
    }
    if (!d_send || !rows) return TSDF_OK;
    if (rows > cap_rows)
        return fail(c, TSDF_EOVERFLOW, "border pack needs %llu rows", (unsigned long long)rows);
    HIPCHK(c, tmp.get(c, &d_rows, rows));
    HIPCHK(c, hipMemcpyAsync(d_aux + MAX_WORLD, cursor, sizeof cursor, hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, launch_border_pack(c->T, c->Pl, c->R.bg, (uint32_t)nb, rank, d_owner, d_aux + MAX_WORLD,
                                 d_rows, (uint32_t)rows, d_send, /*reset=*/false, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->brd_sent.reset(tmp.take(d_rows));
    c->brd_n_sent = rows;
    return TSDF_OK;
}

static bool border_busy(tsdf_ctx* c) {
    if (!c->brd_open) return false;
    fail(c, TSDF_EINVAL, "a border reduce is open on this context: commit or abort it first "
                         "(tsdf_border_commit_device)");
    return true;
}

extern "C" {

// ABI v9: the pack no longer resets the sent bricks -- their mass stays here until
// tsdf_border_commit_device(ctx, 1) after the collective and every rank's merge succeeded; an
// abort keeps it.  The call opens the context's border transaction when it packs rows.
int tsdf_border_pack_device(tsdf_ctx* c, const uint64_t* d_all_keys, const uint64_t* counts,
                            uint64_t stride, uint32_t world, uint32_t rank, uint32_t* d_send,
                            uint64_t cap_rows, uint64_t* send_counts) {
    if (!c) return TSDF_EINVAL;
    if (c->brd_n_sent)
        return fail(c, TSDF_EINVAL, "border pack: the open reduce has packed already (commit first)");
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = border_pack_impl(c, d_all_keys, counts, stride, world, rank, d_send, cap_rows,
                                    send_counts);
    if (rc) return rc;
    if (d_send) c->brd_open = true;
    return TSDF_OK;
}

// The owner's merge of received tiles; the bricks it touches are snapshot first (ABI v9) so an
// aborted reduce restores them.
int tsdf_border_merge_device(tsdf_ctx* c, const uint32_t* d_recv, const uint64_t* recv_counts,
                             uint32_t world) {
    if (!c) return TSDF_EINVAL;
    if (!recv_counts || world == 0 || world > TSDF_MAX_WORLD)
        return fail(c, TSDF_EINVAL, "bad world or null counts");
    uint64_t total = 0;
    for (uint32_t r = 0; r < world; r++) total += recv_counts[r];
    c->brd_open = true;  // a merge is part of the reduce even when this rank received nothing
    if (!total) return TSDF_OK;
    if (!d_recv) return fail(c, TSDF_EINVAL, "null tile buffer");
    int rc = drain(c);
    if (rc) return rc;
    Scratch tmp;
    uint32_t* bk = nullptr;
    HIPCHK(c, tmp.get(c, &bk, total * TSDF_TILE_WORDS));
    // the backup joins the abort's restore list only once its snapshot is launched (a
    // failed launch left uninitialised rows for the restore to write over held bricks)
    HIPCHK(c, launch_border_snapshot(c->T, c->Pl, d_recv, total, bk, c->stream));
    c->brd_backup.emplace_back(DevBuf<uint32_t>(tmp.take(bk)), total);
    uint64_t row = 0;
    for (uint32_t r = 0; r < world; r++) {  // sources in ascending rank order
        if (recv_counts[r])
            HIPCHK(c, launch_border_merge(c->T, c->Pl, d_recv + row * TSDF_TILE_WORDS,
                                          recv_counts[r], c->G, merge_cap(c), c->stream));
        row += recv_counts[r];
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return tsdf_sync(c);
}

// ABI v9: close the context's border transaction.  commit = 1 (the collective and EVERY rank's
// merge succeeded): the bricks this rank sent are reset to the background -- their mass now lives
// at their owners.  commit = 0 (abort): the bricks the merges touched are written back as they
// were, the sent bricks keep their mass; the field is the one before the reduce, bit for bit.
int tsdf_border_commit_device(tsdf_ctx* c, int32_t commit) {
    if (!c) return TSDF_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    hipError_t e = hipSuccess;
    if (commit) {
        if (c->brd_n_sent)
            e = launch_border_reset(c->Pl, c->R.bg, c->brd_sent, (uint32_t)c->brd_n_sent, c->stream);
    } else {
        for (size_t k = c->brd_backup.size(); k-- > 0 && e == hipSuccess;)
            e = launch_border_restore(c->T, c->Pl, c->brd_backup[k].first, c->brd_backup[k].second,
                                      c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess)  // the transaction stays open: the caller may retry
        return fail(c, TSDF_EHIP, "border %s: %s", commit ? "commit" : "abort",
                    hipGetErrorString(e));
    c->brd_sent.reset();
    c->brd_n_sent = 0;
    c->brd_backup.clear();
    c->brd_open = false;
    return TSDF_OK;
}

// ---- one process, several GPUs (SURVEY §8b's num_gpus / device_ids) ------------------------------

int tsdf_create_sharded(const tsdf_params* p, uint32_t n, const int32_t* device_ids, tsdf_ctx** out) {
    if (!p || !out || n == 0 || n > TSDF_MAX_WORLD) return TSDF_EINVAL;
    DeviceGuard caller;  // the caller's device as it was
    for (uint32_t k = 0; k < n; k++) out[k] = nullptr;
    int rc = TSDF_OK;
    for (uint32_t k = 0; k < n && rc == TSDF_OK; k++) {
        tsdf_params q = *p;
        q.device_id = device_ids ? device_ids[k] : (int32_t)k;
        q.n_sectors = n > 1 ? n : 0;
        q.sector = k;
        rc = tsdf_create(&q, &out[k]);
        if (rc) {
            for (uint32_t j = 0; j < k; j++) {
                tsdf_destroy(out[j]);
                out[j] = nullptr;
            }
        }
    }
    // peer access between every pair of distinct devices that supports it, so the input fan-out
    // (tsdf_integrate_sectors) and the border reduce's tile copies go GPU to GPU over xGMI
    for (uint32_t k = 0; k < n && rc == TSDF_OK; k++) {
        tsdf_ctx* c = out[k];
        for (uint32_t j = 0; j < n; j++) {
            const int dk = c->device, dj = out[j]->device;
            if (dk == dj) {
                c->peer_mask |= 1ull << j;
                continue;
            }
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, dk, dj) != hipSuccess || !can) continue;
            if (hipSetDevice(dk) != hipSuccess) continue;
            const hipError_t e = hipDeviceEnablePeerAccess(dj, 0);
            if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) c->peer_mask |= 1ull << j;
            (void)hipGetLastError();  // an already-enabled pair leaves its error code behind
        }
    }
    return rc;
}

// The border reduce of tsdf_brick_keys_device / tsdf_border_pack_device / tsdf_border_merge_device
// among the contexts of one process: the keys meet on the host, and each source's tiles go to
// their owner's GPU with one peer copy per (source, owner) pair (xGMI between GPUs; a device copy
// when two contexts share a GPU).  Transactional (ABI v9): every context packs without
// resetting and every owner snapshots before it merges; only when every copy and merge succeeded
// are the sent bricks reset (commit), otherwise every context is rolled back (abort), so a failed
// reduce neither loses nor double-counts mass.  Synchronous.
int tsdf_border_reduce_local(tsdf_ctx* const* ctxs, uint32_t n, uint64_t* bricks_moved) {
    if (!ctxs_ok(ctxs, n)) return TSDF_EINVAL;
    if (bricks_moved) *bricks_moved = 0;
    if (n == 1) return TSDF_OK;
    for (uint32_t k = 0; k < n; k++)
        if (border_busy(ctxs[k])) return first_error(ctxs, n, TSDF_EINVAL);
    DeviceGuard caller;  // (restored after the buffers are freed on their devices)
    Scratch bufs;
    int rc = TSDF_OK;
    // 1. every context's keys, gathered on the host
    std::vector<uint64_t> counts(n, 0);
    std::vector<std::vector<uint64_t>> hkeys(n);
    for (uint32_t k = 0; k < n && !rc; k++) {
        tsdf_ctx* c = ctxs[k];
        uint64_t nb = 0;
        rc = pool_bricks(c, &nb);
        uint64_t* d = nullptr;
        if (!rc) rc = bufs.get_or_fail(c, &d, nb);
        if (!rc) rc = tsdf_brick_keys_device(c, d, nb, &counts[k]);
        if (!rc) {
            hkeys[k].resize(counts[k]);
            if (counts[k] &&
                hipMemcpy(hkeys[k].data(), d, counts[k] * 8, hipMemcpyDeviceToHost) != hipSuccess)
                rc = fail(c, TSDF_EHIP, "border reduce: key read-back failed");
        }
    }
    uint64_t stride = 1;
    for (uint32_t k = 0; k < n; k++) stride = std::max(stride, counts[k]);
    std::vector<uint64_t> all(stride * n, ~0ull);
    for (uint32_t k = 0; k < n; k++)
        std::copy(hkeys[k].begin(), hkeys[k].end(), all.begin() + k * stride);
    // 2. each context packs the bricks a lower rank owns (no reset: the transaction)
    std::vector<uint32_t*> send(n, nullptr);
    std::vector<std::vector<uint64_t>> sc(n, std::vector<uint64_t>(n, 0));
    for (uint32_t k = 0; k < n && !rc; k++) {
        tsdf_ctx* c = ctxs[k];
        uint64_t* dk = nullptr;
        rc = bufs.get_or_fail(c, &dk, all.size());
        if (!rc && hipMemcpy(dk, all.data(), all.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(c, TSDF_EHIP, "border reduce: key upload failed");
        if (!rc) rc = bufs.get_or_fail(c, &send[k], counts[k] * TSDF_TILE_WORDS);
        if (!rc)
            rc = tsdf_border_pack_device(c, dk, counts.data(), stride, n, k, send[k], counts[k],
                                         sc[k].data());
    }
    // 3. every owner d receives block d of every source, sources ascending; 4. merge
    uint64_t moved = 0;
    for (uint32_t d = 0; d < n && !rc; d++) {
        tsdf_ctx* c = ctxs[d];
        std::vector<uint64_t> rcnt(n, 0);
        uint64_t total = 0;
        for (uint32_t r = 0; r < n; r++) {
            rcnt[r] = sc[r][d];
            total += rcnt[r];
        }
        if (!total) continue;
        uint32_t* dr = nullptr;
        rc = bufs.get_or_fail(c, &dr, total * TSDF_TILE_WORDS);
        uint64_t row = 0;
        for (uint32_t r = 0; r < n && !rc; r++) {
            if (!rcnt[r]) continue;
            uint64_t off = 0;
            for (uint32_t q = 0; q < d; q++) off += sc[r][q];
            const hipError_t e = copy_between(c, dr + row * TSDF_TILE_WORDS, ctxs[r],
                                              send[r] + off * TSDF_TILE_WORDS,
                                              rcnt[r] * TSDF_TILE_WORDS * 4);
            if (e != hipSuccess)
                rc = fail(c, TSDF_EHIP, "border reduce: tile copy: %s", hipGetErrorString(e));
            row += rcnt[r];
        }
        if (!rc) rc = tsdf_border_merge_device(c, dr, rcnt.data(), n);
        moved += total;
    }
    // 5. commit everywhere when everything succeeded, else roll every context back
    const int commit = rc == TSDF_OK ? 1 : 0;
    for (uint32_t k = 0; k < n; k++) {
        const int crc = tsdf_border_commit_device(ctxs[k], commit);
        if (crc && !rc) rc = crc;
    }
    if (!rc && bricks_moved) *bricks_moved = moved;
    return rc ? first_error(ctxs, n, rc) : TSDF_OK;
}

// ---- mesh halo (ABI v9): meshing a sector-sharded field, one owner per cube ---------------------

// The keys of the bricks this context needs to mesh its own and does not observe: for every brick
// holding an observed voxel, its 7 +x / +y / +z neighbours that hold none here (sorted, unique).
int tsdf_halo_keys_device(tsdf_ctx* c, uint64_t* d_keys, uint64_t cap, uint64_t* n_out) {
    if (!c || !n_out) return TSDF_EINVAL;
    *n_out = 0;
    uint64_t nb = 0;
    int rc = drain(c);
    if (!rc) rc = pool_bricks(c, &nb);
    if (rc) return rc;
    if (!nb) return TSDF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint64_t> keys(nb);
    std::vector<uint32_t> obs(nb);
    Scratch tmp;
    uint32_t* d_obs = nullptr;
    HIPCHK(c, tmp.get(c, &d_obs, nb));
    HIPCHK(c, launch_brick_observed(c->Pl, (uint32_t)nb, d_obs, c->stream));
    HIPCHK(c, hipMemcpyAsync(obs.data(), d_obs, nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(keys.data(), c->T.brick_keys, nb * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<uint64_t> have;
    for (uint64_t i = 0; i < nb; i++)
        if (obs[i]) have.push_back(keys[i]);
    std::sort(have.begin(), have.end());
    const std::vector<uint64_t> need = brick_halo_needed(have);
    *n_out = need.size();
    if (need.size() > cap)
        return fail(c, TSDF_EOVERFLOW, "halo keys need %llu entries", (unsigned long long)need.size());
    if (need.empty()) return TSDF_OK;
    if (!d_keys) return fail(c, TSDF_EINVAL, "null key buffer");
    HIPCHK(c, hipMemcpy(d_keys, need.data(), need.size() * 8, hipMemcpyHostToDevice));
    return TSDF_OK;
}

// The tiles of the requested bricks (device keys) that this context observes, into d_send (device,
// cap_rows rows; row order unspecified); *n_rows = the tiles (TSDF_EOVERFLOW above cap_rows).
int tsdf_halo_pack_device(tsdf_ctx* c, const uint64_t* d_req, uint64_t n_req, uint32_t* d_send,
                          uint64_t cap_rows, uint64_t* n_rows) {
    if (!c || !n_rows) return TSDF_EINVAL;
    *n_rows = 0;
    if (!n_req) return TSDF_OK;
    if (!d_req || !d_send) return fail(c, TSDF_EINVAL, "null buffer");
    if (n_req >= 0xFFFFFFFFull || cap_rows >= 0xFFFFFFFFull)
        return fail(c, TSDF_EINVAL, "too many halo requests");
    int rc = drain(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Scratch tmp;
    uint32_t* d_n = nullptr;
    uint32_t nr = 0;
    HIPCHK(c, tmp.get(c, &d_n, 1));
    HIPCHK(c, hipMemsetAsync(d_n, 0, 4, c->stream));
    HIPCHK(c, launch_halo_pack(c->T, c->Pl, d_req, (uint32_t)n_req, d_send, (uint32_t)cap_rows, d_n,
                               c->stream));
    HIPCHK(c, hipMemcpyAsync(&nr, d_n, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_rows = nr;
    if (nr > cap_rows) return fail(c, TSDF_EOVERFLOW, "halo pack needs %u rows", nr);
    return TSDF_OK;
}

// tsdf_extract_mesh_table over this context's bricks, with the halo tiles (device) looked up first
// for their neighbours: after a border reduce, the union of every context's mesh is the mesh of
// the union field, each cube meshed by the owner of its min voxel's brick.
int tsdf_extract_mesh_halo(tsdf_ctx* c, float min_weight, int32_t table, const uint32_t* d_halo,
                           uint64_t n_halo, float* tri, uint64_t cap, uint64_t* n_tri) {
    return mesh_impl(c, min_weight, table, d_halo, n_halo, tri, cap, n_tri);
}

// The sharded mesh among the contexts of one process (2 cm + marching cubes on N
// GPUs): border reduce, halo exchange with one peer copy per (holder, requester) pair, one mesh per
// context; tri holds the contexts' soups one after another in context order (tri == NULL: count).
int tsdf_extract_mesh_local(tsdf_ctx* const* ctxs, uint32_t n, float min_weight, int32_t table,
                            float* tri, uint64_t cap, uint64_t* n_tri) {
    if (!ctxs_ok(ctxs, n) || !n_tri) return TSDF_EINVAL;
    *n_tri = 0;
    if (n == 1) return tsdf_extract_mesh_table(ctxs[0], min_weight, table, tri, cap, n_tri);
    int rc = tsdf_border_reduce_local(ctxs, n, nullptr);
    if (rc) return rc;
    DeviceGuard caller;  // (restored after the buffers are freed on their devices)
    Scratch bufs;
    // every context's requests
    std::vector<uint64_t*> req(n, nullptr);
    std::vector<uint64_t> nreq(n, 0);
    for (uint32_t k = 0; k < n && !rc; k++) {
        rc = tsdf_halo_keys_device(ctxs[k], nullptr, 0, &nreq[k]);
        if (rc == TSDF_EOVERFLOW) rc = TSDF_OK;
        if (!rc) rc = bufs.get_or_fail(ctxs[k], &req[k], nreq[k]);
        uint64_t got = 0;
        if (!rc) rc = tsdf_halo_keys_device(ctxs[k], req[k], nreq[k], &got);
    }
    // holder j packs for requester k on j's GPU; the tiles go to k's halo buffer
    std::vector<uint32_t*> halo(n, nullptr);
    std::vector<uint64_t> nh(n, 0);
    for (uint32_t k = 0; k < n && !rc; k++) {
        if (!nreq[k]) continue;
        rc = bufs.get_or_fail(ctxs[k], &halo[k], nreq[k] * TSDF_TILE_WORDS);
        for (uint32_t j = 0; j < n && !rc; j++) {
            if (j == k) continue;
            uint64_t* dq = nullptr;
            uint32_t* ds = nullptr;
            rc = bufs.get_or_fail(ctxs[j], &dq, nreq[k]);
            if (!rc) {
                const hipError_t e = copy_between(ctxs[j], dq, ctxs[k], req[k], nreq[k] * 8);
                if (e != hipSuccess)
                    rc = fail(ctxs[j], TSDF_EHIP, "halo: key copy: %s", hipGetErrorString(e));
            }
            if (!rc) rc = bufs.get_or_fail(ctxs[j], &ds, nreq[k] * TSDF_TILE_WORDS);
            uint64_t rows = 0;
            if (!rc) rc = tsdf_halo_pack_device(ctxs[j], dq, nreq[k], ds, nreq[k] - nh[k], &rows);
            if (!rc) {
                const hipError_t e = copy_between(ctxs[k], halo[k] + nh[k] * TSDF_TILE_WORDS, ctxs[j],
                                                  ds, rows * TSDF_TILE_WORDS * 4);
                if (e != hipSuccess)
                    rc = fail(ctxs[k], TSDF_EHIP, "halo: tile copy: %s", hipGetErrorString(e));
            }
            nh[k] += rows;
        }
    }
    // one mesh per context, soups concatenated
    uint64_t total = 0;
    for (uint32_t k = 0; k < n && !rc; k++) {
        uint64_t nt = 0;
        float* out = tri && total <= cap ? tri + 9 * total : nullptr;
        rc = mesh_impl(ctxs[k], min_weight, table, halo[k], nh[k], out,
                       tri && total <= cap ? cap - total : 0, &nt);
        if (rc == TSDF_EOVERFLOW) rc = TSDF_OK;  // the total decides below
        total += nt;
    }
    *n_tri = total;
    if (!rc && tri && total > cap)
        rc = fail(ctxs[0], TSDF_EOVERFLOW, "mesh has %llu triangles", (unsigned long long)total);
    return rc ? first_error(ctxs, n, rc) : TSDF_OK;
}

}  // extern "C"
