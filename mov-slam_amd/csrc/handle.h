// Internal to libmovba (not part of include/): the handle behind the C-ABI and the host helpers that api.cpp and upload.cpp
// share.  movba_handle's layout depends on MOVBA_TEST_HOOKS: every translation unit of one library that includes this header
// is compiled with the same setting (csrc/Makefile: the *_hooks.o objects).
//
// Nothing declared here is exported: the functions defined out of line are hidden, the small ones are static inline.
#pragma once
#include <hip/hip_runtime.h>
#include <sched.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "device_types.h"
#include "movba.h"
#include "structure.h"

#define MOVBA_INTERNAL __attribute__((visibility("hidden")))

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            std::fprintf(stderr, "libmovba: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return MOVBA_ERR_HIP;                                                             \
        }                                                                                     \
    } while (0)

namespace movba {

constexpr int kPhaseEvents = 16;
constexpr int kMaxGroups = 4;

static inline double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// between two looks at a word the device writes: spin (lowest latency: the LM chain is ~100 us per trial), or give the
// core away (movba_options::host_wait = 1: the LocalMapping thread then does not starve a Tracking thread it shares a core with)
static inline void host_relax(int mode)
{
    if (mode == 1) { sched_yield(); return; }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
}

// Words the device writes into pinned host memory while the host polls them (k_decide's progress word, the PCG's park
// counter, the structure pass's sequence number): read with acquire loads — what is published before them (the counts, the
// controller's copy) is read after them — and written from the host with release stores.
static inline uint64_t rd_progress(const HostStatus *hs) { return __atomic_load_n(&hs->progress, __ATOMIC_ACQUIRE); }
static inline int32_t rd_pause(const HostStatus *hs) { return __atomic_load_n(&hs->pause_seq, __ATOMIC_ACQUIRE); }
static inline void wr_stop(HostStatus *hs, int32_t v) { __atomic_store_n(&hs->stop, v, __ATOMIC_RELEASE); }
static inline bool caller_stop(const volatile uint8_t *p) { return p && __atomic_load_n(p, __ATOMIC_RELAXED) != 0; }

struct MOVBA_INTERNAL Carver {
    size_t off = 0;
    template <typename T> size_t take(size_t count)
    {
        const size_t o = off;
        off = align_up(off + count * sizeof(T), 256);
        return o;
    }
};

// Diagnostic switches of the PROCESS, read from the environment once (api.cpp: process_switches, the one place that reads it)
struct ProcessSwitches {
    double watchdog_ms = 60000.0;
    bool time_upload = false, time_solve = false, dense_stamps = false, dense_multilaunch = false;
    int band = -1, batch_groups = 0;
};
MOVBA_INTERNAL const ProcessSwitches &process_switches();

// Everything a TEST switches is a per-handle hook of the test build only: -DMOVBA_TEST_HOOKS, libmovba_hooks.so,
// movba_test_hook().  The product library has neither the symbol nor the branches.
struct TestHooks {
    int host_structure = 0;         // structure pass on the host even where the device would build it
    int host_grouping = 0;          // grouping pass (build_basic) on the calling thread even where the device would run it
    int entries_unpacked = 0;       // 12-byte schur entries where the 8-byte packed form would do
    int no_sorted_structure = 0;    // beyond the pair-bin masks: host structure pass instead of the sort-based device pass
    int pcg_packed = 0;             // packed layout of the PCG's pair sums where the padded one would do
    int helper_delay_us = 0;        // the upload's helper thread starts that much later (its early-setup launches too)
    long long wait_ticks = -1;      // >= 0: bound of the in-launch waits of a run's FIRST attempt (10 ns ticks)
    int band_park_trial = -1;       // >= 0: k_band treats that trial's factorisation as one that met a non-positive pivot
    // what the last movba_lba_run_batch over this handle launched with (written by the call, read as hook "batch_variant"):
    // bit 0 ldsp, 1 overflow, 2 padded, 3 stereo (the fold over the batched windows; 0 where none was batched), bits 4-7 the
    // number of stream groups, bit 8: the window was in the batched launches, bit 9: it ran on its own behind them
    int batch_variant = 0;
};
#ifdef MOVBA_TEST_HOOKS
#define HOOK(h, field) ((h)->hooks.field)
#else
static constexpr TestHooks kNoHooks{};
#define HOOK(h, field) (movba::kNoHooks.field)
#endif

struct EventPair { hipEvent_t a, b; int cls; };

// One helper thread per handle: copies the caller's big arrays into the pinned staging buffer while the calling thread
// runs the grouping / validation pass over the edges (both are memory-bound single-thread loops of ~0.1 ms at cfg3).
// Sleeps on a condition variable between uploads.  (api.cpp)
struct Worker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<void()> job;
    int state = 0;              // 0 idle, 1 job posted, 2 job done
    bool quit = false;
    std::atomic<int> posted{0}; // set with state = 1: what the thread polls while it stays awake between jobs
    int spin_ms = 4;            // how long it stays awake after a job (0 with movba_options::host_wait = 1: it sleeps at once)
    MOVBA_INTERNAL void post(std::function<void()> j);
    MOVBA_INTERNAL void wait();
    MOVBA_INTERNAL ~Worker();
};

// A buffer of the handle that is grown on demand and never shrunk: device memory or pinned host memory (default flags).
// One policy for all of them (api.cpp): a quarter more than asked for, rounded up to 1 MiB, and both of the handle's
// streams drained before the old block is freed.  No destructor: movba_destroy releases them behind its own drains.
struct Scratch {
    enum Kind { Device, Pinned };
    char *p = nullptr;
    size_t cap = 0;
    Kind kind = Device;
    MOVBA_INTERNAL int grow(movba_handle *h, size_t bytes);
    MOVBA_INTERNAL void release();
};

// arena / pinned staging buffer of a handle grown to `bytes` (never shrunk; both streams drained first)
MOVBA_INTERNAL int ensure_arena(movba_handle *h, size_t bytes);
MOVBA_INTERNAL int ensure_stage(movba_handle *h, size_t bytes);
// The front of every call that borrows the staging buffer and the pose scratch beside the LBA calls (movba_pose_opt,
// movba_pose_opt_batch, movba_triangulate, the front of movba_two_view / movba_two_view_lo, movba_init_map, movba_view_points,
// movba_point_normals, movba_lba_point_normals, movba_covisibility, movba_track_match, movba_express, movba_advance, movba_mv_raster, movba_lk_track, movba_stereo_points): the device is set, the pose scratch holds dev_bytes (0: the call needs no
// device copy yet) and the staging buffer stage_bytes, and nothing of an earlier call or upload is still using either.
MOVBA_INTERNAL int begin_side_call(movba_handle *h, size_t dev_bytes, size_t stage_bytes);
// device view of [p, p + bytes) if it lies inside a movba_host_alloc block, else nullptr
MOVBA_INTERNAL unsigned long long *host_block_view(const void *p, size_t bytes);

// typed view of the bytes at `off` of a buffer (device-only scratch, the side calls' fixed-size records)
template <typename T> T *at(char *base, size_t off) { return reinterpret_cast<T *>(base + off); }

// One input array of a side call: `count` elements in the staging buffer, mirrored into the pose scratch by the call's one H2D
// copy.  An optional array that is absent is plan(0, c): the layout stays where it is, fill copies nothing, `dev` is nullptr.
template <typename T> struct In {
    size_t off = 0, count = 0;
    void plan(size_t n, Carver &c) { count = n; off = c.take<T>(n); }
    T *host(char *stage) const { return at<T>(stage, off); }   // (inputs the host computes in place)
    void fill(char *stage, const T *src) const { if (count) std::memcpy(stage + off, src, sizeof(T) * count); }
    const T *dev(char *arena) const { return count ? at<T>(arena, off) : nullptr; }
};

// One result array of the caller: written by the kernels where it lies (movba_host_alloc memory), or into the staging buffer
// and copied out behind the synchronisation; `dev` stays nullptr for an array the caller left out.
template <typename T> struct Out {
    T *user = nullptr, *dev = nullptr;
    size_t off = 0, count = 0;
    bool staged = false;
    void plan(T *p, size_t n, Carver &c)
    {
        user = p; count = n;
        if (!p || !n) return;
        dev = reinterpret_cast<T *>(host_block_view(p, sizeof(T) * n));
        staged = !dev;
        if (staged) off = c.take<T>(n);
    }
    // one pair's array: elements [first, first + n) of what the call carved for all pairs at base_off, unless it lies in
    // movba_host_alloc memory (a pair the kernels skip, n == 0, keeps its empty slice)
    void plan_within(T *p, size_t n, size_t base_off, size_t first)
    {
        user = p; count = n;
        if (!p) return;
        if (n) dev = reinterpret_cast<T *>(host_block_view(p, sizeof(T) * n));
        staged = !dev;
        off = base_off + sizeof(T) * first;
    }
    void bind(char *stage_dev) { if (staged) dev = at<T>(stage_dev, off); }
    void fetch(const char *stage) const { if (staged) std::memcpy(user, stage + off, sizeof(T) * count); }
};

}  // namespace movba

struct movba_handle {
    int device = 0;
    int device_cus = 256;               // compute units of the device (or of this process's partition of it): bounds the one-launch direct solver's workgroups
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t copy_stream = nullptr;  // H2D of the caller's arrays, issued by the helper thread of movba_lba_upload (shared by the
                                        // handles of a device: every extra stream of the process competes for the few hardware queues,
                                        // and two streams of a batched run that land on one queue run in turns)
    hipEvent_t copy_event = nullptr;
#ifdef MOVBA_TEST_HOOKS
    movba::TestHooks hooks;             // (test build only: movba_test_hook)
#endif
    unsigned *ingest_counter = nullptr; // device word: workgroups of k_ingest that are through (IngestArgs::counter), never reset
    unsigned ingest_expect = 0;         // its value once every launch queued so far is through
    bool early_setup = false;           // the upload has queued k_init_pose and the first linearisation itself (behind the edge data, in
                                        // the shadow of its own pair layout): the next run starts with the Hpp pass
    int sync_retries = 0;               // > 0: this run's first attempt gave up that many in-launch waits and was repeated on the paths without any
    hipEvent_t edgeb_event = nullptr;   // the derived edge arrays sent early on the copy stream have arrived; device grouping pass: the
                                        // index arrays have been read out of host memory (the big arrays' DMA starts behind it)
    uint64_t count_seq = 0;             // uploads that went through the device structure pass (what the host polls for in the counts buffer)
    movba_options opt{};
    // device arena
    char *arena = nullptr;
    size_t arena_cap = 0;
    uint64_t arena_gen = 0;             // bumped by every (re)allocation: hipFree + hipMalloc may return the same address
    // pinned staging
    char *stage = nullptr;
    size_t stage_cap = 0;
    movba::HostStatus *hstat = nullptr; // pinned, mapped
    movba::HostStatus *hstat_dev = nullptr;
    movba::Ctrl *ctrl_host = nullptr;   // pinned copy of the device Ctrl
    movba::Ctrl *ctrl_host_dev = nullptr;       // its device view (written by k_finalize)
    double *pose_export = nullptr;      // registered device buffer for the final poses
    int64_t pose_export_cap = 0;
    char *stage_dev = nullptr;          // device view of the pinned staging buffer (written by k_export)
    // current window
    bool uploaded = false, ran = false;
    bool export_in_run = false;         // this run's results were written to the staging buffer behind its last kernel
    bool export_hint = false;           // set by movba_lba_solve around its run: a download follows at once
    // movba_lba_solve: result arrays of the caller that lie in movba_host_alloc memory (poses, points, chi2): device view
    // the export kernel writes to, and the host pointer it stands for (download skips the copy-out of exactly that array)
    unsigned long long *user_dst[3] = {nullptr, nullptr, nullptr};
    const void *user_host[3] = {nullptr, nullptr, nullptr};
    bool exported[3] = {true, true, true};      // which of poses / points / chi2 the run's export wrote (the caller asked for)
    movba::Structure st;
    movba::DevWindow win{};
    size_t h2d_bytes = 0;
    const volatile uint8_t *stop = nullptr;
    int early_status = MOVBA_OK;        // decided at upload (MOVBA_EMPTY / MOVBA_NO_FIXED): holds for every run of the window
    int run_status = MOVBA_OK;          // decided per run (MOVBA_STOPPED when the flag was up before the solve)
    movba::PcgParams pp{};
    bool rows_kernel = false;
    bool band = false;                  // this window's reduced system is solved by the single-workgroup banded factorisation (band_kernel.hip)
    int band_bw = 0;                    // its half bandwidth in blocks
    movba::DensePlan dplan;             // static schedule of the one-launch direct solver (kept across uploads of the same size)
    int dplan_nt = -1;
    bool dense_flags_clean = false;     // the window's hand-off flags have been zeroed since its upload (done before the first direct launch)
    unsigned dense_epoch = 0;           // direct launches on this window so far: the value a flag of the current launch carries
    movba::Scratch scratch;             // structure-pass temporaries (struct_kernels.hip)
    movba::Scratch scratch2;            // ... of the sort-based fill (struct_sort.hip): keys, values, rocPRIM's temporary storage
    // movba_lba_run_batch (kept by the first handle of a batch): device views, PCG plans and block prefixes of the windows
    movba::Scratch batch_host{nullptr, 0, movba::Scratch::Pinned}, batch_dev;
    hipStream_t batch_streams[movba::kMaxGroups] = {};  // extra streams of a batched run (groups of windows run out of phase); [0] unused
    hipEvent_t batch_ev[movba::kMaxGroups + 1] = {};    // [0]: fork from the callers' stream, [g]: join of group g
    hipEvent_t batch_phase_ev[movba::kMaxGroups][movba::kPhaseEvents] = {};     // ring: end of group g's schur launch of trial t (t mod 16)
    movba::Scratch pose_scratch;        // device scratch of the side calls (begin_side_call)
#ifdef MOVBA_CLOCK_STAMP
    movba::Scratch stamp;               // diagnostic build only: the clock stamps' buffer (api.cpp: stamp_window, stamp_pose)
#endif
    // movba_lba_marginals (marginals.cpp): device scratch (controller, factor inverses, W, sigma, outputs) and the pinned image of
    // the outputs; the uploaded window's fixed flags (fixed keyframes get zero blocks)
    movba::Scratch marg, marg_host{nullptr, 0, movba::Scratch::Pinned};
    std::vector<uint8_t> pose_fixed;
    movba::Worker packer;               // helper thread of movba_lba_upload
    // profiling
    std::vector<movba::EventPair> ev_used;
    std::vector<hipEvent_t> ev_pool;
    movba_profile prof{};
};
