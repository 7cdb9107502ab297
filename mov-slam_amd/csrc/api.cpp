// C-ABI of libmovba.so (include/movba.h): handle, HBM arena, run / download and the host side of the LM loop (the upload
// is upload.cpp).  The host only feeds the stream: every numerical decision
// (gain ratio, accept/reject, lambda) is taken on the device by k_decide, which publishes
// its progress in pinned host memory so the host can stay a bounded number of trial sets
// ahead without a stream synchronise per trial.
//
// Replaces, behind Optimizer::LocalBundleAdjustment (/root/reference/src/Optimizer.cc:461-841),
// the g2o objects set up at :532-545 and driven at :754-755, and the gate at :757-775.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "handle.h"
#include "kernels.h"
#include "pose_kernels.h"

using namespace movba;

namespace {

enum KernelClass { KC_SCHUR = 0, KC_PCG, KC_BACKSUB, KC_DECIDE, KC_SETUP, KC_FINALIZE };
const char *kKernelNames[MOVBA_NKERNELS] = { "k_schur", "k_pcg", "k_point<backsub>", "k_decide", "setup(init+linearize+lambda)", "k_finalize" };

// blocks handed out by movba_host_alloc: host address range -> device view (process-wide, a handful of entries)
struct HostBlock { char *host; size_t bytes; char *dev; };
std::mutex g_host_blocks_mu;
std::vector<HostBlock> g_host_blocks;

}  // namespace

namespace movba {

void Worker::post(std::function<void()> j)
{
    if (!th.joinable())
        th = std::thread([this] {
            std::unique_lock<std::mutex> lk(m);
            for (;;) {
                // stay awake for a moment after a job: back-to-back uploads find the thread running instead of paying a
                // futex wake-up (tens to hundreds of microseconds) for 70 us of copying
                if (state != 1 && !quit) {
                    lk.unlock();
                    const auto t_spin = std::chrono::steady_clock::now();
                    while (posted.load(std::memory_order_acquire) == 0 &&
                           std::chrono::steady_clock::now() - t_spin < std::chrono::milliseconds(spin_ms)) {
#if defined(__x86_64__)
                        __builtin_ia32_pause();
#endif
                    }
                    lk.lock();
                }
                cv.wait(lk, [&] { return state == 1 || quit; });
                posted.store(0, std::memory_order_relaxed);
                if (quit) return;
                std::function<void()> jb = std::move(job);
                lk.unlock();
                jb();
                lk.lock();
                state = 2;
                cv.notify_all();
            }
        });
    { std::lock_guard<std::mutex> lk(m); job = std::move(j); state = 1; posted.store(1, std::memory_order_release); }
    cv.notify_all();
}

void Worker::wait()
{
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return state != 1; });
    state = 0;
}

Worker::~Worker()
{
    if (th.joinable()) {
        { std::lock_guard<std::mutex> lk(m); quit = true; }
        cv.notify_all();
        th.join();
    }
}

// Diagnostic switches of the PROCESS, read from the environment once, at their first use (never on the path of a solve):
//   MOVBA_WATCHDOG_MS        host gives up a device that makes no progress for that long (default 60 000)
//   MOVBA_TIME_UPLOAD / MOVBA_TIME_SOLVE   print the phases of every upload / solve call to stderr
//   MOVBA_DENSE_STAMPS       the one-launch direct solver records its tasks' clock stamps
//   MOVBA_DENSE_MULTILAUNCH  the direct solver one launch per block column (dense_solve.hip) for every window
//   MOVBA_BAND = 0 / 1       banded factorisation never / wherever its band fits (handles made with solver = 0)
//   MOVBA_BATCH_GROUPS       number of stream groups of a batched run
// Everything a TEST switches (structure pass on the host, entry formats, a late helper thread, short device-side waits, a
// smaller device, a forced park of k_band) is a per-handle hook of the test build only (handle.h: TestHooks).
const ProcessSwitches &process_switches()
{
    static const ProcessSwitches sw = [] {
        ProcessSwitches v;
        if (const char *e = std::getenv("MOVBA_WATCHDOG_MS")) { const double x = std::atof(e); if (x > 0.0) v.watchdog_ms = x; }
        v.time_upload = std::getenv("MOVBA_TIME_UPLOAD") != nullptr; v.time_solve = std::getenv("MOVBA_TIME_SOLVE") != nullptr;
        v.dense_stamps = std::getenv("MOVBA_DENSE_STAMPS") != nullptr; v.dense_multilaunch = std::getenv("MOVBA_DENSE_MULTILAUNCH") != nullptr;
        if (const char *e = std::getenv("MOVBA_BAND")) v.band = std::atoi(e);
        if (const char *e = std::getenv("MOVBA_BATCH_GROUPS")) v.batch_groups = std::atoi(e);
        return v;
    }();
    return sw;
}

int ensure_arena(movba_handle *h, size_t bytes)
{
    if (bytes <= h->arena_cap) return MOVBA_OK;
    if (h->arena) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (h->copy_stream) HIP_TRY(hipStreamSynchronize(h->copy_stream));
        HIP_TRY(hipFree(h->arena)); h->arena = nullptr; h->arena_cap = 0;
    }
    const size_t cap = align_up(bytes + bytes / 4, 1 << 20);
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&h->arena), cap));
    h->arena_cap = cap;
    h->arena_gen += 1;
    return MOVBA_OK;
}

int ensure_stage(movba_handle *h, size_t bytes)
{
    if (bytes <= h->stage_cap) return MOVBA_OK;
    if (h->stage) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (h->copy_stream) HIP_TRY(hipStreamSynchronize(h->copy_stream));
        HIP_TRY(hipHostFree(h->stage)); h->stage = nullptr; h->stage_cap = 0;
    }
    const size_t cap = align_up(bytes + bytes / 4, 1 << 20);
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h->stage), cap, hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&h->stage_dev), h->stage, 0));
    h->stage_cap = cap;
    return MOVBA_OK;
}

int Scratch::grow(movba_handle *h, size_t bytes)
{
    if (bytes <= cap) return MOVBA_OK;
    if (p) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (h->copy_stream) HIP_TRY(hipStreamSynchronize(h->copy_stream));
        release();
    }
    const size_t c = align_up(bytes + bytes / 4, 1 << 20);
    if (kind == Device) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), c));
    else HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&p), c, hipHostMallocDefault));
    cap = c;
    return MOVBA_OK;
}

void Scratch::release()
{
    if (p) (void)(kind == Device ? hipFree(p) : hipHostFree(p));
    p = nullptr; cap = 0;
}

int begin_side_call(movba_handle *h, size_t dev_bytes, size_t stage_bytes)
{
    HIP_TRY(hipSetDevice(h->device));
    if (dev_bytes) { const int rc = h->pose_scratch.grow(h, dev_bytes); if (rc) return rc; }
    const int rc = ensure_stage(h, stage_bytes); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    // (a window uploaded on this handle and not run yet: its arrays may still be crossing the bus out of the staging buffer)
    HIP_TRY(hipEventSynchronize(h->copy_event));
    h->export_in_run = false;        // (results a run may have left in the staging buffer are overwritten here: download exports again)
    return MOVBA_OK;
}

// device view of [p, p + bytes) if it lies inside a movba_host_alloc block, else nullptr
unsigned long long *host_block_view(const void *p, size_t bytes)
{
    if (!p) return nullptr;
    const char *c = static_cast<const char *>(p);
    std::lock_guard<std::mutex> lk(g_host_blocks_mu);
    for (const HostBlock &b : g_host_blocks)
        if (c >= b.host && c + bytes <= b.host + b.bytes) return reinterpret_cast<unsigned long long *>(b.dev + (c - b.host));
    return nullptr;
}

}  // namespace movba

#ifdef MOVBA_CLOCK_STAMP
// Host side of the diagnostic build's clock stamps (clock_stamp.h), all of it: the handle's stamp buffer - the pose call's
// segment slots first, then the window's segment slots and records - its report lines, and the one function that hands a
// run's records to the caller (declared by the scripts that call it, not by include/movba.h).
namespace movba {

static size_t stamp_words(const StampBuf &b) { return (size_t)b.n_seg + 8 * ((size_t)b.n_rec[kStampPoint] + (size_t)b.n_rec[kStampSchur]); }

// the uploaded window's part: capacities from the grids its launches use (launch_backsub, launch_schur), zeroed.  Called at the
// upload and again at the start of every run of the window, solo or in a batch (where k_init_pose used to zero Ctrl's words):
// a run's report and records are its own
int stamp_window(movba_handle *h)
{
    if (h->early_status != MOVBA_OK) return MOVBA_OK;
    DevWindow &w = h->win;
    StampBuf b{};
    b.n_seg = kSegSlots;
    b.n_rec[kStampPoint] = w.n_pt_blocks + 1;
    b.n_rec[kStampSchur] = w.nitems > 0 ? schur_blocks(w) * kSchurWaves : 0;
    const int rc = h->stamp.grow(h, sizeof(unsigned long long) * (kPoseSegSlots + stamp_words(b))); if (rc) return rc;
    b.words = reinterpret_cast<unsigned long long *>(h->stamp.p) + kPoseSegSlots;
    HIP_TRY(hipMemsetAsync(b.words, 0, sizeof(unsigned long long) * stamp_words(b), h->stream));
    w.stamp = b;
    return MOVBA_OK;
}

int stamp_pose(movba_handle *h, PoseDev &p)
{
    const int rc = h->stamp.grow(h, sizeof(unsigned long long) * kPoseSegSlots); if (rc) return rc;
    p.stamp = StampBuf{};
    p.stamp.words = reinterpret_cast<unsigned long long *>(h->stamp.p);
    p.stamp.n_seg = kPoseSegSlots;
    HIP_TRY(hipMemsetAsync(p.stamp.words, 0, sizeof(unsigned long long) * kPoseSegSlots, h->stream));
    return MOVBA_OK;
}

void stamp_report_run(movba_handle *h)
{
    unsigned long long s[kSegSlots];
    if (!h->win.stamp.words || hipMemcpy(s, h->win.stamp.words, sizeof(s), hipMemcpyDeviceToHost) != hipSuccess) return;
    const double iters = h->ctrl_host->pcg_total_iters ? h->ctrl_host->pcg_total_iters : 1, solves = h->ctrl_host->n_solves ? h->ctrl_host->n_solves : 1;
    std::fprintf(stderr, "libmovba[stamp]: k_pcg_rows %llu shader cycles in %llu x 10 ns -> %.3f GHz\n", s[kSegCycles], s[kSegTicks],
                 s[kSegTicks] ? 0.1 * (double)s[kSegCycles] / (double)s[kSegTicks] : 0.0);
    std::fprintf(stderr, "libmovba[stamp]: per-iteration segments (wave 0, cycles):");
    for (int k = 0; k < 8; ++k) std::fprintf(stderr, " s%d=%.0f", k, (double)s[kSegIter + k] / iters);
    for (int wv = 0; wv < 8; ++wv) {
        std::fprintf(stderr, "\nlibmovba[stamp]:   wave %d:", wv);
        for (int k = 0; k < 8; ++k) std::fprintf(stderr, " s%d=%.0f", k, (double)s[kSegWave + 8 * wv + k] / iters);
    }
    std::fprintf(stderr, "\nlibmovba[stamp]: setup phases per launch (cycles):");
    for (int k = 0; k < 8; ++k) std::fprintf(stderr, " p%d=%.0f", k, (double)s[kSegPhase + k] / solves);
    std::fprintf(stderr, "\n");
}

void stamp_report_pose(movba_handle *h, int lm_iters)
{
    unsigned long long s[kPoseSegSlots];
    if (hipMemcpy(s, h->stamp.p, sizeof(s), hipMemcpyDeviceToHost) != hipSuccess) return;
    std::fprintf(stderr, "libmovba[stamp]: k_pose_opt, cycles per LM iteration (%d): system pass %.0f, reduction of 28 %.0f, solve + update %.0f, cost pass + reduction %.0f\n",
                 lm_iters, (double)s[0] / lm_iters, (double)s[1] / lm_iters, (double)s[2] / lm_iters, (double)s[3] / lm_iters);
}

}  // namespace movba

// The records of one class (0: the back-substitution pass, per workgroup; 1: k_schur, per wave; 2: the segment slots, eight to a
// record) that the handle's last run left: up to `cap` records of eight words into `out`.  Returns how many records the class
// has - its launch grid - or an error.
extern "C" int movba_stamp_records(movba_handle *h, int cls, unsigned long long *out, int cap)
{
    if (!h || cls < 0 || (cls >= kStampClasses && cls != kStampSegments) || cap < 0 || (cap > 0 && !out)) return MOVBA_ERR_ARG;
    const StampBuf &b = h->win.stamp;
    if (!h->ran || !b.words) return MOVBA_ERR_STATE;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int have = cls == kStampSegments ? b.n_seg / 8 : b.n_rec[cls];
    const unsigned long long *src = cls == kStampSegments ? b.words : b.words + b.n_seg + 8 * (size_t)(cls == kStampSchur ? b.n_rec[kStampPoint] : 0);
    const int n = std::min(cap, have);
    if (n > 0) HIP_TRY(hipMemcpy(out, src, sizeof(unsigned long long) * 8 * (size_t)n, hipMemcpyDeviceToHost));
    return have;
}
#endif

namespace {

// One launch of the one-launch direct solver at a time per device.  Its workgroups wait for one another, which is safe while all
// of them are resident (<= 248 of the 256 CUs); two such launches dispatched at the same moment from two streams could each get
// part of the chip and wait for workgroups that cannot start until the other gives way - until the 20 ms clock ends both with
// MOVBA_ERR_DEVICE_WAIT.  As long as ONE stream uses the solver on a device (MoV-SLAM: the LocalMapping thread) nothing is
// added; from the moment a second stream does, every launch waits for the one before it through an event.
struct DenseGate {
    std::mutex mu;
    hipStream_t only_stream = nullptr;      // single mode: the one stream that has launched the solver on this device
    bool multi = false;
    hipEvent_t ev = nullptr;                // multi mode: completion of the latest launch, whichever stream it was on
    bool ev_recorded = false;
};
DenseGate &dense_gate(int device) { static DenseGate gates[32]; return gates[device & 31]; }

// one copy stream per device for all handles (created on first use, kept for the life of the process)
hipStream_t shared_copy_stream(int device)
{
    static std::mutex mu;
    static std::vector<hipStream_t> streams;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)streams.size() <= device) streams.resize(device + 1, nullptr);
    if (!streams[device] && hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking) != hipSuccess) streams[device] = nullptr;
    return streams[device];
}

// how long the device may go without ANY progress (a changed progress word, or new work queued) before the host gives up
inline double watchdog_ms() { return process_switches().watchdog_ms; }

hipEvent_t get_event(movba_handle *h)
{
    if (!h->ev_pool.empty()) { hipEvent_t e = h->ev_pool.back(); h->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

struct ScopedEvents {
    movba_handle *h; EventPair p{}; bool on; hipStream_t st;
    ScopedEvents(movba_handle *h_, int cls, hipStream_t st_ = nullptr) : h(h_), on(((h_->opt.profile >> cls) & 1) != 0), st(st_ ? st_ : h_->stream)
    {
        if (!on) return;
        p.a = get_event(h); p.b = get_event(h); p.cls = cls;
        if (!p.a || !p.b) { on = false; return; }
        (void)hipEventRecord(p.a, st);
    }
    ~ScopedEvents()
    {
        if (!on) return;
        (void)hipEventRecord(p.b, st);
        h->ev_used.push_back(p);
    }
};

void harvest_events(movba_handle *h)
{
    for (const EventPair &p : h->ev_used) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            h->prof.ms[p.cls] += ms;
            h->prof.launches[p.cls] += 1;
        }
        h->ev_pool.push_back(p.a);
        h->ev_pool.push_back(p.b);
    }
    h->ev_used.clear();
}

// where k_export leaves a window's results in the pinned staging buffer
struct ExportLayout { size_t o_pose, o_pt, o_chi, o_out, end; };
ExportLayout export_layout(const DevWindow &w)
{
    ExportLayout L;
    L.o_pose = 0;
    L.o_pt = align_up(sizeof(double) * 7 * (size_t)w.NP, 256);
    L.o_chi = L.o_pt + align_up(sizeof(double) * 3 * (size_t)w.P, 256);
    L.o_out = L.o_chi + align_up(sizeof(double) * (size_t)w.E, 256);
    L.end = L.o_out + align_up((size_t)w.E + 8, 256);
    return L;
}

ExportDst export_dst(char *stage_dev, const ExportLayout &L, bool poses, bool points, bool chi2)
{
    ExportDst dst;
    dst.poses = poses ? reinterpret_cast<unsigned long long *>(stage_dev + L.o_pose) : nullptr;
    dst.points = points ? reinterpret_cast<unsigned long long *>(stage_dev + L.o_pt) : nullptr;
    dst.chi2 = chi2 ? reinterpret_cast<unsigned long long *>(stage_dev + L.o_chi) : nullptr;
    dst.outlier = reinterpret_cast<unsigned long long *>(stage_dev + L.o_out);
    return dst;
}

}  // namespace

extern "C" {

int movba_version(void) { return MOVBA_VERSION; }

#ifdef MOVBA_TEST_HOOKS
// Test build only (libmovba_hooks.so; declared by the tests themselves, not by include/movba.h): sets one hook of a handle.
// "device_cus" plans the one-launch direct solver for a device with fewer compute units than this one has.
// "batch_variant" sets nothing: it returns TestHooks::batch_variant, the record of the last batched run, as a code >= 0.
int movba_test_hook(movba_handle *h, const char *name, long long value)
{
    if (!h || !name) return MOVBA_ERR_ARG;
    const std::string n(name);
    if (n == "batch_variant") return h->hooks.batch_variant;
    if (n == "host_structure") h->hooks.host_structure = (int)value;
    else if (n == "host_grouping") h->hooks.host_grouping = (int)value;
    else if (n == "entries_unpacked") h->hooks.entries_unpacked = (int)value;
    else if (n == "no_sorted_structure") h->hooks.no_sorted_structure = (int)value;
    else if (n == "pcg_packed") h->hooks.pcg_packed = (int)value;
    else if (n == "helper_delay_us") h->hooks.helper_delay_us = (int)value;
    else if (n == "wait_ticks") h->hooks.wait_ticks = value;
    else if (n == "band_park_trial") h->hooks.band_park_trial = (int)value;
    else if (n == "device_cus") { if (value > 0 && value < h->device_cus) h->device_cus = (int)value; }
    else return MOVBA_ERR_ARG;
    return MOVBA_OK;
}
#endif

const char *movba_status_string(int s)
{
    switch (s) {
    case MOVBA_OK: return "ok";
    case MOVBA_STOPPED: return "stopped before solve";
    case MOVBA_NO_FIXED: return "no fixed keyframe";
    case MOVBA_EMPTY: return "nothing to optimise";
    case MOVBA_SINGULAR: return "information matrix not positive definite (singular)";
    case MOVBA_ERR_ARG: return "invalid argument";
    case MOVBA_ERR_HIP: return "HIP runtime error";
    case MOVBA_ERR_STATE: return "invalid call order";
    case MOVBA_ERR_DEVICE_WAIT: return "direct solver: a workgroup gave up waiting for another";
    case MOVBA_ERR_TOO_LARGE: return "reduced system too large for the direct solver";
    default: return "unknown";
    }
}

int movba_create(movba_handle **out, int device, void *stream, const movba_options *opt)
{
    if (!out) return MOVBA_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        std::fprintf(stderr, "libmovba: no HIP device available — the local-BA path has no CPU fallback\n");
        return MOVBA_ERR_HIP;
    }
    if (device < 0 || device >= ndev) return MOVBA_ERR_ARG;
    movba_handle *h = new (std::nothrow) movba_handle();
    if (!h) return MOVBA_ERR_HIP;
    h->device = device;
    h->opt.pcg_rel_tol = 1e-10; h->opt.pcg_max_iters = 0; h->opt.run_ahead = 2; h->opt.profile = 0; h->opt.pcg_coarse = 1; h->opt.host_wait = 0; h->opt.pcg_spill = 0; h->opt.solver = 0; h->opt.reorder = 0;
    if (opt) {
        if (opt->pcg_rel_tol > 0) h->opt.pcg_rel_tol = opt->pcg_rel_tol;
        if (opt->pcg_max_iters > 0) h->opt.pcg_max_iters = opt->pcg_max_iters;
        if (opt->run_ahead > 0) h->opt.run_ahead = opt->run_ahead;
        h->opt.profile = opt->profile;
        if (opt->pcg_coarse < 0) h->opt.pcg_coarse = 0;
        h->opt.host_wait = opt->host_wait == 1 ? 1 : 0;
        h->opt.pcg_spill = opt->pcg_spill == 1 ? 1 : 0;
        h->opt.solver = (opt->solver >= 1 && opt->solver <= 3) ? opt->solver : 0;
        h->opt.reorder = opt->reorder == -1 ? -1 : 0;
    }
    if (h->opt.host_wait == 1) h->packer.spin_ms = 0;      // (a caller that asks for yielding waits does not want a spinning helper either)
    for (int k = 0; k < MOVBA_NKERNELS; ++k) h->prof.name[k] = kKernelNames[k];
    if (hipSetDevice(device) != hipSuccess) { delete h; return MOVBA_ERR_HIP; }
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->device_cus = cus; }
    if (stream) { h->stream = static_cast<hipStream_t>(stream); }
    else {
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { delete h; return MOVBA_ERR_HIP; }
        h->own_stream = true;
    }
    if ((h->copy_stream = shared_copy_stream(device)) == nullptr ||
        hipEventCreateWithFlags(&h->copy_event, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->edgeb_event, hipEventDisableTiming) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&h->ingest_counter), 256) != hipSuccess || hipMemset(h->ingest_counter, 0, 256) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&h->hstat), sizeof(HostStatus), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void **>(&h->hstat_dev), h->hstat, 0) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&h->ctrl_host), sizeof(Ctrl), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void **>(&h->ctrl_host_dev), h->ctrl_host, 0) != hipSuccess ||
        configure_kernels(0) != hipSuccess || configure_pcg_rows() != hipSuccess || configure_band() != hipSuccess || configure_struct_kernels() != hipSuccess ||
        configure_dense_kernels() != hipSuccess || configure_dense_persist() != hipSuccess ||
        configure_pose_kernels() != hipSuccess) {
        movba_destroy(h);
        return MOVBA_ERR_HIP;
    }
    std::memset((void *)h->hstat, 0, sizeof(HostStatus));
    *out = h;
    return MOVBA_OK;
}

void movba_destroy(movba_handle *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);        // shared: stays
    if (h->copy_event) (void)hipEventDestroy(h->copy_event);
    if (h->edgeb_event) (void)hipEventDestroy(h->edgeb_event);
    harvest_events(h);
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    for (hipStream_t st : h->batch_streams) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (hipEvent_t e : h->batch_ev) if (e) (void)hipEventDestroy(e);
    for (auto &ring : h->batch_phase_ev) for (hipEvent_t e : ring) if (e) (void)hipEventDestroy(e);
    for (void *dev : { (void *)h->ingest_counter, (void *)h->arena }) if (dev) (void)hipFree(dev);
    for (Scratch *b : { &h->scratch, &h->scratch2, &h->pose_scratch, &h->marg, &h->marg_host, &h->batch_dev, &h->batch_host }) b->release();
    STAMP_HOST(h->stamp.release());
    if (h->stage) (void)hipHostFree(h->stage);
    if (h->hstat) (void)hipHostFree((void *)h->hstat);
    if (h->ctrl_host) (void)hipHostFree(h->ctrl_host);
    {
        DenseGate &g = dense_gate(h->device);       // (queue_direct: the gate must not keep a stream that is about to go)
        std::lock_guard<std::mutex> lk(g.mu);
        if (g.only_stream == h->stream) g.only_stream = nullptr;       // (drained above: nothing of this stream is in flight)
    }
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int movba_structure_probe(const movba_lba_desc *desc, movba_structure_info *info, int32_t *edge_perm, int32_t *free_index)
{
    if (!desc || !info) return MOVBA_ERR_ARG;
    Structure s;
    const int rc = build_structure(*desc, s);
    if (rc < 0) return rc;
    if (s.nfree > MOVBA_MAX_FREE_KEYFRAMES) return MOVBA_ERR_TOO_LARGE;
    info->n_free = s.nfree; info->n_pairs = s.npairs; info->n_entries = s.nentries; info->n_items = s.nitems;
    info->max_degree = s.max_degree; info->already_grouped = s.already_grouped ? 1 : 0; info->reordered = s.reordered ? 1 : 0; info->pad_s = 0;
    info->pcg_on_chip = 0; info->pcg_overflow = 0; info->pcg_max_wave_entries = 0; info->n_row_entries = (int32_t)s.row_ent.size();
    if (rc == MOVBA_OK && s.nfree > 0) {
        PcgParams pp{};
        if (pcg_rows_supported(s.nfree, s.row_ptr.data(), &pp)) {
            info->pcg_on_chip = 1; info->pcg_overflow = pp.overflow;
            for (int wv = 0; wv < kPcgRowsThreads / 64; ++wv)
                info->pcg_max_wave_entries = std::max(info->pcg_max_wave_entries, s.row_ptr[pp.wave_row0[wv + 1]] - s.row_ptr[pp.wave_row0[wv]]);
        }
    }
    {   // launch schedule and pose-major slots: self-checks reported to the caller (CPU tests)
        info->n_sched_slots = (int32_t)s.sched.size(); info->sched_items = 0; info->sched_max_permille = 0; info->slots_ok = 1;
        // (every item once: the wave slots that share it lie side by side in ONE workgroup, their places 0 .. n - 1 in order, and
        //  their entry ranges cut the item's range without gap or overlap)
        std::vector<uint8_t> seen(s.nitems > 0 ? s.nitems : 1, 0);
        int64_t segw[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, tot = 0;
        for (size_t k = 0; k < s.sched.size(); ++k) {
            const SchedItem &it = s.sched[k];
            if (it.tag < 0 || (it.sub & 0xff) != 0) continue;
            const int item = it.tag >> 1, nw = it.sub >> 8;
            bool ok = item < s.nitems && !seen[item] && nw >= 1 && nw <= 4 && (k & 3) + (size_t)nw <= 4 && s.items[item].begin == it.begin;
            int32_t at = it.begin;
            for (int q = 0; ok && q < nw; ++q) {
                const SchedItem &w = s.sched[k + q];
                ok = w.tag == it.tag && w.sub == (q | (nw << 8)) && w.begin == at && w.end >= w.begin;
                at = w.end;
            }
            if (!ok || at != s.items[item].end) { info->sched_items = -1; break; }
            seen[item] = 1; info->sched_items++;
            const int64_t wgt = (int64_t)(s.items[item].end - s.items[item].begin) * ((it.tag & 1) ? 3 : 2) + 128;
            if (s.sched_per_xcd > 0) segw[k / s.sched_per_xcd] += wgt;
            tot += wgt;
        }
        if (tot > 0) { int64_t mx = 0; for (int64_t v : segw) mx = std::max(mx, v); info->sched_max_permille = (int32_t)(mx * 8000 / tot); }
        int64_t nfree_edges = 0;
        for (int32_t v : s.slot) nfree_edges += v >= 0;
        std::vector<uint8_t> hit((size_t)nfree_edges + 1, 0);
        for (int32_t v : s.slot) if (v >= 0) { if (v >= nfree_edges || hit[v]) { info->slots_ok = 0; break; } hit[v] = 1; }
    }
    if (edge_perm) {
        if (s.perm.empty()) for (int e = 0; e < s.E; ++e) edge_perm[e] = e;       // already grouped: identity
        else std::memcpy(edge_perm, s.perm.data(), sizeof(int32_t) * s.perm.size());
    }
    if (free_index) std::memcpy(free_index, s.hidx.data(), sizeof(int32_t) * s.hidx.size());
    return rc;
}

int movba_dense_plan_probe(int32_t n_block_cols, int32_t max_groups, int32_t max_slots, int32_t info[4], int32_t *task_ptr, int32_t task_ptr_cap,
                           int32_t *tasks, int32_t tasks_cap)
{
    if (!info || n_block_cols < 1) return MOVBA_ERR_ARG;
    DensePlan p;
    build_dense_plan(n_block_cols, p, max_groups > 0 ? max_groups : kDenseMaxGroups, max_slots > 0 ? max_slots : kDenseMaxSlots);
    info[0] = p.ok ? 1 : 0; info[1] = p.G; info[2] = p.slots; info[3] = (int32_t)p.tasks.size();
    if (p.ok && task_ptr) for (int g = 0; g <= p.G && g < task_ptr_cap; ++g) task_ptr[g] = p.task_ptr[g];
    if (p.ok && tasks) std::memcpy(tasks, p.tasks.data(), sizeof(DenseTask) * std::min<size_t>(p.tasks.size(), (size_t)std::max(tasks_cap, 0)));
    return MOVBA_OK;
}

}  // extern "C"

namespace {

// PCG parameters of the handle's resident window for a run
PcgParams run_pcg_params(const movba_handle *h)
{
    PcgParams pp = h->pp;
    pp.rel_tol = h->opt.pcg_rel_tol;
    // PCG cap: past ~200 iterations the direct solver is cheaper than carrying on, and a system that slow to converge is
    // one whose iterative answer would depart from the exact step anyway (see the park in k_pcg_rows)
    pp.max_iters = h->opt.pcg_max_iters > 0 ? h->opt.pcg_max_iters : 200;
    // 1: coarse level built beside the solve, one trial old; 2: small window (<= one keyframe per wave), built first and fresh
    bool one_row_per_wave = true;
    for (int wv = 0; wv < kPcgRowsThreads / 64; ++wv) one_row_per_wave &= pp.wave_row0[wv + 1] - pp.wave_row0[wv] <= 1;
    pp.use_coarse = (h->opt.pcg_coarse && h->rows_kernel) ? (one_row_per_wave ? 2 : 1) : 0;
    return pp;
}

// the direct solve of the current trial: one launch when the window's schedule fits (dense_persist.hip), else the launch per
// block column of dense_solve.hip.  The hand-off flags are zeroed once per uploaded window; every launch has its own epoch.
hipError_t queue_direct(movba_handle *h)
{
    const DevWindow &w = h->win;
    if (w.dense.G <= 0) return launch_dense_solve(w, h->stream);
    if (!h->dense_flags_clean) {
        const hipError_t e = hipMemsetAsync(w.dense.flags, 0, sizeof(uint32_t) * (size_t)dense_flag_words(w.dense.ntile), h->stream);
        if (e != hipSuccess) return e;
        h->dense_flags_clean = true; h->dense_epoch = 0;
    }
    hipError_t el;
    {
        DenseGate &g = dense_gate(h->device);
        std::lock_guard<std::mutex> lk(g.mu);
        if (!g.multi && g.only_stream && g.only_stream != h->stream) {
            // a second stream: what the first one has in flight is waited for once, on the host; the event chain takes over
            hipError_t e = hipStreamSynchronize(g.only_stream);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&g.ev, hipEventDisableTiming);
            if (e != hipSuccess) return e;
            g.multi = true; g.ev_recorded = false;
        }
        if (g.multi && g.ev_recorded) { const hipError_t e = hipStreamWaitEvent(h->stream, g.ev, 0); if (e != hipSuccess) return e; }
        el = launch_dense_persist(w, ++h->dense_epoch, h->stream);
        if (g.multi) { if (el == hipSuccess) { el = hipEventRecord(g.ev, h->stream); g.ev_recorded = el == hipSuccess; } }
        else g.only_stream = h->stream;
    }
    if (w.dense.stamps && el == hipSuccess && h->dense_epoch == 3) {
        // diagnostic (MOVBA_DENSE_STAMPS=1): the third direct launch of a window, task by task, in 10 ns ticks from the first start
        const size_t nt_ = h->dplan.tasks.size();
        std::vector<unsigned long long> st(6 * nt_);
        if (hipStreamSynchronize(h->stream) == hipSuccess && hipMemcpy(st.data(), w.dense.stamps, sizeof(unsigned long long) * 6 * nt_, hipMemcpyDeviceToHost) == hipSuccess) {
            unsigned long long t0 = ~0ull;
            for (size_t k = 0; k < nt_; ++k) if (st[6 * k] && st[6 * k] < t0) t0 = st[6 * k];
            static const char *names[] = { "ASM", "UPD", "DIAG", "OFF", "RHS", "BSX", "BSC", "EPI", "RUP", "UPD2", "COL" };
            for (int g = 0; g < h->dplan.G; ++g)
                for (int t = h->dplan.task_ptr[g]; t < h->dplan.task_ptr[g + 1]; ++t) {
                    const DenseTask &tk = h->dplan.tasks[t];
                    const unsigned long long *q = &st[6 * (size_t)t];
                    std::fprintf(stderr, "libmovba[dense]: wg %3d %-4s (%2d,%2d) k=%2d  start %7.2f us  wait %6.2f  work %6.2f", g, names[tk.op], tk.I, tk.K, tk.k,
                                 0.01 * (double)(q[0] - t0), q[1] ? 0.01 * (double)(q[1] - q[0]) : 0.0, 0.01 * (double)(q[5] - (q[1] ? q[1] : q[0])));
                    if (q[2] && q[3]) std::fprintf(stderr, "   [fetch %5.2f  sweep %5.2f  publish %5.2f]", 0.01 * (double)(q[2] - q[1]), 0.01 * (double)(q[3] - q[2]), 0.01 * (double)(q[5] - q[3]));
                    std::fprintf(stderr, "\n");
                }
        }
    }
    return el;
}

// k_band's second argument: the half bandwidth, and in the test build the trial whose factorisation is to park (+ 1, from bit 16)
inline int band_arg(const movba_handle *h) { return h->band_bw | ((HOOK(h, band_park_trial) + 1) << 16); }

// The LM trial loop of the handle's window on its own stream, from the state the device is in: a fresh window (after the
// setup launches), or one that parked itself during a batched run (its pause is then the first thing answered).
int lm_loop(movba_handle *h, bool parked)
{
    const DevWindow &w = h->win;
    hipStream_t s = h->stream;
    PcgParams pp = run_pcg_params(h);
    const int nrowent = (int)h->st.row_ent.size();
    // the reduced solve of a trial: on-chip PCG, or (larger windows, and from the first PCG failure on) the direct solver
    const bool band = h->band;                      // (an exact solve in one launch; it parks the solve only when a pivot comes out non-positive)
    bool direct = !h->rows_kernel && !band;
    int pauses_seen = 0;
    if (!parked) __atomic_store_n(&h->hstat->pause_seq, 0, __ATOMIC_RELAXED);
    const int max_trials = (w.max_iters > 0 ? w.max_iters : 0) * w.max_trials;
    double t_progress = now_ms();                   // last time the device's progress word changed or work was queued
    uint64_t last_pg = ~0ull;
    // k_finalize + the Ctrl read-back are queued speculatively behind a trial that is likely the last one, so that the
    // end of the solve does not wait for a host round trip; a later trial simply queues them again
    int t = 0, final_after = -1;
    auto queue_finalize = [&]() -> int {
        { ScopedEvents ev(h, KC_FINALIZE); HIP_TRY(launch_finalize(w, s)); }        // (also writes Ctrl to h->ctrl_host)
        // ... and the results go across the bus into the staging buffer right behind it: movba_lba_download then finds them
        // there instead of paying a launch and a stream synchronise of its own
        if (h->export_in_run) {
            ExportDst dst = export_dst(h->stage_dev, export_layout(w), h->exported[0], h->exported[1], h->exported[2]);
            if (h->user_dst[0]) dst.poses = h->user_dst[0];
            if (h->user_dst[1]) dst.points = h->user_dst[1];
            if (h->user_dst[2]) dst.chi2 = h->user_dst[2];
            HIP_TRY(launch_export(w, dst, s));
        }
        final_after = t;
        return MOVBA_OK;
    };
    auto queue_solve = [&]() -> int {
        if (band && !direct) { ScopedEvents ev(h, KC_PCG); HIP_TRY(launch_band(w, band_arg(h), s)); }      // (direct: the factorisation parked the solve)
        else if (direct) { ScopedEvents ev(h, KC_PCG); HIP_TRY(queue_direct(h)); }
        else { ScopedEvents ev(h, KC_PCG); HIP_TRY(launch_pcg_rows(w, nrowent, pp, t, s)); }
        return MOVBA_OK;
    };
    auto queue_tail = [&]() -> int {
        // (the pass's extra workgroup takes the LM decision: no launch of its own)
        { ScopedEvents ev(h, KC_BACKSUB); HIP_TRY(launch_backsub(w, s)); }
        return MOVBA_OK;
    };
    // The device parked the solve (k_pcg_rows gave up on trial `td`): every trial set queued behind has turned into no-ops.
    // Queue the direct solver for that trial (its schur partials are still in place) and carry on in direct mode.
    auto answer_pause = [&]() -> int {
        pauses_seen = rd_pause(h->hstat);
        direct = true;
        t = (int)(rd_progress(h->hstat) & 0xffffff);
        int rq = queue_solve(); if (rq != MOVBA_OK) return rq;
        rq = queue_tail(); if (rq != MOVBA_OK) return rq;
        ++t;
        final_after = -1;
        return MOVBA_OK;
    };
    for (;;) {
        for (; t < max_trials; ++t) {
            // stay at most run_ahead trial sets ahead of the device, and never further than the outer iterations that are
            // left: with R iterations to go at most R more trials run unless one is rejected, so the sets queued beyond that
            // would almost always be no-op launches (~5 us each) at the end of the solve
            // (k_decide publishes trials_done, it and done as one word)
            bool finished = false, paused = false;
            for (;;) {
                const uint64_t pg = rd_progress(h->hstat);
                if (pg != last_pg) { last_pg = pg; t_progress = now_ms(); }
                const int td = (int)(pg & 0xffffff), it_done = (int)((pg >> 24) & 0xffffff);
                if ((pg >> 48) & 1) { finished = true; break; }
                if (rd_pause(h->hstat) != pauses_seen) { paused = true; break; }
                const int left = w.max_iters - it_done;
                const int limit = left < h->opt.run_ahead ? (left > 1 ? left : 1) : h->opt.run_ahead;
                if (t - td < limit) break;
                if (final_after != t && t - td < h->opt.run_ahead) { const int rq = queue_finalize(); if (rq != MOVBA_OK) return rq; }
                if (caller_stop(h->stop)) wr_stop(h->hstat, 1);
                if (now_ms() - t_progress > watchdog_ms()) {
                    // raise the device-side stop flag on the way out: whatever is still queued on the stream turns into
                    // no-op launches as soon as a k_decide sees it, and the window has to be uploaded again
                    std::fprintf(stderr, "libmovba: device made no progress for %.0f ms, giving up\n", watchdog_ms());
                    wr_stop(h->hstat, 1); h->uploaded = false;
                    (void)hipStreamSynchronize(s);          // nothing of this solve is left queued when the caller gets the error
                    return MOVBA_ERR_HIP;
                }
                host_relax(h->opt.host_wait);
            }
            if (finished) break;
            if (paused) { const int rq = answer_pause(); if (rq != MOVBA_OK) return rq; --t; continue; }
            if (caller_stop(h->stop)) wr_stop(h->hstat, 1);
            t_progress = now_ms();                          // (new work queued counts as progress)
            if (w.nitems > 0) { ScopedEvents ev(h, KC_SCHUR); HIP_TRY(launch_schur(w, 0, s)); }
            { const int rq = queue_solve(); if (rq != MOVBA_OK) return rq; }
            { const int rq = queue_tail(); if (rq != MOVBA_OK) return rq; }
        }
        if (final_after != t) { const int rq = queue_finalize(); if (rq != MOVBA_OK) return rq; }
        HIP_TRY(hipStreamSynchronize(s));
        // a park that happened behind the last queued set is only seen now
        if (rd_pause(h->hstat) == pauses_seen) break;
        const int rq = answer_pause(); if (rq != MOVBA_OK) return rq;
    }
    harvest_events(h);
    return MOVBA_OK;
}

}  // namespace

extern "C" {

int movba_lba_run(movba_handle *h)
{
    if (!h) return MOVBA_ERR_ARG;
    if (!h->uploaded) return MOVBA_ERR_STATE;
    HIP_TRY(hipSetDevice(h->device));
    h->ran = false; h->run_status = MOVBA_OK;
    if (h->early_status != MOVBA_OK) { h->ran = true; return h->early_status; }
    // early return before the solve (src/Optimizer.cc:749-751); not sticky: the next run looks at the flag again
    if (caller_stop(h->stop)) { h->run_status = MOVBA_STOPPED; h->ran = true; return MOVBA_STOPPED; }
    // (a registered export buffer too small for this window is ignored rather than overrun)
    h->win.pose_export = (h->pose_export && h->pose_export_cap >= (int64_t)sizeof(double) * 7 * h->win.NP) ? h->pose_export : nullptr;
    const DevWindow &w = h->win;
    hipStream_t s = h->stream;
    // (the staging buffer is free once the upload's copies, queued ahead of every kernel of the run, have left it; it is as
    // large as the upload needed, which is more than the results take)
    h->export_in_run = h->export_hint && export_layout(w).end <= h->stage_cap;
    if (!h->export_in_run) for (int k = 0; k < 3; ++k) { h->user_dst[k] = nullptr; h->user_host[k] = nullptr; }
    STAMP_HOST(const int rs = stamp_window(h); if (rs) return rs);     // (a run's report lines are its own: zeroed here as at the upload)

    // One kernel waits for other workgroups INSIDE a launch: the one-launch direct solver (dense_persist.hip).  Its waits are
    // bounded (DevWindow::wait_ticks, 20 ms) and cannot deadlock on an otherwise idle device, but its workgroups are not
    // GUARANTEED their residency either: another process on the GPU, a CU-masked or partitioned device, any other kernel
    // holding the CUs.  A solve in which a wait was given up (Ctrl::n_sync_timeouts) is therefore run AGAIN from the uploaded
    // state on the path that waits for nothing - the direct solver one launch per block column (dense_solve.hip) - instead
    // of handing the caller an error: the reference never skips a solve for such a reason (src/Optimizer.cc:535).
    // movba_lba_result::n_sync_timeouts reports that it happened.  (The deciding wave of the back-substitution pass waits
    // too, for producers that wait for nothing themselves: that wait has the host watchdog's bound, kernels.hip.)
    h->sync_retries = 0;
    // per-attempt values of the window descriptor, put back on every way out of the loop (an error return included)
    struct Restore {
        DevWindow &w; const int32_t G; const unsigned long long ticks;
        ~Restore() { w.dense.G = G; w.wait_ticks = ticks; }
    } restore{ h->win, h->win.dense.G, h->win.wait_ticks };
    for (int attempt = 0;; ++attempt) {
        const bool careful = attempt > 0;
        h->win.wait_ticks = (!careful && HOOK(h, wait_ticks) >= 0) ? (unsigned long long)HOOK(h, wait_ticks) : restore.ticks;
        h->win.dense.G = careful ? 0 : restore.G;
        __atomic_store_n(&h->hstat->progress, (uint64_t)0, __ATOMIC_RELAXED); wr_stop(h->hstat, 0);
        {   // state 0 from the uploaded estimates, first linearisation, lambda_0 and F0
            ScopedEvents ev(h, KC_SETUP);
            if (!h->early_setup) {          // (else: queued by the upload already, behind the edge data)
                HIP_TRY(launch_init(w, s));
                HIP_TRY(launch_linearize(w, s));
            }
            h->early_setup = false;
            if (w.nitems > 0) HIP_TRY(launch_schur(w, 1, s));
            HIP_TRY(launch_lambda_init(w, s));
        }
        const int rl = lm_loop(h, false);
        if (rl != MOVBA_OK) return rl;
        if (h->ctrl_host->n_sync_timeouts > 0 && !careful) {
            std::fprintf(stderr, "libmovba: a workgroup gave up waiting for another in %d launch(es) of this solve: running it again, the direct solver launch by launch\n",
                         h->ctrl_host->n_sync_timeouts);
            h->sync_retries = h->ctrl_host->n_sync_timeouts;
            h->dense_flags_clean = false;           // (hand-off flags of the abandoned launches: zeroed again before the next one-launch solve)
            continue;
        }
        break;
    }
    STAMP_HOST(stamp_report_run(h));
    h->ran = true;
    return MOVBA_OK;
}

// Optimizer::LocalBundleAdjustment's solve on n resident windows at once (multi-session serving; BASELINE cfg5's windows when
// they share a GPU): every kernel of a trial is ONE launch over the concatenated windows — the point and schur grids of a
// single 50-keyframe window leave most of the chip idle, and its PCG occupies 2 of 256 CUs — with per-window LM state, so
// each window takes exactly the steps (and produces exactly the bits) of its solo movba_lba_run.
int movba_lba_run_batch(movba_handle *const *hs, int32_t n)
{
    if (!hs || n < 1) return MOVBA_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        if (!hs[i]) return MOVBA_ERR_ARG;
        if (!hs[i]->uploaded) return MOVBA_ERR_STATE;
        if (hs[i]->device != hs[0]->device || hs[i]->stream != hs[0]->stream) {
            std::fprintf(stderr, "libmovba: the handles of a batch must share one device and one stream\n");
            return MOVBA_ERR_ARG;
        }
        for (int k = 0; k < i; ++k) if (hs[k] == hs[i]) return MOVBA_ERR_ARG;
    }
    movba_handle *h0 = hs[0];
    HIP_TRY(hipSetDevice(h0->device));
    hipStream_t s = h0->stream;
    // windows that return before the solve (nothing to do, no fixed keyframe, stop flag up) and windows without an on-chip
    // PCG (they take the direct solver's per-window launches) stay out of the batched launches
    std::vector<movba_handle *> act, solo;
    for (int i = 0; i < n; ++i) {
        movba_handle *h = hs[i];
        h->ran = false; h->run_status = MOVBA_OK; h->export_in_run = false; h->early_setup = false;      // (the batch queues every window's setup itself)
#ifdef MOVBA_TEST_HOOKS
        h->hooks.batch_variant = 0;
#endif
        if (h->early_status != MOVBA_OK) { h->ran = true; continue; }
        if (caller_stop(h->stop)) { h->run_status = MOVBA_STOPPED; h->ran = true; continue; }
        if (!h->rows_kernel || h->win.kcam) {       // (direct-solver windows and windows with intrinsics by keyframe run on their own)
#ifdef MOVBA_TEST_HOOKS
            h->hooks.batch_variant = 1 << 9;
#endif
            solo.push_back(h);
            continue;
        }
        act.push_back(h);
    }
    const int na = (int)act.size();
    if (na > 0) {
        bool stereo = act[0]->win.stereo != 0, ldsp = true, overflow = false, padded = true;
        for (movba_handle *h : act) {
            if ((h->win.stereo != 0) != stereo) {
                std::fprintf(stderr, "libmovba: a batch holds either stereo or monocular windows, not both\n");
                return MOVBA_ERR_ARG;
            }
            ldsp &= h->win.lds_poses != 0; overflow |= h->pp.overflow != 0; padded &= h->pp.padded != 0 && !h->pp.overflow;
        }
        // Groups of windows on streams of their own, out of phase: a group's PCG launch keeps 2 CUs per window busy for most
        // of a trial while its point / schur launches fill the chip for the rest, so the PCG of one group runs beside the
        // streaming kernels of the others.  Each window's own kernels still run in its solo order on one stream.
        // (two by default: with more streams than hardware queues left to the process the groups fall back into lockstep)
        int ngroups = na >= 2 ? 2 : 1;
        if (process_switches().batch_groups > 0) ngroups = std::max(1, std::min(std::min(kMaxGroups, na), process_switches().batch_groups));
        if (ngroups > 1 && !h0->batch_ev[0]) {
            for (hipEvent_t &e : h0->batch_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            for (auto &ring : h0->batch_phase_ev) for (hipEvent_t &e : ring) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
#ifdef MOVBA_TEST_HOOKS
        {   // (test build: the template arguments of this call's launches, on every handle of the call that reached this point)
            const int fold = (ldsp ? 1 : 0) | (overflow ? 2 : 0) | (padded && !overflow ? 4 : 0) | (stereo ? 8 : 0) | (ngroups << 4);
            for (movba_handle *h : act) h->hooks.batch_variant = fold | (1 << 8);
            for (movba_handle *h : solo) h->hooks.batch_variant |= fold;
        }
#endif
        // the second group runs on the device's shared copy stream (idle during a run): every stream the process creates
        // competes for the few hardware queues, and two groups that land on one queue run in turns (measured: 2.3 -> 3.7 ms)
        for (int g = 2; g < ngroups; ++g)
            if (!h0->batch_streams[g]) HIP_TRY(hipStreamCreateWithFlags(&h0->batch_streams[g], hipStreamNonBlocking));
        struct Group {
            std::vector<movba_handle *> hs;
            hipStream_t s = nullptr;
            BatchDev b{};
            int nb_point = 0, nb_schur = 0, nb_final = 0, nb_init = 0, max_trials = 0, max_iters = 0;
            size_t lds_lin = 0, lds_back = 0, lds_pcg = 0, lds_band = 0;
            bool any_band = false, any_pcg = false;     // windows solved by k_band_b / by k_pcg_rows_b (each window as in its solo run)
            int t = 0, final_after = -1;
            bool finished = false;
        } grp[kMaxGroups];
        for (int i = 0; i < na; ++i) grp[(int)((int64_t)i * ngroups / na)].hs.push_back(act[i]);
        grp[0].s = s;
        for (int g = 1; g < ngroups; ++g) grp[g].s = g == 1 ? h0->copy_stream : h0->batch_streams[g];
        // ---- device views, PCG plans and block prefixes of both groups in one buffer ----
        Carver c;
        size_t o_win[kMaxGroups], o_pp[kMaxGroups], o_bp[kMaxGroups], o_bs[kMaxGroups], o_bf[kMaxGroups], o_bi[kMaxGroups], o_bw[kMaxGroups];
        for (int g = 0; g < ngroups; ++g) {
            const size_t m = grp[g].hs.size();
            o_win[g] = c.take<DevWindow>(m); o_pp[g] = c.take<PcgParams>(m);
            o_bp[g] = c.take<int32_t>(m + 1); o_bs[g] = c.take<int32_t>(m + 1); o_bf[g] = c.take<int32_t>(m + 1); o_bi[g] = c.take<int32_t>(m + 1);
            o_bw[g] = c.take<int32_t>(m + 1);
        }
        { int rc = h0->batch_host.grow(h0, c.off); if (rc == MOVBA_OK) rc = h0->batch_dev.grow(h0, c.off); if (rc) return rc; }
        HIP_TRY(hipStreamSynchronize(s));           // the previous batch's H2D copy of this buffer has landed
        char *bh = h0->batch_host.p, *bd = h0->batch_dev.p;
        const int run_ahead = h0->opt.run_ahead;
        for (int g = 0; g < ngroups; ++g) {
            Group &G = grp[g];
            const int m = (int)G.hs.size();
            DevWindow *wins = reinterpret_cast<DevWindow *>(bh + o_win[g]);
            PcgParams *pps = reinterpret_cast<PcgParams *>(bh + o_pp[g]);
            int32_t *bp = reinterpret_cast<int32_t *>(bh + o_bp[g]), *bs = reinterpret_cast<int32_t *>(bh + o_bs[g]);
            int32_t *bf = reinterpret_cast<int32_t *>(bh + o_bf[g]), *bi = reinterpret_cast<int32_t *>(bh + o_bi[g]);
            int32_t *bwv = reinterpret_cast<int32_t *>(bh + o_bw[g]);
            bp[0] = bs[0] = bf[0] = bi[0] = 0;
            for (int i = 0; i < m; ++i) {
                movba_handle *h = G.hs[i];
                h->win.pose_export = (h->pose_export && h->pose_export_cap >= (int64_t)sizeof(double) * 7 * h->win.NP) ? h->pose_export : nullptr;
                __atomic_store_n(&h->hstat->progress, (uint64_t)0, __ATOMIC_RELAXED); wr_stop(h->hstat, 0); __atomic_store_n(&h->hstat->pause_seq, 0, __ATOMIC_RELAXED);
                STAMP_HOST(const int rs = stamp_window(h); if (rs) return rs);     // (on the callers' stream, ahead of every group's launches)
                wins[i] = h->win; wins[i].lds_poses = ldsp ? 1 : 0;
                pps[i] = run_pcg_params(h);
                bwv[i] = h->band ? band_arg(h) : -1;
                if (h->band) { G.any_band = true; G.lds_band = std::max(G.lds_band, band_lds_bytes(h->win.nfree, h->band_bw)); } else G.any_pcg = true;
                const DevWindow &w = h->win;
                bp[i + 1] = bp[i] + w.n_pt_blocks + 1;          // (+ the deciding workgroup of the window's back-substitution pass)
                bs[i + 1] = bs[i] + (w.nitems > 0 ? schur_blocks(w) : 0);
                bf[i + 1] = bf[i] + (w.E + 255) / 256;
                const int work = w.NP > (3 * w.P) / 2 ? w.NP : (3 * w.P) / 2;
                int nb = (work + 255) / 256; nb = nb < 1 ? 1 : (nb > 1024 ? 1024 : nb);
                bi[i + 1] = bi[i] + nb;
                G.lds_lin = std::max(G.lds_lin, point_lds_bytes_for(w, false, ldsp)); G.lds_back = std::max(G.lds_back, point_lds_bytes_for(w, true, ldsp));
                G.lds_pcg = std::max(G.lds_pcg, pcg_rows_lds_bytes(w.nfree, (int)h->st.row_ent.size(), padded && !overflow));
                G.max_trials = std::max(G.max_trials, (w.max_iters > 0 ? w.max_iters : 0) * w.max_trials);
                G.max_iters = std::max(G.max_iters, w.max_iters);
            }
            G.nb_point = bp[m]; G.nb_schur = bs[m]; G.nb_final = bf[m]; G.nb_init = bi[m];
            G.b.wins = reinterpret_cast<const DevWindow *>(bd + o_win[g]); G.b.pps = reinterpret_cast<const PcgParams *>(bd + o_pp[g]);
            G.b.blk_point = reinterpret_cast<const int32_t *>(bd + o_bp[g]); G.b.blk_schur = reinterpret_cast<const int32_t *>(bd + o_bs[g]);
            G.b.blk_final = reinterpret_cast<const int32_t *>(bd + o_bf[g]); G.b.blk_init = reinterpret_cast<const int32_t *>(bd + o_bi[g]);
            G.b.band_bw = reinterpret_cast<const int32_t *>(bd + o_bw[g]);
            G.b.n = m;
        }
        HIP_TRY(hipMemcpyAsync(bd, bh, c.off, hipMemcpyHostToDevice, s));
        if (ngroups > 1) {                          // the other streams start behind the uploads and this copy
            HIP_TRY(hipEventRecord(h0->batch_ev[0], s));
            for (int g = 1; g < ngroups; ++g) HIP_TRY(hipStreamWaitEvent(grp[g].s, h0->batch_ev[0], 0));
        }
        // ---- setup: state 0, first linearisation, lambda_0 and F0 of every window ----
        for (int g = 0; g < ngroups; ++g) {
            Group &G = grp[g];
            HIP_TRY(launch_init_batch(G.b, G.nb_init, G.s));
            HIP_TRY(launch_point_batch(G.b, G.nb_point, false, stereo, ldsp, G.lds_lin, G.s));
            if (G.nb_schur > 0) HIP_TRY(launch_schur_batch(G.b, G.nb_schur, 1, stereo, G.s));
            HIP_TRY(launch_lambda_init_batch(G.b, G.s));
        }
        // ---- trial sets: each group a bounded number of sets ahead of its slowest window still running ----
        double t_progress = now_ms();               // last time some window's progress word changed or work was queued
        uint64_t last_sum = ~0ull;
        for (;;) {
            bool all_finished = true;
            uint64_t pg_sum = 0;
            for (int g = 0; g < ngroups; ++g) {
                Group &G = grp[g];
                if (G.finished) continue;
                int td_min = 1 << 30, it_min = 1 << 30, running = 0;
                for (movba_handle *h : G.hs) {
                    const uint64_t pg = rd_progress(h->hstat);
                    pg_sum += pg;
                    if (((pg >> 48) & 1) || rd_pause(h->hstat) != 0) continue;      // done, or parked for the direct solver
                    ++running;
                    td_min = std::min(td_min, (int)(pg & 0xffffff)); it_min = std::min(it_min, (int)((pg >> 24) & 0xffffff));
                    if (caller_stop(h->stop)) wr_stop(h->hstat, 1);
                }
                if (running == 0 || G.t >= G.max_trials) {
                    if (G.final_after != G.t) { HIP_TRY(launch_finalize_batch(G.b, G.nb_final, G.s)); G.final_after = G.t; }
                    G.finished = true;
                    continue;
                }
                all_finished = false;
                const int left = G.max_iters - it_min;
                const int limit = left < run_ahead ? (left > 1 ? left : 1) : run_ahead;
                if (G.t - td_min >= limit) {
                    if (G.final_after != G.t && G.t - td_min < run_ahead) { HIP_TRY(launch_finalize_batch(G.b, G.nb_final, G.s)); G.final_after = G.t; }
                    continue;
                }
                // keep the groups out of phase: group g's schur launch of trial t starts when group g-1's has ended (otherwise
                // the streams drift into lockstep, all in their PCG at once with the chip idle: rocprofv3 trace); group g-1's
                // launch of that trial must therefore be queued first
                if (g > 0 && !grp[g - 1].finished && grp[g - 1].t <= G.t) continue;
                if (g > 0 && grp[g - 1].t > G.t) HIP_TRY(hipStreamWaitEvent(G.s, h0->batch_phase_ev[g - 1][G.t % kPhaseEvents], 0));
                if (G.nb_schur > 0) HIP_TRY(launch_schur_batch(G.b, G.nb_schur, 0, stereo, G.s));
                if (g + 1 < ngroups) HIP_TRY(hipEventRecord(h0->batch_phase_ev[g][G.t % kPhaseEvents], G.s));
                if (G.any_pcg) HIP_TRY(launch_pcg_rows_batch(G.b, overflow, padded && !overflow, G.lds_pcg, G.t, G.s));
                if (G.any_band) HIP_TRY(launch_band_batch(G.b, G.lds_band, G.s));
                HIP_TRY(launch_point_batch(G.b, G.nb_point, true, stereo, ldsp, G.lds_back, G.s));
                G.t += 1;
                t_progress = now_ms();
            }
            if (all_finished) break;
            if (pg_sum != last_sum) { last_sum = pg_sum; t_progress = now_ms(); }
            if (now_ms() - t_progress > watchdog_ms()) {
                std::fprintf(stderr, "libmovba: device made no progress for %.0f ms, giving up\n", watchdog_ms());
                for (movba_handle *h : act) { wr_stop(h->hstat, 1); h->uploaded = false; }
                for (int g = 0; g < ngroups; ++g) (void)hipStreamSynchronize(grp[g].s);
                return MOVBA_ERR_HIP;
            }
            host_relax(h0->opt.host_wait);
        }
        for (int g = 1; g < ngroups; ++g) {         // the callers' stream ends behind the others
            HIP_TRY(hipEventRecord(h0->batch_ev[g], grp[g].s));
            HIP_TRY(hipStreamWaitEvent(s, h0->batch_ev[g], 0));
        }
        HIP_TRY(hipStreamSynchronize(s));           // (every group was finalised behind its last trial set, in stream order)
        // windows whose PCG gave up parked themselves: each finishes on the direct solver from where it stands
        for (movba_handle *h : act) {
            if (rd_pause(h->hstat) != 0 && !((rd_progress(h->hstat) >> 48) & 1)) {
                const int rl = lm_loop(h, true);
                if (rl != MOVBA_OK) return rl;
            }
            h->ran = true;
        }
    }
    for (movba_handle *h : solo) { const int rc = movba_lba_run(h); if (rc < 0) return rc; }
    return MOVBA_OK;
}

int movba_lba_download(movba_handle *h, movba_lba_result *res)
{
    if (!h || !res) return MOVBA_ERR_ARG;
    if (!h->uploaded || !h->ran) return MOVBA_ERR_STATE;
    HIP_TRY(hipSetDevice(h->device));
    const int pre = h->early_status != MOVBA_OK ? h->early_status : h->run_status;
    res->status = pre;
    res->iters_done = 0; res->n_solves = 0; res->n_outliers = 0; res->pcg_iters = 0; res->last_rejected = 0;
    res->lambda = 0; res->cost0 = 0; res->cost = 0; res->n_trace = 0;
    res->n_direct = 0; res->direct_from = -1; res->n_chol_fail = 0; res->n_pcg_giveups = 0; res->n_sync_timeouts = 0; res->n_band = 0;
    if (pre != MOVBA_OK) return pre;
    const double t0 = now_ms();
    const DevWindow &w = h->win;
    const Ctrl &c = *h->ctrl_host;
    const size_t nb_pose = sizeof(double) * 7 * (size_t)w.NP, nb_pt = sizeof(double) * 3 * (size_t)w.P, nb_chi = sizeof(double) * (size_t)w.E;
    char *sg = h->stage;
    const ExportLayout L = export_layout(w);
    const size_t o_pose = L.o_pose, o_pt = L.o_pt, o_chi = L.o_chi, o_out = L.o_out;
    // results a movba_lba_solve exported straight into the caller's own (movba_host_alloc) arrays are not in the staging
    // buffer: a download into other arrays exports again
    if (h->export_in_run) {
        void *const arr[3] = { res->poses, res->points, res->chi2 };
        for (int k = 0; k < 3; ++k) if (arr[k] && (!h->exported[k] || (h->user_host[k] && h->user_host[k] != arr[k]))) h->export_in_run = false;
    }
    if (!h->export_in_run) {
        for (int k = 0; k < 3; ++k) h->user_host[k] = nullptr;
        int rs = ensure_stage(h, L.end); if (rs) return rs;
        sg = h->stage;
        HIP_TRY(launch_export(w, export_dst(h->stage_dev, L, res->poses != nullptr, res->points != nullptr, res->chi2 != nullptr), h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    // out of the pinned buffer into the caller's arrays (handing half of it to the helper thread saved 20 us when the
    // thread was awake and cost 0.4 ms when it had to be woken: not worth it for a copy the caller waits on)
    // (arrays in movba_host_alloc memory were written by the export kernel itself)
    const bool in_place = h->export_in_run;
    if (res->chi2 && !(in_place && h->user_host[2] == res->chi2)) std::memcpy(res->chi2, sg + o_chi, nb_chi);
    if (res->poses && !(in_place && h->user_host[0] == res->poses)) std::memcpy(res->poses, sg + o_pose, nb_pose);
    if (res->points && !(in_place && h->user_host[1] == res->points)) std::memcpy(res->points, sg + o_pt, nb_pt);
    if (res->outlier) std::memcpy(res->outlier, sg + o_out, (size_t)w.E);
    int n_out = 0;
    {
        // (flags are 0 / 1 bytes: eight at a time, summed by one multiplication)
        const uint8_t *of = reinterpret_cast<const uint8_t *>(sg + o_out);
        uint64_t acc = 0;
        int e = 0;
        for (; e + 8 <= w.E; e += 8) { uint64_t v; std::memcpy(&v, of + e, 8); acc += (v * 0x0101010101010101ull) >> 56; }
        for (; e < w.E; ++e) acc += of[e] != 0;
        n_out = (int)acc;
    }
    res->iters_done = c.iters_done; res->n_solves = c.n_solves; res->n_outliers = n_out;
    res->pcg_iters = c.pcg_total_iters; res->last_rejected = c.last_rejected;
    res->n_direct = c.n_direct; res->direct_from = c.direct_from; res->n_chol_fail = c.n_chol_fail; res->n_pcg_giveups = c.n_pause;
    res->n_band = c.n_band;
    res->lambda = c.lambda; res->cost0 = c.cost0; res->cost = c.F0;
    res->n_trace = c.n_trace;
    for (int k = 0; k < c.n_trace && k < MOVBA_MAX_TRACE; ++k) {
        res->tr_lambda[k] = c.tr_lambda[k]; res->tr_f0[k] = c.tr_f0[k]; res->tr_f1[k] = c.tr_f1[k];
        res->tr_rho[k] = c.tr_rho[k]; res->tr_accept[k] = c.tr_accept[k]; res->tr_pcg_iters[k] = c.tr_pcg[k];
    }
    res->n_sync_timeouts = c.n_sync_timeouts + h->sync_retries;
    h->prof.download_ms += now_ms() - t0;
    if (c.n_sync_timeouts > 0) {        // (only a batched run, which has no second attempt, or a second attempt that met a wait of the decide wave)
        // (the trials concerned were rejected like failed factorisations, so the state is a valid LM state — but not the one the
        //  reference's exact solver would have reached: never handed out as a success)
        std::fprintf(stderr, "libmovba: the one-launch direct solver gave up waiting between workgroups in %d solve(s): results discarded\n", c.n_sync_timeouts);
        res->status = MOVBA_ERR_DEVICE_WAIT;
        return MOVBA_ERR_DEVICE_WAIT;
    }
    return MOVBA_OK;
}

int movba_lba_solve(movba_handle *h, const movba_lba_desc *desc, movba_lba_result *res)
{
    if (!h || !desc || !res) return MOVBA_ERR_ARG;
    res->status = MOVBA_ERR_ARG;
    const bool lap_on = process_switches().time_solve;
    const double t_s0 = lap_on ? now_ms() : 0.0;
    int rc = movba_lba_upload(h, desc);
    const double t_s1 = lap_on ? now_ms() : 0.0;
    if (rc != MOVBA_OK) { res->status = rc; return rc; }
    h->export_hint = true;
    {
        const DevWindow &w = h->win;
        void *const arr[3] = { res->poses, res->points, res->chi2 };
        const size_t nb[3] = { sizeof(double) * 7 * (size_t)w.NP, sizeof(double) * 3 * (size_t)w.P, sizeof(double) * (size_t)w.E };
        for (int k = 0; k < 3; ++k) {
            h->user_dst[k] = host_block_view(arr[k], nb[k]); h->user_host[k] = h->user_dst[k] ? arr[k] : nullptr;
            h->exported[k] = arr[k] != nullptr;          // (an array the caller does not ask for does not cross the bus)
        }
    }
    rc = movba_lba_run(h);
    h->export_hint = false;
    for (int k = 0; k < 3; ++k) h->user_dst[k] = nullptr;      // (user_host stays for the download below)
    if (rc < 0) { res->status = rc; h->stop = nullptr; return rc; }
    const double t_s2 = lap_on ? now_ms() : 0.0;
    rc = movba_lba_download(h, res);
    if (lap_on) std::fprintf(stderr, "libmovba[solve]: upload %.3f  run %.3f  download %.3f ms\n", t_s1 - t_s0, t_s2 - t_s1, now_ms() - t_s2);
    h->stop = nullptr;      // keep no caller pointer after the call returns
    res->status = rc;
    return rc;
}

int movba_lba_export_poses_device(movba_handle *h, void *dst, int64_t cap)
{
    if (!h || !dst) return MOVBA_ERR_ARG;
    if (!h->uploaded || !h->ran || h->early_status != MOVBA_OK || h->run_status != MOVBA_OK) return MOVBA_ERR_STATE;
    const DevWindow &w = h->win;
    const size_t nb = sizeof(double) * 7 * (size_t)w.NP;
    if (cap < (int64_t)nb) return MOVBA_ERR_ARG;
    HIP_TRY(hipMemcpyAsync(dst, w.st[h->ctrl_host->cur].pose, nb, hipMemcpyDeviceToDevice, h->stream));
    return MOVBA_OK;
}

int movba_lba_set_pose_export(movba_handle *h, void *dst, int64_t cap)
{
    if (!h || (dst && cap <= 0)) return MOVBA_ERR_ARG;
    h->pose_export = static_cast<double *>(dst);
    h->pose_export_cap = dst ? cap : 0;
    return MOVBA_OK;
}

void *movba_host_alloc(size_t bytes)
{
    if (bytes == 0) return nullptr;
    void *p = nullptr, *d = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(p); return nullptr; }
    std::lock_guard<std::mutex> lk(g_host_blocks_mu);
    g_host_blocks.push_back(HostBlock{ static_cast<char *>(p), bytes, static_cast<char *>(d) });
    return p;
}

void movba_host_free(void *p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_host_blocks_mu);
        for (size_t k = 0; k < g_host_blocks.size(); ++k)
            if (g_host_blocks[k].host == p) { g_host_blocks.erase(g_host_blocks.begin() + (long)k); break; }
    }
    (void)hipDeviceSynchronize();           // a kernel still writing results into the block
    (void)hipHostFree(p);
}

int movba_get_profile(movba_handle *h, movba_profile *out)
{
    if (!h || !out) return MOVBA_ERR_ARG;
    *out = h->prof;
    return MOVBA_OK;
}

int movba_set_profile_mask(movba_handle *h, int32_t mask)
{
    if (!h) return MOVBA_ERR_ARG;
    h->opt.profile = mask;
    return MOVBA_OK;
}

int movba_reset_profile(movba_handle *h)
{
    if (!h) return MOVBA_ERR_ARG;
    for (int k = 0; k < MOVBA_NKERNELS; ++k) { h->prof.ms[k] = 0; h->prof.launches[k] = 0; }
    h->prof.upload_ms = h->prof.structure_ms = h->prof.download_ms = 0;
    return MOVBA_OK;
}

}  // extern "C"
