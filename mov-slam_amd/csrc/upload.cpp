// movba_lba_upload / movba_lba_reset (include/movba.h): a window's edges, estimates and pair structure from the caller's
// arrays into the handle's arena, with the handle's helper thread copying the caller's big arrays beside the structure pass.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"
#include "kernels.h"

using namespace movba;

// =====================================================================================================================
// movba_lba_upload, in phases.  One Upload object lives for the duration of one call; its members say who owns what.
//
//   threads     the CALLER's thread runs every phase below.  The handle's HELPER thread (movba_handle::packer) runs the
//               closure post_helper() posts, which copies the caller's big arrays into the staging buffer and sends them
//               to the arena on the copy stream; in direct mode a second one, posted by post_early_setup(), which queues
//               the early setup launches.  Neither closure reads the Upload object: each holds values fixed before it is
//               posted, and writes to the hand-off object alone.
//   hand-off    HelperHandOff: the two things the helper produces for the caller (idx_ready, copy_err) and the things
//               fixed before it is posted.  Everything else in Upload belongs to the caller's thread alone.
//   staging     the pinned buffer is laid out like the edge region of the arena (EdgeLayout): the helper writes
//               [gpose, gpoint) index copies and [raw_begin, grouped_end) there, the caller everything else - and the
//               helper's parts only after join_helper() (+ copy_event, when they are to be rewritten).
//   streams     h->stream: structure kernels, derived arrays, pair region, and later the solve.  h->copy_stream: the
//               caller's arrays (helper) and the early copy of the derived edge arrays.
//   events      copy_event  (copy stream -> stream): the caller's arrays have arrived; recorded by the helper, waited for
//                           by the stream before the solve's first kernel (send_pairs) and by the host before the staging
//                           copy of those arrays is rewritten (ungrouped windows);
//               edgeb_event (copy stream -> stream): the derived edge arrays sent early have arrived; waited for by the
//                           stream ahead of the slot-completion / fill kernels (queue_edge_b).
//   arena       may be reallocated by ensure_arena() in lay_out_rest(): its generation (arena_gen) at the time something
//               was queued tells whether that something has to be queued again.
// =====================================================================================================================
namespace {

// memcpy that takes an empty source (a vector without storage has a null data()): copying nothing from nowhere is undefined
// behaviour for memcpy itself (found by UBSan over the host build, tests/hipstub)
inline void put(void *dst, const void *src, size_t bytes) { if (bytes) std::memcpy(dst, src, bytes); }

// byte offsets of the edge region's arrays, the same in the arena and in the staging buffer; fixed by the caller's counts
struct EdgeLayout {
    // (what the device structure pass reads comes first: it is copied ahead of the rest)
    size_t gpose = 0, ptstart = 0, hidx = 0;
    size_t a_end = 0;                   // end of that first part
    size_t gpoint = 0, free_pose = 0, slot = 0;
    size_t base = 0;                    // first pose-major slot of every keyframe (slots are completed on the device)
    // (the caller's own arrays, contiguous: they cross the bus on the copy stream, straight from the helper thread)
    size_t raw_begin = 0, obs = 0, isig = 0, obsr = 0, pose0 = 0, point0 = 0, kcam = 0;
    size_t grouped_end = 0;             // end of the region when the caller's edges come grouped by map point
    size_t perm = 0;                    // only travels when they do not
    size_t max_end = 0;
    bool has_kcam = false;              // intrinsics by keyframe (src/Optimizer.cc:664, 690-695)
};

constexpr int kSortedMaxPoses = 1024;   // windows the sort-based device structure pass takes (pair counts back: 4 NP^2 bytes of pinned memory)

// (below this many edges the host builds grouping, pair counts and entry lists itself: its passes are a few microseconds then,
//  less than the device's chain of launches and the two trips across the bus - 0.43 against 0.47 ms per call at 693 edges,
//  0.54 against 0.52 at 7 102, scripts/small_paths.py)
constexpr int kDeviceStructureMinEdges = 2048;

struct HelperHandOff {
    // helper -> caller
    std::atomic<int> idx_ready{0};      // the caller's index arrays are in the staging buffer (release / acquire): what the
                                        // structure pass on the device waits for

    hipError_t copy_err = hipSuccess;   // read by the caller only after Worker::wait()
    hipError_t idx_err = hipSuccess;    // ... this one behind idx_ready (release / acquire)
    // fixed before the helper is posted, read by both
    char *arena = nullptr;              // the arena the helper sends to ...
    uint64_t arena_gen = 0;             // ... and its generation: a reallocation later on is told by it
    // caller only
    bool joined = false;
};

// the per-keyframe intrinsics as DevWindow::kcam holds them, 8 doubles a keyframe: fx, fy, cx, cy, bf, 0, 0, 0
void pack_kcam(double *kc, const movba_lba_desc *d, int np)
{
    for (int i = 0; i < np; ++i) {
        const double *ck = d->cam_kf ? d->cam_kf + 4 * (size_t)i : &d->fx;      // (fx, fy, cx, cy are contiguous in the descriptor)
        kc[8 * i] = ck[0]; kc[8 * i + 1] = ck[1]; kc[8 * i + 2] = ck[2]; kc[8 * i + 3] = ck[3];
        kc[8 * i + 4] = d->bf_kf ? d->bf_kf[i] : d->bf; kc[8 * i + 5] = kc[8 * i + 6] = kc[8 * i + 7] = 0.0;
    }
}

// Launches of the structure pass that either thread may queue, as values: the slots' completion (k_slot_point) ...
struct SlotPointLaunch {
    int32_t *slot;
    const int32_t *g_pose, *base, *g_point;
    int32_t *slot_point;
    int E;
    const int32_t *hx;
    int NP;
};
hipError_t queue_slot_point(const SlotPointLaunch &a, hipStream_t s)
{
    return launch_slot_point(a.slot, a.g_pose, a.base, a.g_point, a.slot_point, a.E, a.hx, a.NP, s);
}

// ... and the fill of the entry lists: k_struct_fill, or the sort-based fill of struct_sort.hip where cnt_pt is set
struct FillLaunch {
    StructDev sd{};
    bool scan_first = false;            // k_struct_scan goes in front (launch_counts left it to the fill)
    const int32_t *cnt_pt = nullptr;
    int32_t *off = nullptr;
    unsigned *keys_in = nullptr, *keys_out = nullptr;
    unsigned long long *vals_in = nullptr;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    long long noff = 0;
};
hipError_t queue_fill(const FillLaunch &f, hipStream_t s)
{
    if (f.scan_first) { const hipError_t e = launch_struct_scan(f.sd, s); if (e != hipSuccess) return e; }
    if (f.cnt_pt) return launch_sorted_fill(f.sd, f.cnt_pt, f.off, f.keys_in, f.keys_out, f.vals_in, f.tmp, f.tmp_bytes, f.noff, s);
    return launch_struct_fill(f.sd, s);
}

// What the helper thread queues in direct mode behind the caller's arrays (post_early_setup): fixed by the caller's thread
// before it is posted and never changed after
struct EarlySetup {
    SlotPointLaunch slots;
    FillLaunch fill;
    DevWindow win;                      // state_view(): no pair-region field is set
    int delay_us;                       // (test hook helper_delay_us)
    bool laps;
    double t0;
};

struct Upload {
    movba_handle *const h;
    const movba_lba_desc *const d;
    const int NP, P, E;
    Carver c;                           // the arena's layout, carved phase by phase
    EdgeLayout L;
    HelperHandOff ho;
    char *sg = nullptr;                 // staging buffer
    size_t misc_bytes = 0;              // its tail: counts back / pair ids out (device structure pass)
    bool stereo = false;
    bool done = false;                  // the call is complete (early status): run() returns rc as it stands
    // --- grouping ---
    bool rank_mode = true;              // the staging buffer's slot array holds ranks; pose_slot0 the keyframes' first slots
    int nf = 0, nb = 0, nbins = 0;
    size_t edge_bytes = 0;
    // --- edge copies ---
    uint64_t arena_gen_at_edge_copy = 0;
    bool edge_b_early = false, edge_b_stale = false, edge_b_queued = false;
    double upload_host_ms = 0.0;
    // --- grouping pass on the device (group_on_device) ---
    int nf_expect = 0;                  // non-fixed keyframes: the free keyframes of the window unless one of them has no edge
    bool raw_synced = false;
    bool direct_raw = false;            // the caller's big arrays lie in movba_host_alloc memory: they cross the bus from where they are
    bool dev_first = false;             // validation, point ranges, hessian indices and slots are the device's work: no pass over the edges here
    BasicDev bd{};
    // --- structure pass on the device: scratch (carve_scratch), counts back (counts_out / wait_for_counts) ---
    size_t so_cnt = 0, so_err = 0, so_ent0 = 0, so_cntw = 0, so_cntpt = 0, so_pe = 0, so_info = 0, so_fixed = 0, so_H = 0;
    volatile int32_t *misc_seq = nullptr;
    int32_t seq = 0;
    // --- structure ---
    StructDev sd{};
    bool dev_structure = false, ent_packed = false, filled_early = false;
    bool scan_pending = false;          // k_struct_scan of this upload is still to be launched (in front of the fill)
    bool sorted_structure = false;      // the device pass of struct_sort.hip (beyond k_struct_pairs' 80 free keyframes)
    size_t s2_off = 0, s2_keys_in = 0, s2_keys_out = 0, s2_vals_in = 0, s2_tmp = 0, s2_tmp_bytes = 0;
    uint64_t fill_gen = 0;
    size_t noff = 0, o_ent = 0, o_slotpt = 0;
    // --- pair region / device-only region ---
    size_t pair_begin = 0, hole = 0, h2d = 0, total = 0;
    size_t o_items = 0, o_sched = 0, o_pi = 0, o_pj = 0, o_pis = 0, o_rowptr = 0, o_rowent = 0, o_plan = 0;
    size_t o_cg = 0, o_ch = 0, o_cp = 0, o_ce = 0, o_cij = 0, o_multi = 0, o_pid = 0, o_prange = 0, o_dtp = 0, o_dtk = 0;
    size_t o_st[2][11] = {};
    size_t o_obspm = 0, o_obsrpm = 0, o_part = 0, o_blocks = 0, o_blocks_ov = 0, o_blocks_c = 0, o_aci = 0, o_acitag = 0;
    size_t o_bp = 0, o_xp = 0, o_scale = 0, o_hmax = 0, o_tick = 0, o_recd = 0, o_imgb = 0, o_ctrl = 0, o_chi2 = 0, o_outl = 0;
    size_t o_dtiles = 0, o_ddiag = 0, o_dfail = 0, o_dx = 0, o_dflags = 0, o_dcontrib = 0, o_dstamps = 0;
    std::vector<int32_t> lane_plan;
    int rec_slots = 1;
    size_t ncb = 0;
    int ntile = 0;
    bool dense_one = false, dense_stamps = false;
    // --- timing ---
    double t0 = 0.0, lap_t = 0.0;
    bool lap_on = false;

    Upload(movba_handle *h_, const movba_lba_desc *d_) : h(h_), d(d_), NP(d_->n_poses), P(d_->n_points), E(d_->n_edges) {}
    // (every way out waits for the helper first: it reads the caller's arrays and writes to the hand-off object)
    // (... and in direct mode the copy engine reads the caller's own arrays: through with them before the caller has them back)
    ~Upload() { h->packer.wait(); if (direct_raw && !raw_synced) (void)hipStreamSynchronize(h->copy_stream); }

    const Structure &s() const { return h->st; }
    void lap(const char *what)
    {
        if (!lap_on) return;
        const double t = now_ms();
        std::fprintf(stderr, "libmovba[upload]: %-28s %.3f ms\n", what, t - lap_t);
        lap_t = t;
    }
    int join_helper()
    {
        if (ho.joined) return MOVBA_OK;
        h->packer.wait();
        ho.joined = true;
        if (ho.copy_err != hipSuccess) { std::fprintf(stderr, "libmovba: upload copy failed: %s\n", hipGetErrorString(ho.copy_err)); return MOVBA_ERR_HIP; }
        return MOVBA_OK;
    }

    int run(bool allow_dev_first);
    // phases, in the order run() takes them
    int begin();                        // arguments, edge layout, buffers, streams drained
    void post_helper();                 // the caller's arrays: staging buffer + copy stream, on the helper thread
    int group();                        // build_basic (grouping / validation); the early ways out
    bool dev_first_eligible() const;
    int group_on_device();              // ... the same on the device, behind the index arrays' way into the staging buffer
    void carve_state();                 // device-only arrays whose size follows from the caller's counts alone
    bool state_carved = false;
    int pack_derived();                 // derived edge arrays into the staging buffer
    int send_edge_a();                  // what the device structure pass reads -> stream; the rest early -> copy stream
    int structure_on_host();
    int structure_on_device();
    int structure_on_device_sorted();
    void choose_solver();
    int lay_out_rest();                 // pair region + device-only region; arena / staging buffer sized
    void pack_pairs();
    int send_pairs();
    void device_view();
    // pieces several phases share
    void pack_a(bool raw_too);          // what the device structure pass reads (first part of the edge region) ...
    void pack_b(bool raw_too);          // ... and the rest of the derived arrays
    void pack_edges(bool raw_too) { pack_a(raw_too); pack_b(raw_too); }
    int queue_edge_b();
    // ... of the device structure pass: scratch, counts there and back, the entry lists and the launches that fill them
    int carve_scratch(bool basic);
    void start_struct_dev();
    void aim_struct_dev();
    int launch_counts();
    int counts_out(const int32_t *basic_pe, const int32_t *basic_info);
    int wait_for_counts();
    int after_counts();
    int carve_entries();
    int finish_structure();
    SlotPointLaunch slot_point_launch() const;
    FillLaunch next_fill();
    int queue_slots_and_fill();
    int post_early_setup();
    DevWindow state_view() const;
    size_t ent_words() const { return (ent_packed ? 2 : 3) * noff + 4; }       // int32 words of the entry region
    char *sp(size_t o) const { return sg + (o - hole); }                        // staging address of a pair-region offset
    // tail of the staging buffer (the pair region is packed in front of it): nbins pair counts, the error word, the sequence
    // number of this upload[, kBasicInfo words, NP edges per keyframe]
    int32_t *misc() const { return reinterpret_cast<int32_t *>(sg + h->stage_cap - misc_bytes); }
};

int Upload::begin()
{
    HIP_TRY(hipSetDevice(h->device));
    h->uploaded = false; h->ran = false; h->early_status = MOVBA_OK; h->early_setup = false;
    t0 = lap_t = now_ms();
    lap_on = process_switches().time_upload;
    // ---- edge region of the arena, laid out from the caller's counts alone so that the helper thread can start copying the
    // caller's big arrays (observations, information, initial estimates: 3/4 of the region) into the pinned staging buffer
    // while this thread runs the grouping / validation pass.  Its H2D copies are queued as soon as it is packed, so that
    // the transfer runs while the pair structure is still being worked out ----
    if (NP < 0 || P < 0 || E < 0) return MOVBA_ERR_ARG;
    if ((NP && (!d->poses || !d->pose_fixed)) || (P && !d->points)) return MOVBA_ERR_ARG;
    if (E && (!d->edge_pose || !d->edge_point || !d->obs || !d->inv_sigma2)) return MOVBA_ERR_ARG;
    L.gpose = c.take<int32_t>(E); L.ptstart = c.take<int32_t>(P + 1); L.hidx = c.take<int32_t>(NP);
    L.a_end = c.off;
    L.gpoint = c.take<int32_t>(E);
    L.free_pose = c.take<int32_t>(NP + 1);
    L.slot = c.take<int32_t>(E);
    L.base = c.take<int32_t>(NP + 1);
    L.raw_begin = c.off;
    L.obs = c.take<double>(2 * (size_t)E); L.isig = c.take<double>(E);
    L.obsr = c.take<double>(d->obs_right ? E : 0);
    L.pose0 = c.take<double>(7 * (size_t)NP); L.point0 = c.take<double>(3 * (size_t)P);
    L.has_kcam = d->cam_kf || d->bf_kf;
    L.kcam = c.take<double>(L.has_kcam ? 8 * (size_t)NP : 0);
    L.grouped_end = c.off;
    L.perm = c.take<int32_t>(E);
    L.max_end = c.off;
    // (the device structure passes hand the pair counts back through the tail of the staging buffer: up to kSortedMaxPoses keyframes)
    const size_t nf_dev = (size_t)(NP <= kSortedMaxPoses ? NP : 80);
    misc_bytes = (nf_dev * nf_dev + 8) * sizeof(int32_t) * 2 + 4096 + sizeof(int32_t) * ((size_t)std::min(NP, 1024) + kBasicInfo + 8);
    int rc = ensure_stage(h, L.max_end + misc_bytes); if (rc) return rc;
    // first sizing of the arena: room for the states and pair lists too, so that it is not reallocated a moment later
    if (L.max_end > h->arena_cap) { rc = ensure_arena(h, 10 * L.max_end); if (rc) return rc; }
    HIP_TRY(hipStreamSynchronize(h->stream));     // staging buffer may still be in flight from a previous call
    HIP_TRY(hipStreamSynchronize(h->copy_stream));
    sg = h->stage;
    // (a window is a stereo window when any observation carries a right-image coordinate; looked up on this thread — the first
    //  stereo observation ends the scan — so that nothing the layout below depends on is produced by the helper thread)
    if (d->obs_right) for (int e = 0; e < E && !stereo; ++e) stereo = d->obs_right[e] >= 0.0;
    return MOVBA_OK;
}

// helper: straight copies of the caller's arrays (valid as they are when the edges come grouped by map point, the
// reference's own order; an ungrouped window has them permuted again by pack_b) on their way to the arena
void Upload::post_helper()
{
    ho.arena = h->arena;
    ho.arena_gen = h->arena_gen;
    // (by value: the layout, the buffers and the handle's streams; by reference: the hand-off object alone)
    const EdgeLayout lay = L;
    char *const stage = sg;
    movba_handle *const hh = h;
    const movba_lba_desc *const dd = d;
    const int np = NP, p = P, e = E;
    HelperHandOff *const out = &ho;
    if (direct_raw) {
        // Direct mode: every array of the caller lies in movba_host_alloc memory (pinned, mapped): nothing is staged.  The index
        // arrays, which the pair structure waits for, are read across the bus by a kernel on the handle's stream (k_ingest,
        // group_on_device: no copy command, no event between it and the grouping kernel); estimates, observations and
        // information go through the copy engine, queued here by the helper thread at once.  (A second k_ingest launch on the
        // copy stream was tried for them: the two streams share a hardware queue, and every kernel of the structure chain
        // queued behind it waited for its 60 us; the copy engine's commands cost ~8 us of latency each but run beside anything.)
        h->packer.post([=]() {
            hipError_t err = hipSetDevice(hh->device);
            // (The bus is shared: beside these 3.5 MB the index arrays' k_ingest takes 27 us for its 0.9 MB instead of 19 - 22.
            //  Holding the copy commands back behind that launch was tried: the last, small copy of the chain is a blit kernel,
            //  which then queued up behind the structure kernels of the handle's stream, and the solve's first kernels - which
            //  wait for it - started 25 us later: 1.107 ms per call against 1.09.  With that small copy sent first and only the
            //  large commands held back: the copy engine's chain - three commands of ~8 us latency each and 78 us of transfer -
            //  then ends ~25 us behind the structure kernels instead of ahead of them, and the solve's first kernels wait for IT:
            //  1.09 - 1.10 ms.  The bus time of the upload, ~85 us for 4.4 MB, has to start at once.)
            auto dma = [&](size_t to, const void *from, size_t bytes) {
                if (err == hipSuccess && bytes) err = hipMemcpyAsync(out->arena + to, from, bytes, hipMemcpyHostToDevice, hh->copy_stream);
            };
            dma(lay.obs, dd->obs, sizeof(double) * 2 * (size_t)e);
            dma(lay.isig, dd->inv_sigma2, sizeof(double) * (size_t)e);
            if (dd->obs_right) dma(lay.obsr, dd->obs_right, sizeof(double) * (size_t)e);
            dma(lay.point0, dd->points, sizeof(double) * 3 * (size_t)p);
            dma(lay.pose0, dd->poses, sizeof(double) * 7 * (size_t)np);
            if (lay.has_kcam) {
                pack_kcam(reinterpret_cast<double *>(stage + lay.kcam), dd, np);
                dma(lay.kcam, stage + lay.kcam, sizeof(double) * 8 * (size_t)np);
            }
            if (err == hipSuccess) err = hipEventRecord(hh->copy_event, hh->copy_stream);
            out->copy_err = err;
        });
        ho.idx_ready.store(1, std::memory_order_release);
        return;
    }
    // (test hook helper_delay_us: the helper starts that much later: whatever this thread takes from the helper
    //  without waiting for it shows up as a wrong result instead of hiding behind the usual timing)
    const int helper_delay_us = HOOK(h, helper_delay_us);
    const bool send_idx = dev_first;        // (device grouping pass: the index arrays cross first, on the copy stream, behind edgeb_event)
    h->packer.post([=]() {
        if (helper_delay_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(helper_delay_us));
        // (the index arrays as they are: right when the edges come grouped by point, overwritten by pack_a otherwise)
        std::memcpy(stage + lay.gpose, dd->edge_pose, sizeof(int32_t) * (size_t)e);
        std::memcpy(stage + lay.gpoint, dd->edge_point, sizeof(int32_t) * (size_t)e);
        if (send_idx) {
            hipError_t e0 = hipSetDevice(hh->device);
            if (e0 == hipSuccess) e0 = hipMemcpyAsync(out->arena + lay.gpose, stage + lay.gpose, sizeof(int32_t) * (size_t)e, hipMemcpyHostToDevice, hh->copy_stream);
            if (e0 == hipSuccess) e0 = hipMemcpyAsync(out->arena + lay.gpoint, stage + lay.gpoint, sizeof(int32_t) * (size_t)e, hipMemcpyHostToDevice, hh->copy_stream);
            if (e0 == hipSuccess) e0 = hipEventRecord(hh->edgeb_event, hh->copy_stream);
            out->idx_err = e0;
        }
        out->idx_ready.store(1, std::memory_order_release);
        // ... each part straight on to the device on the copy stream while the next one is being staged: most of the upload
        // is across the bus before the calling thread has finished its pass over the edges (the solve's first kernels wait
        // for copy_event, nothing else does)
        hipError_t err = hipSetDevice(hh->device);
        auto send = [&](size_t from, size_t to) {
            if (err == hipSuccess && to > from)
                err = hipMemcpyAsync(out->arena + from, stage + from, to - from, hipMemcpyHostToDevice, hh->copy_stream);
        };
        std::memcpy(stage + lay.obs, dd->obs, sizeof(double) * 2 * (size_t)e);
        send(lay.obs, lay.isig);
        std::memcpy(stage + lay.isig, dd->inv_sigma2, sizeof(double) * (size_t)e);
        if (dd->obs_right) std::memcpy(stage + lay.obsr, dd->obs_right, sizeof(double) * (size_t)e);
        std::memcpy(stage + lay.pose0, dd->poses, sizeof(double) * 7 * (size_t)np);
        std::memcpy(stage + lay.point0, dd->points, sizeof(double) * 3 * (size_t)p);
        if (lay.has_kcam) pack_kcam(reinterpret_cast<double *>(stage + lay.kcam), dd, np);
        send(lay.isig, lay.grouped_end);
        if (err == hipSuccess) err = hipEventRecord(hh->copy_event, hh->copy_stream);
        out->copy_err = err;
    });
}

int Upload::group()
{
    // (the pose-major slots are left to the device when the edges come grouped by point: the pass leaves each edge's rank
    // among its keyframe's edges where the slots go)
    h->st.no_reorder = h->opt.reorder == -1;
    const int rc = build_basic(*d, h->st, reinterpret_cast<int32_t *>(sg + L.slot));
    rank_mode = true;
    lap("build_basic");
    if (rc < 0) { (void)join_helper(); (void)hipStreamSynchronize(h->copy_stream); return rc; }
    h->stop = d->stop;
    if (rc == MOVBA_EMPTY || s().P == 0) { h->early_status = MOVBA_EMPTY; }
    else if (s().n_fixed == 0) { h->early_status = MOVBA_NO_FIXED; }
    if (h->early_status != MOVBA_OK) {
        const int rw = join_helper(); if (rw) return rw;
        h->prof.structure_ms += now_ms() - t0; h->uploaded = true; done = true; return MOVBA_OK;
    }
    nf = s().nfree;
    // beyond the one-launch direct solver (dense_plan.h) the multi-launch one holds the solution vector in LDS and the lower
    // block triangle in HBM: refused by name past that, instead of failing in a launch
    if (nf > MOVBA_MAX_FREE_KEYFRAMES) {
        (void)join_helper();
        std::fprintf(stderr, "libmovba: %d free keyframes: the reduced system exceeds the direct solver's capacity (%d)\n", nf, MOVBA_MAX_FREE_KEYFRAMES);
        return MOVBA_ERR_TOO_LARGE;
    }
    nb = (P + kPointsPerBlock - 1) / kPointsPerBlock;
    edge_bytes = s().already_grouped ? L.grouped_end : L.max_end;
    nbins = nf * nf;
    return MOVBA_OK;
}

// States, per-edge records, cost partials, controller, results: sizes from NP, P, E (and the free keyframes' number) alone, so
// that a device grouping pass can carve them BEFORE the pair structure exists and start the solve's first kernels on them.
// (pose-major arrays are sized for E edges of free keyframes, their upper bound)
void Upload::carve_state()
{
    for (int b = 0; b < 2; ++b) {
        o_st[b][0] = c.take<double>(7 * (size_t)NP); o_st[b][1] = c.take<double>(12 * (size_t)NP);
        o_st[b][2] = c.take<double>(3 * (size_t)P);  o_st[b][3] = c.take<double>(6 * (size_t)P);
        o_st[b][4] = c.take<double>(3 * (size_t)P);  o_st[b][5] = c.take<double>(4 * (size_t)E);       // erecA
        o_st[b][6] = 0;  o_st[b][7] = 0;
        o_st[b][8] = c.take<double>(nb);
        o_st[b][9] = 0;
        o_st[b][10] = 0;
    }
    o_obspm = c.take<double>(2 * (size_t)E + 2); o_obsrpm = c.take<double>(stereo ? (size_t)E + 1 : 1);
    o_aci = c.take<double>(3 * kCoarseDim * kCoarseDim + 2); o_acitag = c.take<int32_t>(2);
    o_bp = c.take<double>(6 * (size_t)nf + 1); o_xp = c.take<double>(6 * (size_t)nf + 1);
    o_scale = c.take<double>(nb + 1); o_hmax = c.take<double>(nb); o_tick = c.take<uint32_t>(8 * (size_t)nb + 8);
    o_ctrl = c.take<Ctrl>(1); o_chi2 = c.take<double>(E); o_outl = c.take<uint8_t>(E);
    state_carved = true;
}

// The grouping pass on the device: wanted where the device also builds the pair structure through its pair-bin masks (up to 80
// free keyframes: every window MoV-SLAM's local mapping produces) and where the host can tell from the keyframes' flags
// alone how many free keyframes there are.
bool Upload::dev_first_eligible() const
{
    if (HOOK(h, host_structure) || HOOK(h, host_grouping)) return false;
    if (E < kDeviceStructureMinEdges) return false;
    if (E <= 0 || P <= 0 || NP <= 0 || NP > 1024) return false;
    int nfix = 0;
    for (int i = 0; i < NP; ++i) nfix += d->pose_fixed[i] != 0;
    const int nfm = NP - nfix;
    return nfix > 0 && nfm > 0 && nfm <= 80 && struct_lds_fits(nfm, NP);
}

// What build_basic derives in one pass over the caller's edges on this thread (0.11 ms at cfg3, a tenth of the whole call, with
// the device idle but for the copies) is the device's work here: it validates the index arrays, finds the points' ranges,
// counts the edges per keyframe, numbers the free keyframes and ranks every edge among its keyframe's edges (k_basic_hist,
// k_basic_index), then counts the pair bins as before; this thread waits ONCE, for the pair counts and the edges per keyframe
// together, and rebuilds its own small tables (hessian indices, free poses, first slots) from the latter.  A window the pass
// cannot take as it is - edges not grouped by point, a free keyframe nobody observes - is handed back to the host pass.
constexpr int kRetryClassic = 1 << 20;
int Upload::group_on_device()
{
    Structure &st = h->st;
    reset_structure(st, NP, P, E);
    st.no_reorder = h->opt.reorder == -1;
    for (nf_expect = 0, nf = 0; nf < NP; ++nf) nf_expect += d->pose_fixed[nf] == 0;
    nf = nf_expect; nbins = nf * nf;
    nb = (P + kPointsPerBlock - 1) / kPointsPerBlock;
    edge_bytes = L.grouped_end;
    carve_state();
    int rc = carve_scratch(true); if (rc) return rc;
    char *sa = h->scratch.p;
    // (the keyframes' flags are read out of host memory - the staging buffer is mapped -, through the place of the hessian
    //  indices, which the device makes itself here)
    std::memcpy(sg + L.hidx, d->pose_fixed, (size_t)NP);
    // bin totals, error word, edges per keyframe, info words: cleared by the ingest launch itself (direct mode)
    const size_t zero_bytes = so_info + sizeof(int32_t) * kBasicInfo - so_cnt;
    if (!direct_raw) HIP_TRY(hipMemsetAsync(sa + so_cnt, 0, zero_bytes, h->stream));
    bd = BasicDev{};
    bd.E = E; bd.P = P; bd.NP = NP; bd.nblk = (E + kBasicBlock - 1) / kBasicBlock;
    if (direct_raw) {
        // The caller's index arrays out of its own pinned memory, by kernel (struct_kernels.hip: k_ingest), on this stream, in
        // front of the grouping kernel that reads them.
        auto view = [](const void *p, size_t bytes) { return static_cast<const void *>(host_block_view(p, bytes)); };
        IngestArgs ia{};
        ia.seg[0] = IngestSeg{ view(d->edge_pose, sizeof(int32_t) * (size_t)E), h->arena + L.gpose, sizeof(int32_t) * (size_t)E };
        ia.seg[1] = IngestSeg{ view(d->edge_point, sizeof(int32_t) * (size_t)E), h->arena + L.gpoint, sizeof(int32_t) * (size_t)E };
        // (the keyframes' flags with them: four bytes at a time out of the staging buffer's copy, which is padded)
        ia.seg[2] = IngestSeg{ h->stage_dev + L.hidx, sa + so_fixed, ((size_t)NP + 3) & ~(size_t)3 };
        ia.nseg = 3; ia.counter = h->ingest_counter; ia.wait_for = 0;
        ia.zero = reinterpret_cast<unsigned *>(sa + so_cnt); ia.zero_words = (unsigned)(zero_bytes / 4);
        HIP_TRY(launch_ingest(ia, h->stream));
        h->ingest_expect += (unsigned)ingest_workgroups();

    } else {
        // the index arrays are on their way on the copy stream (post_helper): the grouping kernel starts behind their event
        while (ho.idx_ready.load(std::memory_order_acquire) == 0) host_relax(h->opt.host_wait);
        if (ho.idx_err != hipSuccess) { std::fprintf(stderr, "libmovba: upload copy failed: %s\n", hipGetErrorString(ho.idx_err)); return MOVBA_ERR_HIP; }
        HIP_TRY(hipStreamWaitEvent(h->stream, h->edgeb_event, 0));
    }
    arena_gen_at_edge_copy = ho.arena_gen;
    bd.edge_pose = reinterpret_cast<const int32_t *>(h->arena + L.gpose); bd.edge_point = reinterpret_cast<const int32_t *>(h->arena + L.gpoint);
    // (staged mode: the flags are read out of the mapped staging buffer; direct mode: k_ingest has brought them along)
    bd.pose_fixed = direct_raw ? reinterpret_cast<const uint8_t *>(sa + so_fixed) : reinterpret_cast<const uint8_t *>(h->stage_dev + L.hidx);
    bd.pt_start = reinterpret_cast<int32_t *>(h->arena + L.ptstart); bd.rank = reinterpret_cast<int32_t *>(h->arena + L.slot);
    bd.H = reinterpret_cast<int32_t *>(sa + so_H); bd.pose_edges = reinterpret_cast<int32_t *>(sa + so_pe);
    bd.hidx = reinterpret_cast<int32_t *>(h->arena + L.hidx); bd.base = reinterpret_cast<int32_t *>(h->arena + L.base);
    bd.free_pose = reinterpret_cast<int32_t *>(h->arena + L.free_pose); bd.info = reinterpret_cast<int32_t *>(sa + so_info);
    HIP_TRY(launch_basic(bd, h->stream));
    rc = launch_counts(); if (rc) return rc;
    lap("grouping + count launches");
    rc = wait_for_counts(); if (rc) return rc;
    const int32_t *info = misc() + nbins + 2, *pe = info + kBasicInfo;
    if (info[0]) { (void)join_helper(); (void)hipStreamSynchronize(h->copy_stream); return MOVBA_ERR_ARG; }      // an index out of range
    if (info[1] || info[2] != nf_expect) return kRetryClassic;
    st.pose_edges.assign(pe, pe + NP); st.pose_edges.push_back(0);
    index_poses(d->pose_fixed, st);
    if (st.nfree != nf_expect || st.E_free != info[3]) return MOVBA_ERR_HIP;      // (the device and this thread number the same keyframes)
    st.already_grouped = true; st.perm.clear(); st.gp = d->edge_pose; st.gl = d->edge_point;
    st.pt_start.clear();        // (the points' ranges exist on the device only)
    rank_mode = true;
    h->stop = d->stop;
    lap("wait for the grouping pass and the pair counts");
    return MOVBA_OK;
}

void Upload::pack_a(bool raw_too)
{
    if (!s().already_grouped || raw_too) {         // (grouped order: the helper thread copied the caller's index arrays)
        put(sg + L.gpose, s().gp, sizeof(int32_t) * E);
        put(sg + L.gpoint, s().gl, sizeof(int32_t) * E);
    }
    put(sg + L.ptstart, s().pt_start.data(), sizeof(int32_t) * (P + 1));
    put(sg + L.hidx, s().hidx.data(), sizeof(int32_t) * NP);
}

void Upload::pack_b(bool raw_too)
{
    if (!s().already_grouped) put(sg + L.perm, s().perm.data(), sizeof(int32_t) * E);
    if (!rank_mode) put(sg + L.slot, s().slot.data(), sizeof(int32_t) * E);
    else put(sg + L.base, s().pose_slot0.data(), sizeof(int32_t) * NP);
    put(sg + L.free_pose, s().free_pose.data(), sizeof(int32_t) * nf);
    double *obs = reinterpret_cast<double *>(sg + L.obs), *isg = reinterpret_cast<double *>(sg + L.isig);
    double *obr = reinterpret_cast<double *>(sg + L.obsr);
    if (!s().already_grouped) {       // the helper's straight copies are in caller order: permute into grouped order
        for (int g = 0; g < E; ++g) {
            const int e = s().perm[g];
            obs[2 * g] = d->obs[2 * e]; obs[2 * g + 1] = d->obs[2 * e + 1]; isg[g] = d->inv_sigma2[e];
        }
        if (d->obs_right) for (int g = 0; g < E; ++g) obr[g] = d->obs_right[s().perm[g]];
    } else if (raw_too) {
        put(obs, d->obs, sizeof(double) * 2 * (size_t)E);
        put(isg, d->inv_sigma2, sizeof(double) * (size_t)E);
        if (d->obs_right) put(obr, d->obs_right, sizeof(double) * (size_t)E);
    }
    if (raw_too) {
        put(sg + L.pose0, d->poses, sizeof(double) * 7 * (size_t)NP);
        put(sg + L.point0, d->points, sizeof(double) * 3 * (size_t)P);
    }
}

int Upload::pack_derived()
{
    if (!s().already_grouped) {
        // (rare: the helper's straight copies get permuted below, so it has to be through with them)
        const int rw = join_helper(); if (rw) return rw;
        // ... and so do its transfers out of the staging buffer (found by ThreadSanitizer over the fake device, tests/hipstub: the
        // copy engine was still reading the caller-order observations while they were being permuted; harmless for the result —
        // the permuted region is sent again behind that copy — but a torn first copy is nothing to rely on)
        HIP_TRY(hipEventSynchronize(h->copy_event));
        build_slots(h->st); rank_mode = false;
        pack_edges(false);
    } else {
        while (ho.idx_ready.load(std::memory_order_acquire) == 0) host_relax(h->opt.host_wait);
        pack_a(false);
        pack_b(false);      // (ranks where the slots go, the keyframes' first slots, the free keyframes)
    }
    lap("pack derived arrays");
    return MOVBA_OK;
}

int Upload::send_edge_a()
{
    const double t_up0 = now_ms();
    HIP_TRY(hipMemcpyAsync(h->arena, sg, L.a_end, hipMemcpyHostToDevice, h->stream));
    arena_gen_at_edge_copy = ho.arena_gen;
    // grouped edges: the rest of the derived arrays (point ids, ranks / slots, first slots) leaves at once on the copy
    // stream, beside the structure kernels of this stream; what needs it (slot completion, fill) waits for edgeb_event
    // (not where the host goes on to build the pair structure itself - windows below kDeviceStructureMinEdges -: it packs its
    //  slots over the ranks in the staging buffer, which this copy would still be reading; that part then travels once, later)
    if (s().already_grouped && h->arena_gen == ho.arena_gen && E >= kDeviceStructureMinEdges && !HOOK(h, host_structure)) {
        HIP_TRY(hipMemcpyAsync(h->arena + L.a_end, sg + L.a_end, L.raw_begin - L.a_end, hipMemcpyHostToDevice, h->copy_stream));
        HIP_TRY(hipEventRecord(h->edgeb_event, h->copy_stream));
        edge_b_early = true;
    }
    upload_host_ms = now_ms() - t_up0;
    return MOVBA_OK;
}

int Upload::queue_edge_b()
{
    if (dev_first) { edge_b_queued = true; return MOVBA_OK; }       // (point ids, ranks, first slots: all made on the device)
    if (edge_b_early) HIP_TRY(hipStreamWaitEvent(h->stream, h->edgeb_event, 0));
    if (!edge_b_early || edge_b_stale) {
        // (not sent yet, or packed again since: host-built slots instead of ranks)
        HIP_TRY(hipMemcpyAsync(h->arena + L.a_end, sg + L.a_end, L.raw_begin - L.a_end, hipMemcpyHostToDevice, h->stream));
    }
    if (!s().already_grouped) {
        // the helper's straight copies were permuted again by pack_edges: that part travels once more, behind the first copy
        { const int rw = join_helper(); if (rw) return rw; }      // (its copy_event must have been recorded)
        HIP_TRY(hipStreamWaitEvent(h->stream, h->copy_event, 0));
        HIP_TRY(hipMemcpyAsync(h->arena + L.raw_begin, sg + L.raw_begin, edge_bytes - L.raw_begin, hipMemcpyHostToDevice, h->stream));
    }
    edge_b_queued = true;
    return MOVBA_OK;
}

// the per-pair entry lists built on the host (ungrouped edges, more than 80 free keyframes, or a pair-bin mask beyond LDS)
int Upload::structure_on_host()
{
    const int rc = build_structure(*d, h->st);         // (runs build_basic again, with the slots this time)
    if (rc < 0) return rc;
    rank_mode = false;
    pack_b(false); edge_b_stale = true;      // (slots instead of ranks in the staging buffer now)
    noff = (size_t)(s().nentries - s().E_free);
    o_slotpt = c.take<int32_t>((size_t)s().E_free + 1);
    return MOVBA_OK;
}

// scratch of the device structure pass (and of the device grouping pass in front of it); the sort-based pass keeps per-point
// couple counts where the mask pass keeps per-chunk counts
int Upload::carve_scratch(bool basic)
{
    const int nchunks = (P + 63) / 64;
    Carver sc;
    so_cnt = sc.take<int32_t>(nbins); so_err = sc.take<int32_t>(4);
    so_pe = sc.take<int32_t>(basic ? NP : 0); so_info = sc.take<int32_t>(basic ? kBasicInfo : 0);     // (zeroed together with the two above)
    so_ent0 = sc.take<int32_t>(nbins);
    so_cntw = sc.take<int32_t>(sorted_structure ? 0 : (size_t)nbins * nchunks);
    so_cntpt = sc.take<int32_t>(sorted_structure ? (size_t)P + 1 : 0);
    so_fixed = sc.take<uint8_t>(basic ? (size_t)NP + 4 : 0);
    so_H = sc.take<int32_t>(basic ? (size_t)((E + kBasicBlock - 1) / kBasicBlock) * NP : 0);
    return h->scratch.grow(h, sc.off);
}

// sd for this upload's structure pass: sizes and the scratch words of carve_scratch, then its arena addresses
void Upload::start_struct_dev()
{
    char *sa = h->scratch.p;
    sd = StructDev{};
    sd.P = P; sd.nfree = nf; sd.NP = NP;
    if (!sorted_structure) { sd.nchunks = (P + 63) / 64; sd.cntw = reinterpret_cast<int32_t *>(sa + so_cntw); }
    sd.cnt = reinterpret_cast<int32_t *>(sa + so_cnt); sd.error = reinterpret_cast<int32_t *>(sa + so_err);
    sd.ent0 = reinterpret_cast<int32_t *>(sa + so_ent0);
    sd.abort = dev_first ? reinterpret_cast<const int32_t *>(sa + so_info) : nullptr;
    aim_struct_dev();
}

// sd's addresses in the arena: the edge arrays where the edge copy (or the device grouping pass) put them, and the entry lists
// once carve_entries has placed them.  Set when the pass starts, when the entries are carved, and when lay_out_rest has moved
// the arena (the fill then runs again, on the new one).
void Upload::aim_struct_dev()
{
    char *a = h->arena;
    sd.g_pose = reinterpret_cast<int32_t *>(a + L.gpose); sd.pt_start = reinterpret_cast<int32_t *>(a + L.ptstart);
    sd.hidx = reinterpret_cast<int32_t *>(a + L.hidx);
    sd.slot = reinterpret_cast<const int32_t *>(a + L.slot);
    if (!o_ent) return;
    int32_t *ed = reinterpret_cast<int32_t *>(a + o_ent);
    sd.ent_i = ed; sd.ent_j = ed + noff; sd.ent_l = ed + 2 * noff;
    sd.ent64 = ent_packed ? reinterpret_cast<unsigned long long *>(a + o_ent) : nullptr;
}

// count launches of the device structure pass (struct_kernels.hip); the bins' totals (and, after a device grouping pass, its
// results) come back through the tail of the staging buffer
int Upload::launch_counts()
{
    start_struct_dev();
    HIP_TRY(launch_struct_count(sd, h->stream));
    const int rc = counts_out(dev_first ? reinterpret_cast<const int32_t *>(h->scratch.p + so_pe) : nullptr,
                              dev_first ? reinterpret_cast<const int32_t *>(h->scratch.p + so_info) : nullptr);
    if (rc) return rc;
    // (the scan over the chunks is what the FILL needs, not the host: in direct mode the helper thread launches it with the fill)
    scan_pending = dev_first && direct_raw && h->opt.profile == 0;
    if (!scan_pending) HIP_TRY(launch_struct_scan(sd, h->stream));
    return MOVBA_OK;
}

// the counts into misc(), behind this upload's sequence number (what wait_for_counts polls for)
int Upload::counts_out(const int32_t *basic_pe, const int32_t *basic_info)
{
    misc_seq = reinterpret_cast<volatile int32_t *>(misc()) + nbins + 1;
    seq = (int32_t)(++h->count_seq & 0x7fffffff);
    __atomic_store_n(misc_seq, seq - 1, __ATOMIC_RELAXED);
    HIP_TRY(launch_struct_counts_out(sd, reinterpret_cast<int32_t *>(h->stage_dev + h->stage_cap - misc_bytes), seq, h->stream, basic_pe, basic_info));
    return MOVBA_OK;
}

int Upload::wait_for_counts()
{
    const double t_wait = now_ms();
    while (__atomic_load_n(misc_seq, __ATOMIC_ACQUIRE) != seq) {
        host_relax(h->opt.host_wait);
        if (now_ms() - t_wait > 10000.0) { HIP_TRY(hipStreamSynchronize(h->stream)); if (__atomic_load_n(misc_seq, __ATOMIC_ACQUIRE) != seq) return MOVBA_ERR_HIP; }
    }
    return MOVBA_OK;
}

// ... counted and filled on the GPU (struct_kernels.hip): the reference's own edge order, up to 80 free keyframes
int Upload::structure_on_device()
{
    int rc = carve_scratch(false); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(h->scratch.p + so_cnt, 0, so_err + 16 - so_cnt, h->stream));        // bin totals and the error word
    rc = launch_counts(); if (rc) return rc;
    lap("edge H2D + count launches");
    return after_counts();
}

int Upload::after_counts()
{
    int32_t *cnt = misc();
    if (!dev_first) { const int rc = wait_for_counts(); if (rc) return rc; }
    if (cnt[nbins] != 0) return MOVBA_ERR_ARG;     // duplicate observation
    lap("wait for the pair counts");
    // covisibility ordering (structure.h): a window whose keyframe ids do not follow its covisibility graph is renumbered
    // here, from the counts: hessian indices, free-pose list and first slots are sent again (a few hundred bytes) and the
    // count / scan kernels run once more in the new numbering (the host permutes its copy of the counts itself)
    if (!h->st.no_reorder) {
        std::vector<int32_t> new_of_old;
        if (covisibility_order(nf, cnt, new_of_old)) {
            apply_pose_order(h->st, new_of_old, cnt);
            h->st.reordered = true;
            std::memcpy(sg + L.hidx, s().hidx.data(), sizeof(int32_t) * NP);
            std::memcpy(sg + L.base, s().pose_slot0.data(), sizeof(int32_t) * NP);
            std::memcpy(sg + L.free_pose, s().free_pose.data(), sizeof(int32_t) * nf);
            HIP_TRY(hipMemcpyAsync(h->arena + L.hidx, sg + L.hidx, sizeof(int32_t) * NP, hipMemcpyHostToDevice, h->stream));
            if (dev_first) {
                // (the device made these itself in the caller's numbering: only the three renumbered tables travel)
                HIP_TRY(hipMemcpyAsync(h->arena + L.base, sg + L.base, sizeof(int32_t) * NP, hipMemcpyHostToDevice, h->stream));
                HIP_TRY(hipMemcpyAsync(h->arena + L.free_pose, sg + L.free_pose, sizeof(int32_t) * nf, hipMemcpyHostToDevice, h->stream));
            } else edge_b_stale = true;
            HIP_TRY(hipMemsetAsync(h->scratch.p + so_cnt, 0, so_err + 16 - so_cnt, h->stream));
            HIP_TRY(launch_struct_count(sd, h->stream));
            HIP_TRY(launch_struct_counts_out(sd, nullptr, 0, h->stream));
            HIP_TRY(launch_struct_scan(sd, h->stream));
            scan_pending = false;
            lap("covisibility reorder + recount");
        }
    }
    // slots, point ids, observations and initial estimates cross the bus, then the entry lists are filled, while the
    // host lays out the pairs
    int rc = queue_edge_b(); if (rc) return rc;
    rc = carve_entries(); if (rc) return rc;
    if (c.off <= h->arena_cap && h->arena_gen == ho.arena_gen) {
        filled_early = true; fill_gen = h->arena_gen;
        if (dev_first && direct_raw && h->opt.profile == 0) rc = post_early_setup();      // (on the helper thread)
        else rc = queue_slots_and_fill();
        if (rc) return rc;
    }
    lap("edge B H2D + fill kernel (queued)");
    return finish_structure();
}

// the off-diagonal entries the pair counts add up to (bounded: the entry lists' offsets are int32), and the arena's entry lists
// and slot -> point map carved for them
int Upload::carve_entries()
{
    const int32_t *cnt = misc();
    int64_t n = 0;
    for (int i = 0; i < nf; ++i) for (int j = i + 1; j < nf; ++j) n += cnt[(size_t)i * nf + j];
    if (n > (int64_t)0x7fffffff / 4) return MOVBA_ERR_ARG;
    noff = (size_t)n;
    o_ent = c.take<int32_t>(ent_words());
    o_slotpt = c.take<int32_t>((size_t)s().E_free + 1);
    aim_struct_dev();
    return MOVBA_OK;
}

// the host's part of the pair structure, from the counts (finish_pairs): the entries it lays out are the ones carved
int Upload::finish_structure()
{
    const int rc = finish_pairs(h->st, misc());
    lap("finish_pairs");
    if (rc < 0) return rc;
    if ((size_t)(s().nentries - s().E_free) != noff) return MOVBA_ERR_ARG;
    return MOVBA_OK;
}

// ... beyond k_struct_pairs' reach (more than 80 free keyframes, or a pair-bin mask that does not fit LDS): counted by atomics
// and filled by a stable sort of the points' couples (struct_sort.hip); the same hand-offs with the host as above
int Upload::structure_on_device_sorted()
{
    sorted_structure = true;
    int rc = carve_scratch(false); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(h->scratch.p + so_cnt, 0, so_err + 16 - so_cnt, h->stream));        // bin totals and the error word
    start_struct_dev();
    HIP_TRY(launch_couple_count(sd, reinterpret_cast<int32_t *>(h->scratch.p + so_cntpt), h->stream));
    rc = counts_out(nullptr, nullptr); if (rc) return rc;
    lap("edge H2D + count launches");
    rc = wait_for_counts(); if (rc) return rc;
    if (misc()[nbins] != 0) return MOVBA_ERR_ARG;     // duplicate observation
    lap("wait for the pair counts");
    rc = queue_edge_b(); if (rc) return rc;
    rc = carve_entries(); if (rc) return rc;
    // keys, values and rocPRIM's temporary storage of the fill
    Carver s2;
    s2_off = s2.take<int32_t>((size_t)P + 1);
    s2_keys_in = s2.take<unsigned>(noff + 1); s2_keys_out = s2.take<unsigned>(noff + 1);
    s2_vals_in = s2.take<unsigned long long>(noff + 1);
    s2_tmp_bytes = sorted_fill_temp_bytes(P, (long long)noff, nf);
    s2_tmp = s2.take<char>(s2_tmp_bytes);
    rc = h->scratch2.grow(h, s2.off); if (rc) return rc;
    if (c.off <= h->arena_cap && h->arena_gen == ho.arena_gen) {
        rc = queue_slots_and_fill(); if (rc) return rc;
        filled_early = true; fill_gen = h->arena_gen;
    }
    lap("edge B H2D + fill kernels (queued)");
    return finish_structure();
}

// where the slots' completion reads and writes, in the arena as it is now
SlotPointLaunch Upload::slot_point_launch() const
{
    char *a = h->arena;
    return SlotPointLaunch{ reinterpret_cast<int32_t *>(a + L.slot), reinterpret_cast<const int32_t *>(a + L.gpose),
                            rank_mode ? reinterpret_cast<const int32_t *>(a + L.base) : nullptr, reinterpret_cast<const int32_t *>(a + L.gpoint),
                            reinterpret_cast<int32_t *>(a + o_slotpt), E, dev_first ? reinterpret_cast<const int32_t *>(h->scratch.p + so_H) : nullptr, NP };
}

// the fill as it is to be queued next: with the chunk scan in front where launch_counts left it to the fill (and then no more)
FillLaunch Upload::next_fill()
{
    FillLaunch f;
    f.sd = sd;
    f.scan_first = scan_pending;
    scan_pending = false;
    if (sorted_structure) {
        char *s2 = h->scratch2.p;
        f.cnt_pt = reinterpret_cast<const int32_t *>(h->scratch.p + so_cntpt); f.off = reinterpret_cast<int32_t *>(s2 + s2_off);
        f.keys_in = reinterpret_cast<unsigned *>(s2 + s2_keys_in); f.keys_out = reinterpret_cast<unsigned *>(s2 + s2_keys_out);
        f.vals_in = reinterpret_cast<unsigned long long *>(s2 + s2_vals_in);
        f.tmp = s2 + s2_tmp; f.tmp_bytes = s2_tmp_bytes; f.noff = (long long)noff;
    }
    return f;
}

// on this thread: the slots' completion (the fill reads them), then the fill of a device structure pass
int Upload::queue_slots_and_fill()
{
    HIP_TRY(queue_slot_point(slot_point_launch(), h->stream));
    if (dev_structure) HIP_TRY(queue_fill(next_fill(), h->stream));
    return MOVBA_OK;
}

// The slots' completion, the fill of the entry lists and the solve's first two kernels - state 0 from the uploaded estimates,
// the first linearisation: they need the edge data, the slots and the state arrays, none of which depends on the pair
// structure - are queued by the HELPER thread (idle in direct mode) while this thread lays out the pairs: four launches and an
// event wait are ~25 us of API calls that would otherwise stand in front of finish_pairs, and the kernels run in the shadow of
// the pair layout; movba_lba_run then starts with the Hpp pass.  Whatever order the two threads' commands reach the stream in,
// each of this thread's (the pair region's copy) is independent of the helper's; send_pairs joins the helper before the run
// can queue anything behind them.
int Upload::post_early_setup()
{
    { const int rw = join_helper(); if (rw) return rw; }      // (its DMA commands are queued: ~30 us into the call)
    // (everything the launches need, as one value: the closure reads nothing of this object, which goes on meanwhile)
    const EarlySetup es{ slot_point_launch(), next_fill(), state_view(), HOOK(h, helper_delay_us), lap_on, t0 };
    const int device = h->device;
    const hipStream_t stream = h->stream;
    const hipEvent_t copy_event = h->copy_event;
    HelperHandOff *const out = &ho;
    h->packer.post([es, device, stream, copy_event, out]() {
        if (es.delay_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(es.delay_us));
        double tl[6]; tl[0] = now_ms();
        hipError_t err = hipSetDevice(device);
        if (err == hipSuccess) err = queue_slot_point(es.slots, stream);
        tl[1] = now_ms();
        if (err == hipSuccess) err = queue_fill(es.fill, stream);
        tl[2] = now_ms();
        if (err == hipSuccess) err = hipStreamWaitEvent(stream, copy_event, 0);
        tl[3] = now_ms();
        if (err == hipSuccess) err = launch_init(es.win, stream);
        tl[4] = now_ms();
        if (err == hipSuccess) err = launch_linearize(es.win, stream);
        tl[5] = now_ms();
        out->copy_err = err;
        if (es.laps) std::fprintf(stderr, "libmovba[upload]: helper's launches (ms into the call): start %.3f, slots %.3f, scan + fill %.3f, event wait %.3f, init %.3f, linearise %.3f\n",
                                  tl[0] - es.t0, tl[1] - es.t0, tl[2] - es.t0, tl[3] - es.t0, tl[4] - es.t0, tl[5] - es.t0);
    });
    ho.joined = false;                              // (send_pairs waits for it)
    h->early_setup = true;
    return MOVBA_OK;
}

void Upload::choose_solver()
{
    h->pp = PcgParams{};
    h->rows_kernel = pcg_rows_supported(s().nfree, s().row_ptr.data(), &h->pp);
    // (test switch: the packed layout of the mat-vec's pair sums where the padded one would do - same bits, tests/test_gpu_parity.py)
    if (HOOK(h, pcg_packed)) h->pp.padded = 0;
    // A reduced matrix beyond the PCG workgroup's registers (dense covisibility: every keyframe pair shares points, as in the
    // reference's own windows, KeyFrame.cc:227-231; or simply more keyframes) is not iterated over from L2: the one-launch
    // direct solver takes the window from the first trial, whatever its pattern.  Measured (profiles/r03zd_solver_switch.log,
    // solve kernels per window solve): 50 keyframes, 900 gather entries, all in registers: PCG 0.71 ms, direct 1.30; 56
    // keyframes, 1 020 entries, the first to overflow: PCG 1.35, direct 1.26; 80 keyframes, 1 500 entries: 2.21 / 1.74; 50
    // keyframes with tracks of up to 20, 1 600 entries: 1.88 / 1.38 - the PCG's cost doubles the moment it spills, so that is
    // where the switch sits.
    // (movba_options::pcg_spill = 1 keeps the spilling PCG whatever the size; ::solver = 1 takes every window direct.)
    {
        const bool over = h->rows_kernel && h->pp.overflow;
        if (h->rows_kernel && ((over && !h->opt.pcg_spill) || h->opt.solver == 1)) h->rows_kernel = false;
    }
    // The banded factorisation in one workgroup (band_kernel.hip): every window whose band - in the numbering the upload has
    // settled on - fits one CU's LDS, the PCG's windows and the dense small ones of the direct solver alike.
    {
        int bw = 0;
        for (int p = nf; p < s().npairs; ++p) bw = std::max(bw, (int)(s().pair_j[p] - s().pair_i[p]));
        h->band_bw = bw;
        // ... where it is the faster of the two.  Its cost (tests/dev/band_scan.py, profiles/r04_band_scan.log; cycles from the
        // stamp build): per block step ~1 970 for the pivot block, ~780 per round of the panel, ~420 per round of 512 trailing
        // elements - with the AVERAGE number of blocks below a pivot, min(bw, nfree - 1 - k) over the steps -, plus assembly,
        // sweeps and epilogue; against the PCG's ~130 000 cycles whatever the size.  At a band of 9: 8 keyframes 0.49 ms per
        // resident window solve against 0.78, 16: 0.63 / 0.78, 24: 0.78 / 0.80, from 28 on the PCG wins (0.88 / 0.87; 40: 1.12 / 0.88).
        // MOVBA_BAND=0 / 1 (or movba_options::solver = 3 / 2) switch the choice off / force it.
        const int band_env = process_switches().band;
        double m_sum = 0.0;
        for (int k = 0; k < nf; ++k) m_sum += std::min(bw, nf - 1 - k);
        const double m_avg = nf > 0 ? m_sum / nf : 0.0;
        const double rt = std::ceil((m_avg * (m_avg + 1.0) * 18.0 + 6.0 * m_avg) / 512.0), rp = std::max(1.0, std::ceil(m_avg * 36.0 / 512.0));
        const double est = nf * (1970.0 + 780.0 * rp + 420.0 * rt) + 54.0 * nf * (bw + 1) + 360.0 * nf + 5000.0;
        // (the environment variable speaks for handles made with solver = 0 only)
        const bool forced = h->opt.solver == 2 || (h->opt.solver == 0 && band_env == 1);
        const bool off = h->opt.solver == 3 || h->opt.solver == 1 || (h->opt.solver == 0 && band_env == 0);
        const bool want = forced || (h->rows_kernel && est <= 130000.0);
        h->band = want && !off && band_supported(nf, bw);
    }
    if (h->rows_kernel && !h->band) build_coarse(h->st, h->pp.wave_row0, kPcgRowsThreads / 64);
    lap("pcg plan + coarse lists");
}

int Upload::lay_out_rest()
{
    // ---- pair region (second H2D copy): packed in the staging buffer right behind the edge region, `hole` bytes before
    // its place in the arena (the device-only arrays carved above sit in between) ----
    pair_begin = c.off; hole = pair_begin - L.max_end;
    o_items = c.take<Item>((size_t)s().nitems + 1); o_sched = c.take<SchedItem>(s().sched.size() + 1);
    o_pi = c.take<int32_t>(s().npairs + 1); o_pj = c.take<int32_t>(s().npairs + 1); o_pis = c.take<int32_t>(s().npairs + 1);
    o_rowptr = c.take<int32_t>(nf + 1); o_rowent = c.take<RowEnt>(s().row_ent.size() + 1);
    lane_plan.clear();
    if (h->rows_kernel) {
        // which two oriented blocks every lane of k_pcg_rows holds, and where their partial items are
        lane_plan.assign((size_t)kPcgRowsThreads * 12, -1);
        for (int wv = 0; wv < kPcgRowsThreads / 64; ++wv) {
            const int r0 = h->pp.wave_row0[wv], r1 = h->pp.wave_row0[wv + 1];
            const int P0 = s().row_ptr[r0] >> 1, P1 = s().row_ptr[r1] >> 1;
            for (int ln = 0; ln < 64 && P0 + ln < P1; ++ln)
                for (int k = 0; k < 2; ++k) {
                    const RowEnt &re = s().row_ent[2 * (P0 + ln) + k];
                    int32_t *pl = &lane_plan[((size_t)(wv * 64 + ln) * 3 + k) * 4];
                    if (re.block < 0) continue;
                    pl[0] = re.block; pl[1] = (re.col * 6) | (re.transposed ? (1 << 30) : 0);
                    pl[2] = s().pair_item_start[re.block]; pl[3] = s().pair_item_start[re.block + 1];
                }
            for (int ln = 0; ln < 64; ++ln) {               // owner lanes: what they need of their keyframe
                int32_t *pl = &lane_plan[((size_t)(wv * 64 + ln) * 3 + 2) * 4];
                pl[0] = pl[1] = pl[2] = pl[3] = 0;
                if (ln >= 6 * (r1 - r0)) continue;
                const int bi = r0 + ln / 6;
                pl[0] = s().pair_item_start[bi]; pl[1] = s().pair_item_start[bi + 1]; pl[2] = s().row_ptr[bi]; pl[3] = s().row_ptr[bi + 1];
            }
        }
        for (int wv = 0; wv <= kPcgRowsThreads / 64; ++wv) h->pp.wave_ent0[wv] = s().row_ptr[h->pp.wave_row0[wv]];
        h->pp.nrowent = s().row_ptr[nf];
    }
    // the diagonal items' records (DevWindow::rec_d): by keyframe and place in the pair
    rec_slots = 1;
    for (int hh = 0; hh < nf; ++hh) rec_slots = std::max(rec_slots, (int)(s().pair_item_start[hh + 1] - s().pair_item_start[hh]));
    // where the schur pass leaves the block of every single-item off-diagonal pair for those lanes (DevWindow::img_b)
    for (SchedItem &si : h->st.sched) {
        si.dst_a = -1; si.dst_b = -1;
        if (si.tag >= 0 && (si.tag & 1)) { const Item &it = s().items[(size_t)(si.tag >> 1)]; si.dst_a = it.pair * rec_slots + ((si.tag >> 1) - s().pair_item_start[it.pair]); }
    }
    if (h->rows_kernel && !h->pp.overflow) {
        std::vector<int32_t> slot_of_item((size_t)s().nitems, -1);
        for (size_t q = 0; q < s().sched.size(); ++q)      // (the slot of the wave that stores the item: place 0 among the item's waves)
            if (s().sched[q].tag >= 0 && (s().sched[q].sub & 0xff) == 0) slot_of_item[(size_t)(s().sched[q].tag >> 1)] = (int32_t)q;
        for (int t = 0; t < kPcgRowsThreads; ++t)
            for (int k = 0; k < 2; ++k) {
                const int32_t *pl = &lane_plan[((size_t)t * 3 + k) * 4];
                if (pl[0] < nf || pl[3] - pl[2] != 1) continue;         // no block, a diagonal one, or a pair cut into several items
                SchedItem &si = h->st.sched[(size_t)slot_of_item[(size_t)pl[2]]];
                const int32_t dst = 36 * k * kPcgRowsThreads + t;
                if ((pl[1] >> 30) & 1) si.dst_b = dst; else si.dst_a = dst;
            }
    }
    ncb = s().cblk_g.size();
    o_plan = c.take<int32_t>(lane_plan.size() + 4);
    o_cg = c.take<int32_t>(ncb + 1); o_ch = c.take<int32_t>(ncb + 1); o_cp = c.take<int32_t>(ncb + 2); o_ce = c.take<int32_t>(s().cblk_ent.size() + 1);
    o_cij = c.take<int32_t>(s().cblk_ij.size() + 1); o_multi = c.take<int32_t>(s().multi_pairs.size() + 1);
    o_pid = c.take<int32_t>((size_t)nf * nf + 1);                                // block -> pair map of the direct solver's assembly
    // one-launch direct solver: the static schedule depends on the number of block columns only (rebuilt when that changes)
    ntile = dense_ntile(nf);
    const bool dense_multi = process_switches().dense_multilaunch;
    // every workgroup of the one-launch solver must be resident while it runs: no more of them than the device (a partition
    // of an MI355X in CPX mode shows 32 compute units) has to give, a thirty-second held back as on the whole chip (248 of
    // 256); a plan that then needs more tiles per workgroup than fit LDS falls to the multi-launch solver
    const int dense_groups = std::min(kDenseMaxGroups, h->device_cus - std::max(1, h->device_cus / 32));
    if (h->dplan_nt != ntile) { build_dense_plan(ntile, h->dplan, std::max(dense_groups, 1)); h->dplan_nt = ntile; }
    dense_one = !dense_multi && dense_groups >= 8 && dense_persist_supported(h->dplan);
    o_dtp = c.take<int32_t>(dense_one ? h->dplan.task_ptr.size() : 1); o_dtk = c.take<DenseTask>(dense_one ? h->dplan.tasks.size() : 1);
    o_prange = c.take<int32_t>(dense_one ? 2 * (size_t)nf * nf : 1);
    if (!dev_structure) o_ent = c.take<int32_t>(ent_words());       // host-built entry lists (off-diagonal; the diagonal ones are their slot) travel with the pair region
    h2d = c.off;
    // ---- device-only region (what does not depend on the pair structure: carve_state) ----
    if (!state_carved) carve_state();
    const size_t part_stride = ((size_t)s().nitems * kPartStride + 31) / 32 * 32;
    o_part = c.take<double>(part_stride + 1); o_blocks = c.take<double>((size_t)s().npairs * 36 + 1);
    o_recd = c.take<double>((size_t)nf * rec_slots * 48 + 2); o_imgb = c.take<double>((size_t)72 * kPcgRowsThreads);
    o_blocks_ov = c.take<double>(h->rows_kernel && h->pp.overflow ? s().row_ent.size() * 36 + 2 : 2);
    o_blocks_c = c.take<double>((size_t)s().npairs * 36 + 1);
    // direct solver (dense_solve.hip): tiles of the lower block triangle + right-hand side row, diagonal factors, failure flag
    o_dtiles = c.take<double>(dense_tiles_doubles(nf)); o_ddiag = c.take<double>((size_t)ntile * kDenseNB * kDenseNB + 1); o_dfail = c.take<int32_t>(4);
    o_dx = c.take<double>((size_t)ntile * kDenseNB + 1);
    o_dflags = c.take<uint32_t>(dense_one ? (size_t)dense_flag_words(ntile) : 8);
    o_dcontrib = c.take<double>(dense_one ? (size_t)ntile * ntile * kDenseNB : 1);
    dense_stamps = process_switches().dense_stamps;
    o_dstamps = c.take<unsigned long long>(dense_one && dense_stamps ? 6 * h->dplan.tasks.size() : 1);
    total = c.off;

    // (a reallocation of the arena or of the staging buffer below must find the helper thread through with both: it reads
    //  the caller's arrays into the staging buffer and sends them to the arena it was given at the start)
    if (total > h->arena_cap || h2d - hole + misc_bytes > h->stage_cap) { const int rw = join_helper(); if (rw) return rw; }
    int rc = ensure_arena(h, total); if (rc) return rc;
    if (dev_first && (h->arena_gen != arena_gen_at_edge_copy || h2d - hole + misc_bytes > h->stage_cap)) return kRetryClassic;   // (tables the device made are gone with the old arena)
    if (h->arena_gen != arena_gen_at_edge_copy) {
        // the arena was reallocated (told by its generation: the new allocation may sit at the old address): queue the
        // edge region again (the staging copy is intact); the fill below then runs on the new arena
        HIP_TRY(hipMemcpyAsync(h->arena, sg, edge_bytes, hipMemcpyHostToDevice, h->stream));
        aim_struct_dev();
    }
    if (h2d - hole + misc_bytes > h->stage_cap) {
        // (rare: huge host-built entry lists) a bigger staging buffer: ensure_stage drains the stream first, so the edge copy
        // has landed; the edge region is packed again only to keep the buffer self-consistent
        rc = ensure_stage(h, h2d - hole + misc_bytes); if (rc) return rc;
        sg = h->stage;
        pack_edges(true);
    }
    return MOVBA_OK;
}

void Upload::pack_pairs()
{
    if (!dev_structure && noff) {
        int32_t *eh = reinterpret_cast<int32_t *>(sp(o_ent));
        if (ent_packed) {
            unsigned long long *e64 = reinterpret_cast<unsigned long long *>(eh);
            for (size_t k = 0; k < noff; ++k) e64[k] = ent_pack(s().ent_i[k], s().ent_j[k], s().ent_l[k]);
        } else {
            put(eh, s().ent_i.data(), sizeof(int32_t) * noff); put(eh + noff, s().ent_j.data(), sizeof(int32_t) * noff);
            put(eh + 2 * noff, s().ent_l.data(), sizeof(int32_t) * noff);
        }
    }
    put(sp(o_items), s().items.data(), sizeof(Item) * (size_t)s().nitems);
    put(sp(o_sched), s().sched.data(), sizeof(SchedItem) * s().sched.size());
    put(sp(o_pi), s().pair_i.data(), sizeof(int32_t) * s().npairs);
    put(sp(o_pj), s().pair_j.data(), sizeof(int32_t) * s().npairs);
    put(sp(o_pis), s().pair_item_start.data(), sizeof(int32_t) * (s().npairs + 1));
    put(sp(o_rowptr), s().row_ptr.data(), sizeof(int32_t) * (nf + 1));
    put(sp(o_rowent), s().row_ent.data(), sizeof(RowEnt) * s().row_ent.size());
    if (!lane_plan.empty()) put(sp(o_plan), lane_plan.data(), sizeof(int32_t) * lane_plan.size());
    put(sp(o_cg), s().cblk_g.data(), sizeof(int32_t) * ncb);
    put(sp(o_ch), s().cblk_h.data(), sizeof(int32_t) * ncb);
    put(sp(o_cp), s().cblk_ptr.data(), sizeof(int32_t) * s().cblk_ptr.size());
    put(sp(o_ce), s().cblk_ent.data(), sizeof(int32_t) * s().cblk_ent.size());
    put(sp(o_cij), s().cblk_ij.data(), sizeof(int32_t) * s().cblk_ij.size());
    put(sp(o_multi), s().multi_pairs.data(), sizeof(int32_t) * s().multi_pairs.size());
    put(sp(o_pid), s().pid.data(), sizeof(int32_t) * (size_t)nf * nf);
    if (dense_one) {
        put(sp(o_dtp), h->dplan.task_ptr.data(), sizeof(int32_t) * h->dplan.task_ptr.size());
        put(sp(o_dtk), h->dplan.tasks.data(), sizeof(DenseTask) * h->dplan.tasks.size());
        int32_t *pr = reinterpret_cast<int32_t *>(sp(o_prange));
        for (size_t q = 0; q < (size_t)nf * nf; ++q) {
            const int32_t pair = s().pid[q];
            pr[2 * q] = pair >= 0 ? s().pair_item_start[pair] : 0;
            pr[2 * q + 1] = pair >= 0 ? s().pair_item_start[pair + 1] : 0;
        }
    }
    lap("carve + pack pair region");
}

int Upload::send_pairs()
{
    const double t2 = now_ms();
    h->prof.structure_ms += (t2 - t0) - upload_host_ms;
    // The pair region (~100 KB at cfg3) stands between the last structure kernel and the solve's first pass over the pairs: a
    // copy command costs it ~10 us to start and ~9 us to be seen finished by the kernel behind it; read out of the (mapped)
    // staging buffer by k_ingest it is one more kernel in the chain.  Large regions (host-built entry lists) take the copy engine.
    if (h2d - pair_begin <= (size_t)1 << 20) {
        IngestArgs ia{};
        ia.seg[0] = IngestSeg{ h->stage_dev + L.max_end, h->arena + pair_begin, ((h2d - pair_begin) + 3) & ~(size_t)3 };
        ia.nseg = 1; ia.counter = nullptr; ia.wait_for = 0;
        HIP_TRY(launch_ingest(ia, h->stream));
    } else
        HIP_TRY(hipMemcpyAsync(h->arena + pair_begin, sg + L.max_end, h2d - pair_begin, hipMemcpyHostToDevice, h->stream));
    if (!(filled_early && fill_gen == h->arena_gen)) { const int rq = queue_slots_and_fill(); if (rq) return rq; }
    // the solve's kernels start behind the caller's arrays on the copy stream (the structure pass above did not need them)
    { const int rw = join_helper(); if (rw) return rw; }          // (the helper has recorded copy_event by now)
    HIP_TRY(hipStreamWaitEvent(h->stream, h->copy_event, 0));
    // (arrays the copy engine reads out of the caller's own memory: through before the caller has them back)
    if (direct_raw) { HIP_TRY(hipEventSynchronize(h->copy_event)); raw_synced = true; }
    // no synchronise: the solve's kernels queue on the same stream behind these transfers, and the caller's buffers were
    // copied to the staging buffer already (the next upload synchronises before it refills it)
    lap("pair H2D (queued)");
    h->prof.upload_ms += now_ms() - t2 + upload_host_ms;
    h->h2d_bytes = h2d;
    return MOVBA_OK;
}

// The window's device view as far as it exists once carve_state() and the entry / slot carving have run: the window's sizes
// and settings, the edge region, the states, the per-edge arrays, controller, cost partials, ticks, results, and the entry
// lists with their slot -> point map.  Every pair-region field stays null or zero, direct_only included (device_view() adds
// them).  The early setup (post_early_setup) launches with this view; what its kernels read of it (kernels.hip):
//   k_init_pose               NP, P, n_pt_blocks, max_iters, pose0, point0, st[0], ctrl, dec_rec, aci_tag, ac_prev
//   k_point<false, *, *>,     NP, P, E, nfree, n_pt_blocks, st, ctrl, pt_start, g_pose, hidx, slot, obs, obs_r, isig, obs_pm,
//   k_point_kf<false, *>      obsr_pm, xp, hmax_part, out_chi2, dec_rec, huber_delta, and the camera: fx, fy, cx, cy, bf, kcam
//   launch_linearize          kcam, stereo, lds_poses, n_pt_blocks (and, for the LDS size, NP, nfree)
DevWindow Upload::state_view() const
{
    char *a = h->arena;
    DevWindow w{};
    w.NP = NP; w.P = P; w.E = E; w.nfree = nf; w.n_pt_blocks = nb;
    w.max_iters = d->max_iters; w.flags = d->flags; w.max_trials = d->max_trials > 0 ? d->max_trials : 10;
    w.fx = d->fx; w.fy = d->fy; w.cx = d->cx; w.cy = d->cy; w.huber_delta = d->huber_delta; w.chi2_gate = d->chi2_gate;
    w.g_pose = reinterpret_cast<int32_t *>(a + L.gpose); w.g_point = reinterpret_cast<int32_t *>(a + L.gpoint);
    w.pt_start = reinterpret_cast<int32_t *>(a + L.ptstart); w.perm = s().already_grouped ? nullptr : reinterpret_cast<int32_t *>(a + L.perm);
    w.hidx = reinterpret_cast<int32_t *>(a + L.hidx); w.free_pose = reinterpret_cast<int32_t *>(a + L.free_pose);
    w.obs = reinterpret_cast<double *>(a + L.obs); w.isig = reinterpret_cast<double *>(a + L.isig);
    w.obs_r = d->obs_right ? reinterpret_cast<double *>(a + L.obsr) : nullptr; w.bf = d->bf; w.stereo = stereo ? 1 : 0;
    w.kcam = L.has_kcam ? reinterpret_cast<const double *>(a + L.kcam) : nullptr;
    w.slot = reinterpret_cast<int32_t *>(a + L.slot);
    w.obs_pm = reinterpret_cast<double *>(a + o_obspm); w.obsr_pm = reinterpret_cast<double *>(a + o_obsrpm);
    {
        const int32_t *ed = reinterpret_cast<const int32_t *>(a + o_ent);
        w.ent_i = ed; w.ent_j = ed + noff; w.ent_l = ed + 2 * noff;
        w.ent64 = ent_packed ? reinterpret_cast<const unsigned long long *>(a + o_ent) : nullptr;
        w.slot_point = reinterpret_cast<const int32_t *>(a + o_slotpt); w.n_diag = s().E_free;
    }
    w.pose0 = reinterpret_cast<double *>(a + L.pose0); w.point0 = reinterpret_cast<double *>(a + L.point0);
    for (int b = 0; b < 2; ++b) {
        DevState &S = w.st[b];
        S.pose = reinterpret_cast<double *>(a + o_st[b][0]); S.Rt = reinterpret_cast<double *>(a + o_st[b][1]);
        S.point = reinterpret_cast<double *>(a + o_st[b][2]); S.Hll = reinterpret_cast<double *>(a + o_st[b][3]);
        S.bl = reinterpret_cast<double *>(a + o_st[b][4]); S.erecA = reinterpret_cast<double *>(a + o_st[b][5]);
        S.Fpart = reinterpret_cast<double *>(a + o_st[b][8]);
    }
    w.aci = reinterpret_cast<float *>(a + o_aci); w.ac_prev = reinterpret_cast<double *>(a + o_aci) + 2 * kCoarseDim * kCoarseDim; w.aci_tag = reinterpret_cast<int32_t *>(a + o_acitag);
    w.bp = reinterpret_cast<double *>(a + o_bp); w.xp = reinterpret_cast<double *>(a + o_xp);
    w.scale_part = reinterpret_cast<double *>(a + o_scale); w.hmax_part = reinterpret_cast<double *>(a + o_hmax);
    w.dec_rec = reinterpret_cast<unsigned *>(a + o_tick);
    w.ctrl = reinterpret_cast<Ctrl *>(a + o_ctrl); w.hstat = h->hstat_dev; w.ctrl_out = h->ctrl_host_dev;
    w.out_chi2 = reinterpret_cast<double *>(a + o_chi2); w.out_outlier = reinterpret_cast<uint8_t *>(a + o_outl);
    w.wait_ticks = 2000000ull;
    w.lds_poses = point_lds_need(NP, nf) <= kPointLdsLimit ? 1 : 0;
    return w;
}

// the handle's view of the uploaded window: state_view() and the pair region
void Upload::device_view()
{
    DevWindow &w = h->win;
    char *a = h->arena;
    w = state_view();
    w.npairs = s().npairs; w.nitems = s().nitems;
    w.items = reinterpret_cast<Item *>(a + o_items);
    w.sched = reinterpret_cast<SchedItem *>(a + o_sched); w.sched_per_xcd = s().sched_per_xcd;
    w.pair_i = reinterpret_cast<int32_t *>(a + o_pi); w.pair_j = reinterpret_cast<int32_t *>(a + o_pj);
    w.pair_item_start = reinterpret_cast<int32_t *>(a + o_pis); w.row_ptr = reinterpret_cast<int32_t *>(a + o_rowptr);
    w.row_ent = reinterpret_cast<RowEnt *>(a + o_rowent);
    w.lane_plan = reinterpret_cast<int32_t *>(a + o_plan);
    w.n_agg = s().n_agg; w.n_cblk = (int32_t)ncb;
    w.cblk_g = reinterpret_cast<int32_t *>(a + o_cg); w.cblk_h = reinterpret_cast<int32_t *>(a + o_ch);
    w.cblk_ptr = reinterpret_cast<int32_t *>(a + o_cp); w.cblk_ent = reinterpret_cast<int32_t *>(a + o_ce);
    w.cblk_ij = reinterpret_cast<int32_t *>(a + o_cij);
    w.multi_pairs = reinterpret_cast<int32_t *>(a + o_multi); w.n_multi = (int32_t)s().multi_pairs.size();
    w.part = reinterpret_cast<double *>(a + o_part); w.blocks = reinterpret_cast<double *>(a + o_blocks);
    w.rec_d = reinterpret_cast<double *>(a + o_recd); w.img_b = reinterpret_cast<double *>(a + o_imgb); w.rec_slots = rec_slots;
    w.blocks_c = reinterpret_cast<double *>(a + o_blocks_c); w.blocks_ov = reinterpret_cast<double *>(a + o_blocks_ov);
    w.dense.tiles = reinterpret_cast<double *>(a + o_dtiles); w.dense.diagL = reinterpret_cast<double *>(a + o_ddiag);
    w.dense.pid = reinterpret_cast<const int32_t *>(a + o_pid); w.dense.fail = reinterpret_cast<int32_t *>(a + o_dfail);
    w.dense.prange = dense_one ? reinterpret_cast<const int32_t *>(a + o_prange) : nullptr;
    w.dense.ntile = ntile; w.dense.n = 6 * nf; w.dense.xsol = reinterpret_cast<double *>(a + o_dx);
    w.dense.task_ptr = reinterpret_cast<const int32_t *>(a + o_dtp); w.dense.tasks = reinterpret_cast<const DenseTask *>(a + o_dtk);
    w.dense.flags = reinterpret_cast<unsigned *>(a + o_dflags); w.dense.failw = w.dense.flags + dense_flag_count(ntile);
    w.dense.ctag = w.dense.flags + dense_ctag_word(ntile);
    w.dense.contrib = reinterpret_cast<double *>(a + o_dcontrib);
    w.dense.stamps = dense_one && dense_stamps ? reinterpret_cast<unsigned long long *>(a + o_dstamps) : nullptr;
    w.dense.G = dense_one ? h->dplan.G : 0; w.dense.slots = dense_one ? h->dplan.slots : 0;
    h->dense_flags_clean = false; h->dense_epoch = 0;
    w.direct_only = h->rows_kernel ? 0 : 1;
}
int Upload::run(bool allow_dev_first)
{
    int rc = begin(); if (rc) return rc;
    dev_first = allow_dev_first && dev_first_eligible();
    if (dev_first) {
        // arrays of the caller that lie in movba_host_alloc memory (pinned, mapped) are read by the device where they are
        direct_raw = host_block_view(d->edge_pose, sizeof(int32_t) * (size_t)E) && host_block_view(d->edge_point, sizeof(int32_t) * (size_t)E) && host_block_view(d->obs, sizeof(double) * 2 * (size_t)E) && host_block_view(d->inv_sigma2, sizeof(double) * (size_t)E) &&
                     host_block_view(d->poses, sizeof(double) * 7 * (size_t)NP) && host_block_view(d->points, sizeof(double) * 3 * (size_t)P) &&
                     (!d->obs_right || host_block_view(d->obs_right, sizeof(double) * (size_t)E));
    }
    post_helper();
    if (dev_first) {
        rc = group_on_device(); if (rc) return rc;
        ent_packed = s().E_free < kEntPackSlots && P < kEntPackPoints && !HOOK(h, entries_unpacked);
        dev_structure = true;
        rc = after_counts(); if (rc) return rc;
        choose_solver();
        rc = lay_out_rest(); if (rc) return rc;
        pack_pairs();
        rc = send_pairs(); if (rc) return rc;
        device_view();
        h->uploaded = true;
        return MOVBA_OK;
    }
    rc = group(); if (rc || done) return rc;
    rc = pack_derived(); if (rc) return rc;
    rc = send_edge_a(); if (rc) return rc;
    // The per-pair entry lists are counted and filled on the GPU (struct_kernels.hip) when the caller's edges are
    // already grouped by map point (the reference's own order) and the pair-bin masks fit in LDS; otherwise on the host.
    // (on the device: up to 80 free keyframes, and as many keyframes in all as the kernels' LDS image has room for)
    const bool on_device = s().already_grouped && s().nfree > 0 && !HOOK(h, host_structure) && E >= kDeviceStructureMinEdges;
    const bool masks_fit = s().nfree <= 80 && struct_lds_fits(s().nfree, NP);
    // entry lists and slot -> point map: device-only, carved ahead of the pair region so that the fill kernel can be
    // launched before the pair region is laid out (host-built entry lists travel inside the pair region instead)
    // 8-byte packed entries when slots and point ids fit (any realistic window; the test hook entries_unpacked keeps the 12-byte form)
    ent_packed = s().E_free < kEntPackSlots && P < kEntPackPoints && !HOOK(h, entries_unpacked);
    // (beyond the pair-bin masks: the sort-based pass, for packed entries and up to kSortedMaxPoses keyframes)
    const bool sorted = on_device && !masks_fit && ent_packed && NP <= kSortedMaxPoses && !HOOK(h, no_sorted_structure);
    dev_structure = on_device && (masks_fit || sorted);
    rc = !dev_structure ? structure_on_host() : (masks_fit ? structure_on_device() : structure_on_device_sorted()); if (rc) return rc;
    if (!edge_b_queued) { rc = queue_edge_b(); if (rc) return rc; }
    choose_solver();
    rc = lay_out_rest(); if (rc) return rc;
    pack_pairs();
    rc = send_pairs(); if (rc) return rc;
    device_view();
    h->uploaded = true;
    return MOVBA_OK;
}

}  // namespace

extern "C" {

int movba_lba_upload(movba_handle *h, const movba_lba_desc *d)
{
    if (!h || !d) return MOVBA_ERR_ARG;
    int rc;
    {
        Upload u(h, d);
        rc = u.run(true);
    }
    if (rc == kRetryClassic) {
        // (edges not grouped by point, a free keyframe without an edge, an arena that had to grow under the device's own tables:
        //  once more with the grouping pass on this thread)
        Upload u(h, d);
        rc = u.run(false);
    }
    // (movba_lba_marginals: fixed keyframes get zero blocks, free ones outside the system NaN - the hessian index alone does not
    //  tell them apart)
    STAMP_HOST(if (rc == MOVBA_OK) rc = stamp_window(h));
    if (rc == MOVBA_OK) h->pose_fixed.assign(d->pose_fixed, d->pose_fixed + (d->pose_fixed ? d->n_poses : 0));
    return rc;
}

int movba_lba_reset(movba_handle *h)
{
    if (!h) return MOVBA_ERR_ARG;
    if (!h->uploaded) return MOVBA_ERR_STATE;
    h->ran = false;
    return MOVBA_OK;
}

}  // extern "C"
