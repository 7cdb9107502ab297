// Clock stamps of the diagnostic build (-DMOVBA_CLOCK_STAMP, scripts/build_variant.sh): the one way a kernel takes a stamp and the
// one bounded place a stamp goes.  This is the only device-side file that tests the define: the kernel files call the macros
// below, which expand to nothing in the product build, where this file declares nothing at all.
//
// Two primitives.
//   A RECORD is eight words in registers.  Its readings are of the 100 MHz clock, taken behind s_waitcnt vmcnt(0) lgkmcnt(0)
//   (STAMP_READ) or bare (STAMP_TICKS); STAMP_WORD fills in what else the record carries, word 7 is its valid mark.  It is
//   stored once per workgroup or wave (STAMP_STORE), and only by the launch the gate lets through (STAMP_GATE: the launch that
//   finds Ctrl::n_solves == kStampSolve).
//   A SEGMENT is the shader-cycle delta since the previous stamp of its set, accumulated in registers under a name
//   (STAMP_SEG; STAMP_SEG_BEHIND stands behind a value of the dependency chain: stamps are scalar instructions, the chain is
//   vector ones).  A set is declared (STAMP_SEGMENTS), started where its first segment begins (STAMP_SEG_START) and added
//   to its slots of the buffer once, at the end (STAMP_SEG_FLUSH).  Every segment reads the clock the same way, s_memtime
//   behind a compiler barrier (the phase stamps of k_pcg_rows' setup, k_band and the coarse builder used the bare builtin and
//   added to memory at every stamp until they were folded into this one: their figures are not those of the r05 logs to the
//   cycle, profiles/clock_stamp_refactor.json).
// Beside them STAMP_SPAN: one stretch of a kernel in both clocks (k_pcg_rows' "cycles in ticks" line), no record, no set.
// Both leave through StampBuf, the tail of DevWindow and of PoseDev: the handle's stamp buffer (api.cpp) with its capacities.
// stamp_store and stamp_add refuse what lies beyond them; the capacities follow the launch grids, so that is a guard and not
// the normal path.
#pragma once

#ifndef MOVBA_CLOCK_STAMP

#define STAMP_RECORD(st) do { } while (0)
#define STAMP_GATE(st, ctrl) do { } while (0)
#define STAMP_TICKS(st, k) do { } while (0)
#define STAMP_READ(st, k) do { } while (0)
#define STAMP_WORD(st, k, value) do { } while (0)
#define STAMP_STORE(st, buf, cls, idx, who) do { } while (0)
#define STAMP_SEGMENTS(sg, n) do { } while (0)
#define STAMP_SEG_START(sg) do { } while (0)
#define STAMP_SEG(sg, k) do { } while (0)
#define STAMP_SEG_START_BEHIND(sg, dep, when) do { } while (0)
#define STAMP_SEG_BEHIND(sg, k, dep, when) do { } while (0)
#define STAMP_SEG_FLUSH(sg, n, buf, slot0, who) do { } while (0)
#define STAMP_SPAN(sp) do { } while (0)
#define STAMP_SPAN_END(sp, buf, slot_cycles, slot_ticks, who) do { } while (0)
#define STAMP_HOST(call) do { } while (0)

#else

#include <hip/hip_runtime.h>

#include <cstdint>

struct movba_handle;

namespace movba {

struct PoseDev;

constexpr int kStampSolve = 3;          // the launch whose records are kept: the one that finds Ctrl::n_solves == 3
enum { kStampPoint = 0, kStampSchur = 1, kStampClasses = 2 };      // record classes: back-substitution pass (per workgroup), k_schur (per wave)
constexpr int kStampSegments = kStampClasses;       // movba_stamp_records only: the segment slots, read out eight to a record
// segment slots of a window: k_pcg_rows' shader cycles and 10 ns ticks, its per-iteration segments (wave 0), the phases of a
// launch (k_pcg_rows' setup 6 7 0 1, the coarse builder 2 - 5; k_band 0 1 2 4 5), the per-iteration segments by wave (k_band:
// the fine stamps of one block step in wave 0's row)
enum { kSegCycles = 0, kSegTicks = 1, kSegIter = 2, kSegPhase = 10, kSegWave = 18, kSegSlots = 88 };
constexpr int kPoseSegSlots = 8;        // k_pose_opt, slots 0 - 3: system pass, reduction of 28, solve + update, cost pass + reduction

// n_seg accumulators, then the records of class 0, then those of class 1 (eight words each)
struct StampBuf {
    unsigned long long *words;
    int32_t n_seg, n_rec[kStampClasses], pad_s;
};

#ifdef __HIPCC__
__device__ __forceinline__ unsigned long long stamp_ticks() { return __builtin_amdgcn_s_memrealtime(); }
__device__ __forceinline__ unsigned long long stamp_ticks_drained()
{
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    return __builtin_amdgcn_s_memrealtime();
}
__device__ __forceinline__ unsigned long long stamp_cycles()
{
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    return t;
}
__device__ __forceinline__ unsigned long long stamp_cycles_behind(double dep)
{
    const int d = __builtin_amdgcn_readfirstlane(__double2loint(dep));
    unsigned long long t;
    asm volatile("s_nop 7\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "s"(d) : "memory");
    return t;
}
// where the wave runs: HW_ID in bits 0 - 31, XCC_ID from bit 32
__device__ __forceinline__ unsigned long long stamp_hw_id()
{
    return (unsigned long long)__builtin_amdgcn_s_getreg(63492) | ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32);
}
// (a zero is not added: sets share their slots across workgroups, each adding what it stamped itself)
__device__ __forceinline__ void stamp_add(const StampBuf &b, int slot, unsigned long long v)
{
    if (v != 0 && slot >= 0 && slot < b.n_seg) b.words[slot] += v;
}
__device__ __forceinline__ void stamp_store(const StampBuf &b, int cls, long idx, const unsigned long long (&rec)[8])
{
    if (idx < 0 || idx >= b.n_rec[cls]) return;
    unsigned long long *dst = b.words + b.n_seg + 8 * ((size_t)(cls == kStampSchur ? b.n_rec[kStampPoint] : 0) + (size_t)idx);
    for (int k = 0; k < 8; ++k) dst[k] = rec[k];
}
#endif

// host side (api.cpp, one block): the buffer of a window (sized by its launch grids, zeroed) / of a pose call, and the report
// lines behind a run's final synchronisation
int stamp_window(movba_handle *h);
int stamp_pose(movba_handle *h, PoseDev &p);
void stamp_report_run(movba_handle *h);
void stamp_report_pose(movba_handle *h, int lm_iters);

}  // namespace movba

#define STAMP_RECORD(st) unsigned long long st[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }; st[0] = movba::stamp_ticks()
#define STAMP_GATE(st, ctrl) const bool st##_on = (ctrl)->n_solves == movba::kStampSolve
#define STAMP_TICKS(st, k) do { st[k] = movba::stamp_ticks(); } while (0)
#define STAMP_READ(st, k) do { st[k] = movba::stamp_ticks_drained(); } while (0)
#define STAMP_WORD(st, k, value) do { st[k] = (unsigned long long)(value); } while (0)
#define STAMP_STORE(st, buf, cls, idx, who) do { if ((who) && st##_on) movba::stamp_store(buf, cls, (long)(idx), st); } while (0)
#define STAMP_SEGMENTS(sg, n) unsigned long long sg[n] = {}, sg##_last = 0
#define STAMP_SEG_START(sg) do { sg##_last = movba::stamp_cycles(); } while (0)
#define STAMP_SEG(sg, k) do { const unsigned long long t_ = movba::stamp_cycles(); sg[k] += t_ - sg##_last; sg##_last = t_; } while (0)
#define STAMP_SEG_START_BEHIND(sg, dep, when) do { if (when) sg##_last = movba::stamp_cycles_behind(dep); } while (0)
#define STAMP_SEG_BEHIND(sg, k, dep, when) do { if (when) { const unsigned long long t_ = movba::stamp_cycles_behind(dep); sg[k] += t_ - sg##_last; sg##_last = t_; } } while (0)
#define STAMP_SEG_FLUSH(sg, n, buf, slot0, who) do { if (who) for (int k_ = 0; k_ < (n); ++k_) movba::stamp_add(buf, (slot0) + k_, sg[k_]); } while (0)
#define STAMP_SPAN(sp) const unsigned long long sp##_c0 = movba::stamp_cycles(), sp##_t0 = movba::stamp_ticks()
#define STAMP_SPAN_END(sp, buf, slot_cycles, slot_ticks, who) \
    do { if (who) { movba::stamp_add(buf, slot_cycles, movba::stamp_cycles() - sp##_c0); movba::stamp_add(buf, slot_ticks, movba::stamp_ticks() - sp##_t0); } } while (0)
#define STAMP_HOST(call) do { call; } while (0)

#endif
