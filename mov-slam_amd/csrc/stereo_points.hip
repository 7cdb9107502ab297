// The kernels of movba_stereo_points (include/movba.h), two launches on one stream.
//
// k_st_frame: one workgroup of 1024 threads per frame; thread t takes points t, t + 1024, ...  In turn:
//   the gates (st_gate_point), which leave the int distance and the depth in device scratch;
//   the exact upper median of the accepted distances by a radix select - four passes of eight bits, most significant first, each
//     a 256-bin count in LDS (integer atomics: a count does not depend on its order) of the distances that carry the prefix found
//     so far, then the bin that holds the rank, which every thread finds for itself from the same bins.  Only the value is
//     observable, so nothing is sorted here: 4 reads of n ints instead of a sort of n;
//   the pruning (st_prune_point) with the counts of the points left with a depth and of those at or below th_depth;
//   the selection.  MOVBA_STEREO_SELECT_ALL: an exclusive prefix sum over contiguous chunks, so that places ascend with the
//     index.  MOVBA_STEREO_SELECT_CLOSE: the keys (st_key: the depth's bits above the index - distinct, so the method cannot
//     change the outcome) go into LDS, padded with all-ones to a power of two, a bitonic network sorts them ascending as
//     k_adv_sort does, and the first st_list_len of them are the walk.  Either way the frame's list and its length go to scratch.
//   LDS is the one dynamic block: 8 bytes x pow2ceil(the call's largest CLOSE frame), 128 KiB at the bound and never less than
//   kStMinLds; the bins and the waves' partial sums lie at its start and are dead before the keys are written.
// k_st_emit: up to 64 workgroups per frame.  The frame's start in the dense lists is the sum of the earlier frames' counts (at most
//   1024 words, which every workgroup adds up itself); sel_ptr, the rows of a share of the frame's list (st_emit_item) and a
//   share of the padding behind the total (st_pad).
// Global memory is written with ordinary vector stores; there is no floating-point atomic and no floating-point sum whose
// order could matter.
#include <hip/hip_runtime.h>

#include "stereo_points.h"

namespace movba {

namespace {

// the sum of v over the workgroup, in every thread; `part` is kStWaves words of LDS
__device__ inline int32_t st_block_sum(int32_t v, int32_t *part)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                        // (part may still be read from the sum before)
    if (lane == 0) part[wave] = v;
    __syncthreads();
    int32_t total = 0;
    for (int w = 0; w < kStWaves; ++w) total += part[w];
    return total;
}

__global__ __launch_bounds__(kStThreads) void k_st_frame(const StDev d)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char st_lds[];
    int32_t *hist = reinterpret_cast<int32_t *>(st_lds), *part = hist + 256;        // 256 + kStWaves words: within kStMinLds
    uint64_t *keys = reinterpret_cast<uint64_t *>(st_lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t f = blockIdx.x, p0 = d.pt_ptr[f], n = d.pt_ptr[f + 1] - p0;
    const StFrame &fr = d.frame[f];

    int32_t mine = 0;
    for (int32_t i = tid; i < n; i += kStThreads) {
        st_gate_point(d, fr, (size_t)p0 + i);
        mine += d.dist[p0 + i] != kStNoDist ? 1 : 0;
    }
    const int32_t n_cand = st_block_sum(mine, part);            // (its barriers also publish the scratch to the workgroup)

    int32_t median = -1;
    float th = 0.f;
    if (n_cand > 0) {                       // (the whole workgroup)
        int32_t rank = st_median_rank(n_cand);
        uint32_t prefix = 0, mask = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            __syncthreads();                // (the bins of the pass before have been read)
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int32_t i = tid; i < n; i += kStThreads) {
                const int32_t v = d.dist[p0 + i];
                if (v != kStNoDist && ((uint32_t)v & mask) == prefix) atomicAdd(&hist[((uint32_t)v >> shift) & 255], 1);
            }
            __syncthreads();
            int b = 0;
            while (b < 255 && rank >= hist[b]) rank -= hist[b++];
            prefix |= (uint32_t)b << shift;
            mask |= 0xffu << shift;
        }
        median = (int32_t)prefix;
        th = st_threshold(median);
    }

    int32_t left = 0, close = 0;
    for (int32_t i = tid; i < n; i += kStThreads) {
        const float z = st_prune_point(d, (size_t)p0 + i, th);
        if (z > 0.f) { ++left; if (z <= fr.th_depth) ++close; }
    }
    const int32_t n_stereo = st_block_sum(left, part), n_close = st_block_sum(close, part);
    if (tid == 0) { d.n_stereo[f] = n_stereo; d.median_dist[f] = median; d.th_dist[f] = th; }

    int32_t count = 0;
    if (fr.select == MOVBA_STEREO_SELECT_ALL) {
        // thread t takes the contiguous chunk [t * per, (t + 1) * per), so places ascend with the index
        const int32_t per = (n + kStThreads - 1) / kStThreads, i0 = min(tid * per, n), i1 = min(i0 + per, n);
        int32_t own = 0;
        for (int32_t i = i0; i < i1; ++i) own += d.z[p0 + i] > 0.f ? 1 : 0;
        int32_t incl = own;
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        __syncthreads();                    // (part may still be read from the sums before)
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        int32_t at = incl - own;
        for (int w = 0; w < wave; ++w) at += part[w];
        for (int32_t i = i0; i < i1; ++i)
            if (d.z[p0 + i] > 0.f) d.list[p0 + at++] = i;
        count = n_stereo;
    } else if (fr.select == MOVBA_STEREO_SELECT_CLOSE && n_stereo > 0) {
        const int32_t m = st_pow2ceil(n);   // (n <= max_close, which sized the block)
        __syncthreads();                    // (part has been read by every thread)
        for (int32_t i = tid; i < m; i += kStThreads) {
            const float z = i < n ? d.z[p0 + i] : -1.f;
            keys[i] = z > 0.f ? st_key(z, i) : ~0ull;
        }
        __syncthreads();
        for (int32_t k = 2; k <= m; k <<= 1) {
            for (int32_t j = k >> 1; j > 0; j >>= 1) {
                for (int32_t t = tid; t < (m >> 1); t += kStThreads) {
                    const int32_t a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                    const uint64_t ka = keys[a], kb = keys[b];
                    if ((ka > kb) == ((a & k) == 0)) { keys[a] = kb; keys[b] = ka; }
                }
                __syncthreads();
            }
        }
        count = st_list_len(n_stereo, n_close, d.max_point);
        for (int32_t j = tid; j < count; j += kStThreads) d.list[p0 + j] = st_key_index(keys[j]);
    }
    if (tid == 0) d.counts[f] = count;
}

__global__ __launch_bounds__(kStEmitThreads) void k_st_emit(const StDev d)
{
    __shared__ int32_t sums[2][kStEmitWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t f = blockIdx.x;
    int32_t before = 0, all = 0;
    for (int32_t i = tid; i < d.n_frames; i += kStEmitThreads) {
        const int32_t c = d.counts[i];
        all += c;
        if (i < f) before += c;
    }
    for (int o = 32; o > 0; o >>= 1) { before += __shfl_xor(before, o); all += __shfl_xor(all, o); }
    if (lane == 0) { sums[0][wave] = before; sums[1][wave] = all; }
    __syncthreads();
    before = all = 0;
    for (int w = 0; w < kStEmitWaves; ++w) { before += sums[0][w]; all += sums[1][w]; }
    const int32_t chunk = blockIdx.y, n_chunks = gridDim.y, count = d.counts[f];
    if (tid == 0 && chunk == 0) {
        d.sel_ptr[f] = before;
        if (f == d.n_frames - 1) d.sel_ptr[d.n_frames] = all;
    }
    const StFrame &fr = d.frame[f];
    const int32_t p0 = d.pt_ptr[f];
    for (int32_t j = chunk * kStEmitThreads + tid; j < count; j += n_chunks * kStEmitThreads) st_emit_item(d, fr, p0, before, j);
    const int64_t group = (int64_t)f * n_chunks + chunk, groups = (int64_t)d.n_frames * n_chunks;
    for (int64_t o = (int64_t)all + group * kStEmitThreads + tid; o < d.n_pt; o += groups * kStEmitThreads) st_pad(d, (size_t)o);
}

}  // namespace

hipError_t launch_stereo_points(const StDev &d, hipStream_t s)
{
    if (d.n_frames <= 0) return hipGetLastError();
    const size_t sort = d.max_close > 0 ? 8 * (size_t)st_pow2ceil(d.max_close) : 0, lds = sort > (size_t)kStMinLds ? sort : (size_t)kStMinLds;
    // (above the 64 KB a kernel may ask for unannounced; per device, so said where it is needed rather than once per process)
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_st_frame), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * MOVBA_MAX_STEREO_POINTS);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_st_frame, dim3(d.n_frames), dim3(kStThreads), lds, s, d);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (workgroups per frame: by the LARGEST frame, so that neither a call of one frame nor one large frame among many tiny ones is
    // one workgroup's work; a workgroup whose share of its frame's list is empty only pads)
    // - but no more than 8192 workgroups in all: each adds up the frames' counts for itself
    const int chunks = std::min(std::min(kStEmitChunks, std::max(1, 8192 / d.n_frames)), std::max(1, (d.max_frame + kStEmitThreads - 1) / kStEmitThreads));
    hipLaunchKernelGGL(k_st_emit, dim3(d.n_frames, chunks), dim3(kStEmitThreads), 0, s, d);
    return hipGetLastError();
}

}  // namespace movba
