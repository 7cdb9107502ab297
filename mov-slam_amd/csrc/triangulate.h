// Device view + launch wrapper of movba_triangulate (triangulate.hip; host side: triangulate.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace movba {

// Everything k_triangulate reads and writes.  The inputs lie in device memory (one packed copy); points / code are device
// memory or device views of pinned host memory (the staging buffer, or the caller's movba_host_alloc arrays).
struct TriDev {
    int32_t n_matches, n_pairs;
    const double *poses, *cam;      // n_views x 7, n_views x 4
    const double *bf, *b;           // n_views each, or nullptr
    const int32_t *pair_view;       // n_pairs x 2, every index checked by the host
    const int32_t *pair_ptr;        // n_pairs + 1, ascending, [0] = 0, [n_pairs] = n_matches
    const double *obs1, *obs2;      // n_matches x 2
    const double *ur1, *ur2, *depth1, *depth2;      // n_matches each, or nullptr
    double gate, far_th;
    double *points;                 // n_matches x 3 out
    uint8_t *code;                  // n_matches out
};

constexpr int kTriThreads = 256;        // one thread per match
constexpr int kTriPairCache = 8;        // pairs whose two views a workgroup holds in LDS at a time

hipError_t launch_triangulate(const TriDev &d, hipStream_t s);

}  // namespace movba
