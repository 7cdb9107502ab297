// The fake device's side of movba_express (mov-slam_amd/csrc/express.cpp): the launch wrapper of express.h as a closure on the
// fake stream (tests/hipstub/fake_hip.cpp), and nothing else.  It runs the library's own steps (express.h: ex_item item by item,
// then ex_counts, serially, in the kernels' order), reading every input through the pointers the host laid out - checking every
// index on the way, so that an array the host packed wrongly is reported rather than followed - and writing results where the
// host said: the sanitizers see the host's layout and hand-offs, and the driver can check the values that come back.  Test
// infrastructure only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <vector>

#include "express.h"
#include "movba.h"

namespace {
std::atomic<int> g_ex_errors{0};

void bad(const char *what)
{
    std::fprintf(stderr, "fake_express: %s\n", what);
    g_ex_errors.fetch_add(1);
}
}  // namespace

extern "C" int fake_express_errors() { return g_ex_errors.load(); }

namespace movba {

hipError_t launch_express(const ExDev &dev, hipStream_t s)
{
    const ExDev d = dev;
    fake_enqueue(s, [=] {
        if (d.n_items <= 0 || d.n_images <= 0) return;
        if (!d.pixels || !d.img_off || !d.rows || !d.cols || !d.threshold || !d.item_rect || !d.item_mode || !d.item_image || !d.features) { bad("an input is missing"); return; }
        if (!d.code || !d.desc || !d.count || !d.n_features) { bad("an output is missing"); return; }
        std::vector<char> has((size_t)d.n_images, 0);
        int32_t last = 0;
        for (int32_t k = 0; k < d.n_items; ++k) {
            const int32_t im = d.item_image[k];
            if (im < last || im >= d.n_images) { bad("an item's image is no image, or the items are not in image order"); return; }
            if (d.item_mode[k] != MOVBA_EX_DETECT && d.item_mode[k] != MOVBA_EX_DESCRIBE) { bad("an unknown mode"); return; }
            last = im;
            has[(size_t)im] = 1;
        }
        int64_t end = 0;
        for (int32_t i = 0; i < d.n_images; ++i) {
            if (d.rows[i] < 1 || d.cols[i] < 1 || d.threshold[i] < 0 || d.threshold[i] > 255) { bad("an image's record is out of range"); return; }
            if (d.features[i] != 0) { bad("a counter does not arrive zeroed"); return; }
            if (!has[(size_t)i]) continue;
            if (d.img_off[i] != end) { bad("the images that have items do not lie tightly, one behind the other"); return; }
            end += (int64_t)d.rows[i] * d.cols[i];
        }
        for (int32_t k = 0; k < d.n_items; ++k) ex_item(d, k);
        ex_counts(d);
    });
    return hipSuccess;
}

}  // namespace movba
