// movba_express (include/movba.h): EXPRESS detection and descriptors - the pixel arithmetic of MOVExtractor::operator() - for the
// blocks of many frames per call, and movba_express_grid, the lattice of extract_moves.  The device passes are express.hip (one
// wavefront per item; the steps with a serial meaning: express.h); this file checks the call, packs what has to cross the bus
// into the handle's staging buffer - the pixels of the images that have items tightly, row by row without the stride's padding -
// sends it with ONE copy, queues the two launches and hands the results over after ONE synchronisation.  Result arrays that lie
// in movba_host_alloc memory are written by the kernels themselves; others arrive in the staging buffer and are copied out.
#include <cstring>

#include "express.h"
#include "handle.h"

using namespace movba;

namespace {

constexpr int64_t kExMaxPixels = 1 << 28;

// everything about a call with items that can be wrong, checked before anything is queued or written; the bytes of the images
// that have items come out of the same walk
bool ex_desc_ok(const movba_express_desc &d, const movba_express_result &r, size_t *pixel_bytes)
{
    const size_t ni = (size_t)d.n_images, n_items = (size_t)d.item_ptr[ni];
    if (!d.image || !d.rows || !d.cols || !d.stride || !d.threshold || !d.item_rect || !d.item_mode) return false;
    if (!r.code || !r.desc || !r.count || !r.n_features) return false;
    int64_t all = 0, packed = 0;
    for (size_t i = 0; i < ni; ++i) {
        if (d.rows[i] < 1 || d.cols[i] < 1 || d.stride[i] < d.cols[i]) return false;
        if (d.threshold[i] < 0 || d.threshold[i] > 255) return false;
        all += (int64_t)d.rows[i] * d.cols[i];
        if (all > kExMaxPixels) return false;
        if (d.item_ptr[i + 1] == d.item_ptr[i]) continue;
        if (!d.image[i]) return false;
        packed += (int64_t)d.rows[i] * d.cols[i];
    }
    for (size_t k = 0; k < n_items; ++k)
        if (d.item_mode[k] != MOVBA_EX_DETECT && d.item_mode[k] != MOVBA_EX_DESCRIBE) return false;
    *pixel_bytes = (size_t)packed;
    return true;
}

}  // namespace

extern "C" {

int movba_express(movba_handle *h, const movba_express_desc *desc, movba_express_result *res)
{
    if (!h || !desc || !res) return MOVBA_ERR_ARG;
    const movba_express_desc &d = *desc;
    if (d.n_images < 0 || d.n_images > MOVBA_MAX_EXPRESS_IMAGES) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    if (d.n_images == 0) { res->status = MOVBA_OK; return MOVBA_OK; }
    const size_t ni = (size_t)d.n_images;
    bool ok = d.item_ptr && d.item_ptr[0] == 0;
    for (size_t i = 0; ok && i < ni; ++i) ok = d.item_ptr[i + 1] >= d.item_ptr[i];
    if (!ok || d.item_ptr[ni] > MOVBA_MAX_EXPRESS_ITEMS) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    if (d.item_ptr[ni] == 0) { res->status = MOVBA_OK; return MOVBA_OK; }
    size_t pixel_bytes = 0;
    if (!ex_desc_ok(d, *res, &pixel_bytes)) { res->status = MOVBA_ERR_ARG; return MOVBA_ERR_ARG; }
    const size_t n_items = (size_t)d.item_ptr[ni];

    // Layout.  [0, h2d): the inputs and the zeroed counters, one H2D copy into the handle's side-call scratch; behind them in
    // the staging buffer: the results (Out: those that are staged).
    Carver c;
    In<int32_t> off, rows, cols, thr, rect, mode, image, feat;
    In<uint64_t> ref;
    In<uint8_t> pix;
    off.plan(ni, c); rows.plan(ni, c); cols.plan(ni, c); thr.plan(ni, c); feat.plan(ni, c);
    rect.plan(4 * n_items, c); mode.plan(n_items, c); image.plan(n_items, c); ref.plan(d.item_ref ? 4 * n_items : 0, c);
    pix.plan(pixel_bytes, c);
    const size_t h2d = c.off;
    Out<uint8_t> code;
    Out<uint64_t> words;
    Out<int32_t> count, dist, nfeat;
    code.plan(res->code, n_items, c); words.plan(res->desc, 4 * n_items, c); count.plan(res->count, n_items, c);
    dist.plan(res->distance, n_items, c); nfeat.plan(res->n_features, ni, c);
    const size_t total = c.off;

    res->status = MOVBA_ERR_HIP;            // (until the device work is through)
    int rc = begin_side_call(h, h2d, total); if (rc) return rc;

    char *sg = h->stage, *ar = h->pose_scratch.p;
    rows.fill(sg, d.rows); cols.fill(sg, d.cols); thr.fill(sg, d.threshold);
    rect.fill(sg, d.item_rect); mode.fill(sg, d.item_mode); ref.fill(sg, d.item_ref);
    int32_t *img_off = off.host(sg), *item_image = image.host(sg);
    uint8_t *pixels = pix.host(sg);
    std::memset(feat.host(sg), 0, sizeof(int32_t) * ni);
    size_t at = 0;
    for (size_t i = 0; i < ni; ++i) {
        img_off[i] = 0;
        if (d.item_ptr[i + 1] == d.item_ptr[i]) continue;
        img_off[i] = (int32_t)at;
        const size_t nc = (size_t)d.cols[i];
        for (size_t y = 0; y < (size_t)d.rows[i]; ++y, at += nc) std::memcpy(pixels + at, d.image[i] + y * (size_t)d.stride[i], nc);
        for (int32_t k = d.item_ptr[i]; k < d.item_ptr[i + 1]; ++k) item_image[k] = (int32_t)i;
    }

    ExDev e{};
    e.n_images = d.n_images; e.n_items = (int32_t)n_items;
    e.pixels = pix.dev(ar); e.img_off = off.dev(ar); e.rows = rows.dev(ar); e.cols = cols.dev(ar); e.threshold = thr.dev(ar);
    e.item_rect = rect.dev(ar); e.item_mode = mode.dev(ar); e.item_image = image.dev(ar); e.item_ref = ref.dev(ar);
    e.features = const_cast<int32_t *>(feat.dev(ar));
    code.bind(h->stage_dev); words.bind(h->stage_dev);
    for (Out<int32_t> *o : { &count, &dist, &nfeat }) o->bind(h->stage_dev);
    e.code = code.dev; e.desc = words.dev; e.count = count.dev; e.distance = dist.dev; e.n_features = nfeat.dev;

    HIP_TRY(hipMemcpyAsync(ar, sg, h2d, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_express(e, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));

    code.fetch(sg); words.fetch(sg);
    for (const Out<int32_t> *o : { &count, &dist, &nfeat }) o->fetch(sg);
    res->status = MOVBA_OK;
    return MOVBA_OK;
}

int movba_express_grid(int32_t rows, int32_t cols, int32_t *rects, int32_t cap)
{
    if (cap < 0 || (cap > 0 && !rects)) return MOVBA_ERR_ARG;
    if (rows <= 16 || cols <= 16) return 0;
    // y = 8, 24, ... < rows - 8
    const int64_t ny = ((int64_t)rows - 17) / 16 + 1, nx = ((int64_t)cols - 17) / 16 + 1;
    if (ny * nx > INT32_MAX) return MOVBA_ERR_ARG;
    int32_t n = 0;
    for (int64_t y = 8; y < rows - 8 && n < cap; y += 16)
        for (int64_t x = 8; x < cols - 8 && n < cap; x += 16, ++n) {
            int32_t *r = rects + 4 * (size_t)n;
            r[0] = (int32_t)(x - 8); r[1] = (int32_t)(y - 8); r[2] = 16; r[3] = 16;
        }
    return (int32_t)(ny * nx);
}

}  // extern "C"
