// cv2.SIFT_create(nfeatures=0, contrastThreshold=, edgeThreshold=).detectAndCompute(img_u8, None) of the global align step
// (karios/matcher/global_align.py:48-50, 160-166).  tests/sift_restatement.py is the definition; the kernels live in k_sift.hip.
//
// The call works octave by octave: the octave's Gaussian and DoG levels are built, scanned for extrema, the candidates refined,
// given their orientations and described while those levels are still there; the next octave starts from this one's level
// nOctaveLayers.  The host reads three counters per octave (candidates, refined, key points) to size the next launch.  At the end
// the key-point records travel to the host once, are ordered and deduplicated there (sift_order.hpp: a radix sort on (x, y), then
// sf::key_less within the runs of one point), and a gather kernel writes the outputs in that order.
//
// Workspace: 2 n + 6 planes of the doubled image (n + 3 Gaussian levels, n + 2 DoG levels, the row pass of the blur) - 12 planes
// for the default n = 3, 23.1 GB at 10980 x 10980 - plus the lists (23.7 GB with them on the 3.2 M key points of DESIGN section
// 12.4).  A call whose planes exceed 1 GB retires them when it returns, with an error too: they are freed at the context's next
// flush, so the next call allocates its own while the old ones still stand (twice the planes for a moment).
#include "api_internal.hpp"
#include "k_sift.hpp"
#include "sift_order.hpp"

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

namespace {

// counts: per octave candidates, refined, key points.  Times in microseconds: device time between stream events for the stages
// (per octave: blur + DoG, scan, refine, orient, describe), host time for the final order and for the whole call.
enum { ST_OCTAVES = 0, ST_BEFORE, ST_AFTER, ST_WS_BYTES, ST_PER_OCTAVE, ST_US_BASE = 52, ST_US_SORT, ST_US_GATHER, ST_US_CALL, ST_US_PER_OCTAVE,
       ST_REGROW_CAND = 136, ST_REGROW_KP, ST_WORDS = 160 };   // how often a list was too small and its stage ran again
enum { SG_BLUR = 0, SG_SCAN, SG_REFINE, SG_ORIENT, SG_DESCRIBE, SG_COUNT };
const size_t RETIRE_ABOVE = (size_t)1 << 30;

struct sift_out {
    float *x, *y, *size, *angle, *response;
    int *octave;
    void *desc;
    int desc_dtype;
    ptrdiff_t desc_stride;
};

int sift_args(km_ctx *c, const void *img, int H, int W, ptrdiff_t stride, int nfeatures, int n_layers, double contrast, double edge, double sigma, int cap,
              const sift_out &o, const int *count)
{
    if (nfeatures != 0) return km_fail(c, KM_E_UNSUPPORTED, "sift_detect_and_compute: nfeatures = %d (only 0, every key point, is supported)", nfeatures);
    if (!img || !count) return km_fail(c, KM_E_ARG, "sift_detect_and_compute: null argument");
    if (H < 1 || W < 1 || stride < W) return km_fail(c, KM_E_ARG, "sift_detect_and_compute: image %d x %d, row stride %td", H, W, stride);
    if (H > 32767 || W > 32767) return km_fail(c, KM_E_UNSUPPORTED, "sift_detect_and_compute: image %d x %d (at most 32767 a side)", H, W);
    if (n_layers < 1 || n_layers > 8) return km_fail(c, KM_E_ARG, "sift_detect_and_compute: n_octave_layers = %d (1 .. 8)", n_layers);
    if (!(contrast >= 0) || !(edge > 0) || !(sigma > 0))
        return km_fail(c, KM_E_ARG, "sift_detect_and_compute: contrast_threshold %g, edge_threshold %g, sigma %g", contrast, edge, sigma);
    if (o.desc_dtype != KM_U8 && o.desc_dtype != KM_F32) return km_fail(c, KM_E_ARG, "sift_detect_and_compute: descriptor dtype %d (uint8 or float32)", o.desc_dtype);
    if (cap < 0 || (cap > 0 && (!o.x || !o.y || !o.size || !o.angle || !o.response || !o.octave || !o.desc || o.desc_stride < sf::D_LEN)))
        return km_fail(c, KM_E_ARG, "sift_detect_and_compute: bad output arguments");
    return KM_OK;
}

int make_taps(km_ctx *c, double sigma, ksf_taps *t)
{
    float full[2 * sf::MAX_RADIUS + 1];
    const int n = sf::gaussian_kernel(sigma, full, 2 * sf::MAX_RADIUS + 1);
    if (n == 0) return km_fail(c, KM_E_UNSUPPORTED, "sift_detect_and_compute: the Gaussian kernel of sigma %g is wider than %d taps", sigma, 2 * sf::MAX_RADIUS + 1);
    t->radius = n / 2;
    for (int j = 0; j <= sf::MAX_RADIUS; j++) t->k[j] = j <= t->radius ? full[t->radius + j] : 0.f;
    return KM_OK;
}

// a list that keeps its first `used` bytes when it grows (the old buffer is retired, so it is still there to copy from)
void *grow_keep(km_ctx *c, int slot, size_t used, size_t bytes)
{
    void *old = km_ws_peek(c, slot);
    void *p = km_ws(c, slot, bytes);
    if (p && old && p != old && used)
        if (hipMemcpyAsync(p, old, used, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) { km_fail(c, KM_E_HIP, "sift: copy of a grown list"); return nullptr; }
    return p;
}

void retire_slot(km_ctx *c, int slot)
{
    km_dev_mem &b = c->lane ? c->ws_b[slot] : c->ws[slot];
    if (b.p) c->retired.push_back(std::move(b));
}

// Stage times without a synchronisation of their own: an event on the stream where a stage begins; the time between two neighbours
// is credited to the earlier one's word of the stats.  Only kept when the caller asked for stats.
struct stage_clock {
    std::vector<std::pair<int, km_event_h>> marks;
    bool on = false;
    void mark(km_ctx *c, int word)
    {
        if (!on) return;
        km_event_h e;
        if (e.create(0) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(e, c->stream);
        marks.emplace_back(word, std::move(e));
    }
    void read(int64_t *st)          // after the stream has been synchronised
    {
        for (size_t i = 0; on && i + 1 < marks.size(); i++) {
            float ms = 0;
            if (marks[i].first >= 0 && hipEventElapsedTime(&ms, marks[i].second, marks[i + 1].second) == hipSuccess)
                st[marks[i].first] += (int64_t)(ms * 1000.f + 0.5f);
        }
    }
};
double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int read_counter(km_ctx *c, const unsigned *d, unsigned *h)
{
    KM_D2H(c, h, d, sizeof(unsigned));
    KM_FLUSH(c);
    return KM_OK;
}

// d_img on the device; the outputs on the device with room for `cap` key points.  *count: the true number, always.
int sift_dev(km_ctx *c, const uint8_t *d_img, int H, int W, ptrdiff_t stride, int n_layers, double contrast, double edge, double sigma, int cap,
             const sift_out &o, int *count, int64_t *stats)
{
    int rc;
    int64_t st[ST_WORDS] = {0};
    const double t_call = now_us();
    stage_clock clock;
    clock.on = stats != nullptr;
    *count = 0;
    const int h0 = 2 * H, w0 = 2 * W;
    const int n_oct = sf::n_octaves(h0, w0);
    st[ST_OCTAVES] = n_oct;
    if (stats) memcpy(stats, st, sizeof st);
    if (n_oct == 0) return KM_OK;

    const int n_gauss = n_layers + 3, n_dog = n_layers + 2;
    const size_t plane0 = (size_t)h0 * w0;
    const size_t plane_bytes = plane0 * sizeof(float) * (size_t)(n_gauss + n_dog + 1);
    float *gauss = (float *)km_ws(c, WS_SF_GAUSS, plane0 * sizeof(float) * n_gauss);
    float *dog = (float *)km_ws(c, WS_SF_DOG, plane0 * sizeof(float) * n_dog);
    float *tmp = (float *)km_ws(c, WS_SF_TMP, plane0 * sizeof(float));
    unsigned *counters = (unsigned *)km_ws(c, WS_SF_STATE, 3 * sf::MAX_OCTAVES * sizeof(unsigned));
    struct plane_guard {      // on every way out
        km_ctx *c;
        bool big;
        ~plane_guard() { if (big) { retire_slot(c, WS_SF_GAUSS); retire_slot(c, WS_SF_DOG); retire_slot(c, WS_SF_TMP); } }
    } guard = {c, plane_bytes > RETIRE_ABOVE};
    if (!gauss || !dog || !tmp || !counters) return KM_E_NOMEM;
    KM_HIP(c, hipMemsetAsync(counters, 0, 3 * sf::MAX_OCTAVES * sizeof(unsigned), c->stream));
    size_t list_bytes = 0;

    std::vector<ksf_taps> taps((size_t)n_gauss);
    if ((rc = make_taps(c, (double)sf::base_sigma(sigma), &taps[0]))) return rc;
    for (int i = 1; i < n_gauss; i++)
        if ((rc = make_taps(c, sf::level_sigma(sigma, n_layers, i), &taps[(size_t)i]))) return rc;
    const float threshold = (float)(int)(0.5 * contrast / n_layers * 255);   // floor of a value >= 0

    // the base: the doubled image into level 1's place, blurred into level 0
    clock.mark(c, ST_US_BASE);
    if ((rc = ksf_base(c, d_img, H, W, stride, gauss + plane0)) || (rc = ksf_blur(c, gauss + plane0, h0, w0, taps[0], tmp, gauss, nullptr))) return rc;

    size_t total = 0;      // key points of the octaves so far
    sf::Key *kp = nullptr;
    uint8_t *desc = nullptr;
    int h = h0, w = w0;
    for (int o = 0; o < n_oct; o++) {
        const size_t plane = (size_t)h * w;
        // level 0 of this octave sits at `gauss` (the base, or the decimated level n_layers of the octave before: written below)
        const int us = ST_US_PER_OCTAVE + SG_COUNT * o;
        clock.mark(c, us + SG_BLUR);
        for (int i = 1; i < n_gauss; i++)
            if ((rc = ksf_blur(c, gauss + (size_t)(i - 1) * plane, h, w, taps[(size_t)i], tmp, gauss + (size_t)i * plane, dog + (size_t)(i - 1) * plane))) return rc;
        unsigned *cnt = counters + 3 * o;
        unsigned n_cand = 0, n_ref = 0, n_kp = 0;
        clock.mark(c, us + SG_SCAN);
        if (h > 2 * sf::BORDER && w > 2 * sf::BORDER) {
            // a CLAHE'd texture at 10980 x 10980 has 0.19 % of (samples x layers) in octave 0 (profiles/sift_probe.json); 0.4 % of room,
            // and the scan runs again when a dense pattern needs more
            size_t cand_cap = std::max<size_t>(256, plane * (size_t)n_layers / 256);
            for (int attempt = 0;; attempt++) {
                ksf_cand *cand = (ksf_cand *)km_ws(c, WS_SF_CAND, cand_cap * sizeof(ksf_cand));
                if (!cand) return KM_E_NOMEM;
                if ((rc = ksf_scan(c, dog, plane, h, w, n_layers, threshold, cand, (unsigned)std::min<size_t>(cand_cap, 0xffffffffu), cnt)) ||
                    (rc = read_counter(c, cnt, &n_cand)))
                    return rc;
                if (n_cand <= cand_cap) break;
                if (attempt == 1) return km_fail(c, KM_E_INTERNAL, "sift_detect_and_compute: the candidate list kept overflowing");
                st[ST_REGROW_CAND]++;
                cand_cap = n_cand;                               // every sample of a tie-heavy image can be a candidate: scan again with room
                KM_HIP(c, hipMemsetAsync(cnt, 0, sizeof(unsigned), c->stream));
            }
            list_bytes = std::max(list_bytes, cand_cap * sizeof(ksf_cand));
        }
        if (n_cand) {
            const ksf_cand *cand = (const ksf_cand *)km_ws_peek(c, WS_SF_CAND);
            sf::Refined *refined = (sf::Refined *)km_ws(c, WS_SF_REFINED, (size_t)n_cand * sizeof(sf::Refined));
            if (!refined) return KM_E_NOMEM;
            clock.mark(c, us + SG_REFINE);
            if ((rc = ksf_refine(c, dog, plane, h, w, o, cand, n_cand, n_layers, contrast, edge, sigma, refined, cnt + 1)) ||
                (rc = read_counter(c, cnt + 1, &n_ref)))
                return rc;
            if (n_ref) {
                size_t room = (size_t)n_ref * 2 + 64;
                clock.mark(c, us + SG_ORIENT);
                for (int attempt = 0;; attempt++) {
                    kp = (sf::Key *)grow_keep(c, WS_SF_KP, total * sizeof(sf::Key), (total + room) * sizeof(sf::Key));
                    if (!kp) return KM_E_NOMEM;
                    if ((rc = ksf_orient(c, gauss, plane, h, w, o, refined, n_ref, kp + total, (unsigned)room, cnt + 2)) ||
                        (rc = read_counter(c, cnt + 2, &n_kp)))
                        return rc;
                    if (n_kp <= room) break;
                    if (attempt == 1) return km_fail(c, KM_E_INTERNAL, "sift_detect_and_compute: the key-point list kept overflowing");
                    st[ST_REGROW_KP]++;
                    room = n_kp;
                    KM_HIP(c, hipMemsetAsync(cnt + 2, 0, sizeof(unsigned), c->stream));
                }
                if (n_kp) {
                    desc = (uint8_t *)grow_keep(c, WS_SF_DESC, total * sf::D_LEN, (total + n_kp) * sf::D_LEN);
                    if (!desc) return KM_E_NOMEM;
                    clock.mark(c, us + SG_DESCRIBE);
                    if ((rc = ksf_describe(c, gauss, plane, h, w, o, kp + total, n_kp, desc + total * sf::D_LEN))) return rc;
                }
            }
        }
        st[ST_PER_OCTAVE + 3 * o] = n_cand; st[ST_PER_OCTAVE + 3 * o + 1] = n_ref; st[ST_PER_OCTAVE + 3 * o + 2] = n_kp;
        total += n_kp;
        clock.mark(c, us + SG_BLUR);      // the decimation counts as the octave's dense part
        if (o + 1 < n_oct) {
            // level n_layers, every second sample, becomes level 0 of the next octave (a quarter plane at the front of level 0's
            // place: the two do not overlap)
            if ((rc = ksf_decimate(c, gauss + (size_t)n_layers * plane, h, w, gauss))) return rc;
            h /= 2; w /= 2;
        }
    }
    st[ST_BEFORE] = (int64_t)total;
    if (total > 0x7fffffffu) return km_fail(c, KM_E_UNSUPPORTED, "sift_detect_and_compute: %zu key points", total);

    // the final order on the host, the gather on the device
    std::vector<int> perm;
    clock.mark(c, -1);
    if (total) {
        std::vector<sf::Key> keys(total);
        KM_D2H(c, keys.data(), kp, total * sizeof(sf::Key));
        KM_FLUSH(c);
        const double t_sort = now_us();
        sf::final_order(keys.data(), total, perm);
        st[ST_US_SORT] = (int64_t)(now_us() - t_sort);
    }
    const size_t n_out = perm.size();
    st[ST_AFTER] = (int64_t)n_out;
    *count = (int)n_out;
    const size_t n_write = std::min<size_t>(n_out, (size_t)cap);
    clock.mark(c, ST_US_GATHER);
    if (n_write) {
        int *d_perm = (int *)km_ws(c, WS_SF_PERM, n_write * sizeof(int));
        if (!d_perm) return KM_E_NOMEM;
        if ((rc = km_h2d_staged(c, c->stream, d_perm, n_write * sizeof(int), perm.data(), n_write * sizeof(int), n_write * sizeof(int), 1)) ||
            (rc = ksf_gather(c, kp, desc, d_perm, (int)n_write, o.x, o.y, o.size, o.angle, o.response, o.octave, o.desc, o.desc_dtype, o.desc_stride)))
            return rc;
    }
    clock.mark(c, -1);
    KM_HIP(c, hipStreamSynchronize(c->stream));
    clock.read(st);
    st[ST_US_CALL] = (int64_t)(now_us() - t_call);
    st[ST_WS_BYTES] = (int64_t)(plane_bytes + list_bytes + total * (sizeof(sf::Key) + sf::D_LEN));
    if (stats) memcpy(stats, st, sizeof st);
    if (n_out > (size_t)cap)
        return km_fail(c, KM_E_CAPACITY, "sift_detect_and_compute: %zu key points, room for %d (the first %d are written)", n_out, cap, cap);
    return KM_OK;
}

}  // namespace

extern "C" {

int km_sift_detect_and_compute_dev(km_ctx *c, const uint8_t *d_img, int H, int W, ptrdiff_t stride, int nfeatures, int n_octave_layers,
                                   double contrast_threshold, double edge_threshold, double sigma, int cap, float *d_x, float *d_y, float *d_size,
                                   float *d_angle, float *d_response, int *d_octave, void *d_desc, int desc_dtype, ptrdiff_t desc_stride, int *count,
                                   int64_t *stats)
{
    int rc;
    const sift_out o = {d_x, d_y, d_size, d_angle, d_response, d_octave, d_desc, desc_dtype, desc_stride};
    if ((rc = begin_call(c)) || (rc = sift_args(c, d_img, H, W, stride, nfeatures, n_octave_layers, contrast_threshold, edge_threshold, sigma, cap, o, count)))
        return rc;
    try {
        return sift_dev(c, d_img, H, W, stride, n_octave_layers, contrast_threshold, edge_threshold, sigma, cap, o, count, stats);
    } catch (const std::bad_alloc &) {   // the host copies of the key points: nothing throws across the boundary
        return km_fail(c, KM_E_NOMEM, "sift_detect_and_compute: no host memory for the key points");
    }
}

int km_sift_detect_and_compute(km_ctx *c, const uint8_t *img, int H, int W, ptrdiff_t stride, int nfeatures, int n_octave_layers, double contrast_threshold,
                               double edge_threshold, double sigma, int cap, float *x, float *y, float *size, float *angle, float *response, int *octave,
                               void *desc, int desc_dtype, ptrdiff_t desc_stride, int *count, int64_t *stats)
{
    int rc;
    const sift_out o = {x, y, size, angle, response, octave, desc, desc_dtype, desc_stride};
    if ((rc = begin_call(c)) || (rc = sift_args(c, img, H, W, stride, nfeatures, n_octave_layers, contrast_threshold, edge_threshold, sigma, cap, o, count)))
        return rc;
    if (cap > 0 && desc_stride != sf::D_LEN) return km_fail(c, KM_E_ARG, "sift_detect_and_compute: the host form writes dense descriptor rows (stride %d)", (int)sf::D_LEN);
    void *d_img;
    const size_t elem = km_dtype_size(desc_dtype), room = (size_t)cap;
    // device outputs: six field arrays of `cap` words, then `cap` dense descriptor rows
    char *d_out = (char *)km_ws(c, WS_SF_OUT, room * (6 * 4 + sf::D_LEN * elem) + 16);
    if (!d_out) return KM_E_NOMEM;
    if ((rc = upload_image(c, WS_RAW_A, img, 1, H, W, stride, &d_img))) return rc;
    float *f = (float *)d_out;
    const sift_out d = {f, f + room, f + 2 * room, f + 3 * room, f + 4 * room, (int *)(f + 5 * room), f + 6 * room, desc_dtype, sf::D_LEN};
    try {
        rc = sift_dev(c, (const uint8_t *)d_img, H, W, W, n_octave_layers, contrast_threshold, edge_threshold, sigma, cap, d, count, stats);
    } catch (const std::bad_alloc &) {
        return km_fail(c, KM_E_NOMEM, "sift_detect_and_compute: no host memory for the key points");
    }
    if (rc != KM_OK && rc != KM_E_CAPACITY) return rc;
    const size_t n = std::min<size_t>((size_t)*count, room);
    if (n) {
        KM_D2H(c, x, d.x, n * 4); KM_D2H(c, y, d.y, n * 4); KM_D2H(c, size, d.size, n * 4); KM_D2H(c, angle, d.angle, n * 4);
        KM_D2H(c, response, d.response, n * 4); KM_D2H(c, octave, d.octave, n * 4);
        KM_D2H(c, desc, d.desc, n * sf::D_LEN * elem);
        KM_FLUSH(c);
    }
    return rc;
}

}  // extern "C"
