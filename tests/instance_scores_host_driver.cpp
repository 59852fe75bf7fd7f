// Host-side checks of pc_frame_probs and pc_instance_scores without a GPU, linked against the AddressSanitizer + UBSan build of the library
// (`make -C pi-consistency-activity-detection_amd/csrc asan/instance_scores_host_driver`): every call returns through the entry's own argument
// checks, in front of any HIP call, so undefined behaviour on the host side (the frame-size, frame-range and crop arithmetic at the ends of
// int) ends the process with a sanitizer report.  tests/test_instance_scores_cpu.py builds and runs it.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "picons.h"

static int fails = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { ++fails; std::printf("FAILED %s:%d  %s  [%s]\n", __FILE__, __LINE__, #cond, pc_last_error()); } \
    } while (0)
#define REFUSED(call, word) EXPECT((call) == PC_E_ARG && std::strstr(pc_last_error(), word))

int main() {
    EXPECT(pc_version() == PC_VERSION && PC_VERSION >= 107);
    EXPECT(PC_PROB_ONE == 65535 && PC_SCORE_WORDS == 3);
    alignas(16) static char dummy[256];
    const float* lg = reinterpret_cast<const float*>(dummy);
    uint16_t* pb = reinterpret_cast<uint16_t*>(dummy);
    uint16_t* pb_odd = reinterpret_cast<uint16_t*>(dummy + 1);
    const int32_t views[6] = {0, 0, 0, 4, 8, 1}, starts[2] = {0, 1};

    // pc_frame_probs(logits, F, H, W, S, views, V, view_stride, starts, n, f_skip, prob, s): frames of 12 x 16, crops of 8
    REFUSED(pc_frame_probs(nullptr, 20, 12, 16, 8, views, 2, 2, starts, 2, 2, pb, nullptr), "null");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, nullptr, 2, 2, starts, 2, 2, pb, nullptr), "null");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, views, 2, 2, nullptr, 2, 2, pb, nullptr), "null");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, views, 2, 2, starts, 2, 2, nullptr, nullptr), "null");
    REFUSED(pc_frame_probs(lg, 0, 12, 16, 8, views, 2, 2, starts, 2, 2, pb, nullptr), "outside");
    REFUSED(pc_frame_probs(lg, 20, 0, 16, 8, views, 2, 2, starts, 2, 2, pb, nullptr), "outside");
    REFUSED(pc_frame_probs(lg, 20, 12, INT_MIN, 8, views, 2, 2, starts, 2, 2, pb, nullptr), "outside");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 0, views, 2, 2, starts, 2, 2, pb, nullptr), "outside");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 16, views, 2, 2, starts, 2, 2, pb, nullptr), "outside");          // S > H
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 32772, views, 2, 2, starts, 2, 2, pb, nullptr), "outside");
    REFUSED(pc_frame_probs(lg, 20, 65536, 32768, 8, views, 2, 2, starts, 2, 2, pb, nullptr), "2^31");
    REFUSED(pc_frame_probs(lg, 20, INT_MAX, INT_MAX, 8, views, 2, 2, starts, 2, 2, pb, nullptr), "2^31");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 6, views, 2, 2, starts, 2, 2, pb, nullptr), "multiple of 4");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, views, 0, 2, starts, 2, 2, pb, nullptr), "V =");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, views, 33, 2, starts, 2, 2, pb, nullptr), "V =");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, views, 2, 2, starts, 0, 2, pb, nullptr), "n =");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, views, 2, 33, starts, 33, 2, pb, nullptr), "n =");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, views, 2, 1, starts, 2, 2, pb, nullptr), "view_stride");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, views, 2, INT_MIN, starts, 2, 2, pb, nullptr), "view_stride");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, views, 2, 2, starts, 2, 0, pb, nullptr), "f_skip");
    REFUSED(pc_frame_probs(reinterpret_cast<const float*>(dummy + 4), 20, 12, 16, 8, views, 2, 2, starts, 2, 2, pb, nullptr), "16-byte");
    REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, views, 2, 2, starts, 2, 2, pb_odd, nullptr), "2-byte");
    {
        const int32_t low[6] = {0, 0, 0, 5, 8, 0}, neg[6] = {0, -1, 0, 4, 8, 1}, far[6] = {0, 0, 0, INT_MAX, 8, 0}, fl[6] = {0, 0, 2, 4, 8, 1};
        REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, low, 2, 2, starts, 2, 2, pb, nullptr), "view 1");        // 5 + 8 > 12
        REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, neg, 2, 2, starts, 2, 2, pb, nullptr), "view 0");
        REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, far, 2, 2, starts, 2, 2, pb, nullptr), "view 1");        // h0 + S beyond int32
        REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, fl, 2, 2, starts, 2, 2, pb, nullptr), "flip");
        const int32_t bad_start[2] = {0, -1};
        REFUSED(pc_frame_probs(lg, 20, 12, 16, 8, views, 2, 2, bad_start, 2, 2, pb, nullptr), "negative");
    }
    // the checks come in the documented order: with everything wrong, the null pointer is named
    REFUSED(pc_frame_probs(nullptr, 0, 0, 0, 3, nullptr, 0, 0, nullptr, 0, 0, nullptr, nullptr), "null");

    // pc_instance_scores(imap, prob, F, H, W, f0, nf, K, out, s)
    const uint8_t* im = reinterpret_cast<const uint8_t*>(dummy);
    const uint8_t* im_odd = reinterpret_cast<const uint8_t*>(dummy + 1);       // a map may start at any byte address: not a refusal by itself
    int32_t* op = reinterpret_cast<int32_t*>(dummy);
    REFUSED(pc_instance_scores(nullptr, pb, 4, 12, 12, 0, 4, 8, op, nullptr), "null");
    REFUSED(pc_instance_scores(im, nullptr, 4, 12, 12, 0, 4, 8, op, nullptr), "null");
    REFUSED(pc_instance_scores(im, pb, 4, 12, 12, 0, 4, 8, nullptr, nullptr), "null");
    REFUSED(pc_instance_scores(im, pb, 0, 12, 12, 0, 1, 8, op, nullptr), "outside");
    REFUSED(pc_instance_scores(im, pb, -1, 12, 12, 0, 1, 8, op, nullptr), "outside");
    REFUSED(pc_instance_scores(im, pb, 4, 0, 12, 0, 4, 8, op, nullptr), "outside");
    REFUSED(pc_instance_scores(im, pb, 4, 12, 0, 0, 4, 8, op, nullptr), "outside");
    REFUSED(pc_instance_scores(im, pb, 4, INT_MIN, 12, 0, 4, 8, op, nullptr), "outside");
    REFUSED(pc_instance_scores(im, pb, 4, 65536, 32768, 0, 4, 8, op, nullptr), "2^31");
    REFUSED(pc_instance_scores(im, pb, 4, INT_MAX, INT_MAX, 0, 4, 8, op, nullptr), "2^31");
    REFUSED(pc_instance_scores(im, pb, 4, 12, 12, -1, 4, 8, op, nullptr), "f0");
    REFUSED(pc_instance_scores(im, pb, 4, 12, 12, 0, 0, 8, op, nullptr), "f0");
    REFUSED(pc_instance_scores(im, pb, 4, 12, 12, 0, -2, 8, op, nullptr), "f0");
    REFUSED(pc_instance_scores(im, pb, 4, 12, 12, 0, 5, 8, op, nullptr), "f0");
    REFUSED(pc_instance_scores(im, pb, 4, 12, 12, 3, 2, 8, op, nullptr), "f0");
    REFUSED(pc_instance_scores(im, pb, 4, 12, 12, 4, 1, 8, op, nullptr), "f0");
    REFUSED(pc_instance_scores(im, pb, INT_MAX, 12, 12, INT_MAX, INT_MAX, 8, op, nullptr), "f0");          // f0 + nf beyond int32
    REFUSED(pc_instance_scores(im, pb, INT_MAX, 12, 12, 1, INT_MAX, 8, op, nullptr), "f0");
    REFUSED(pc_instance_scores(im, pb, 4, 12, 12, 0, 4, 0, op, nullptr), "K =");
    REFUSED(pc_instance_scores(im, pb, 4, 12, 12, 0, 4, 33, op, nullptr), "K =");
    REFUSED(pc_instance_scores(im, pb, 4, 12, 12, 0, 4, -1, op, nullptr), "K =");
    REFUSED(pc_instance_scores(im, pb, 4, 12, 12, 0, 4, INT_MAX, op, nullptr), "K =");
    REFUSED(pc_instance_scores(im_odd, pb_odd, 4, 12, 12, 0, 4, 8, op, nullptr), "aligned");
    REFUSED(pc_instance_scores(im_odd, pb, 4, 12, 12, 0, 4, 8, reinterpret_cast<int32_t*>(dummy + 2), nullptr), "aligned");
    REFUSED(pc_instance_scores(nullptr, nullptr, 0, 0, 0, -1, 0, 0, nullptr, nullptr), "null");

    if (fails) { std::printf("%d host-side checks failed\n", fails); return 1; }
    std::printf("instance scores host driver: all checks passed\n");
    return 0;
}
