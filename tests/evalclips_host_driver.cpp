// Host-side checks of pc_truth_frame_flags / pc_eval_clips_from_u8 / pc_video_vote without a GPU, linked against the AddressSanitizer +
// UBSan build of the library (`make -C pi-consistency-activity-detection_amd/csrc asan/evalclips_host_driver`): every call returns through the
// entry's own argument checks, in front of any HIP call, so an out-of-bounds access or undefined behaviour on the host side (the walk over
// the host array `starts`, the crop arithmetic) ends the process with a sanitizer report.  tests/test_evalstep_cpu.py builds and runs it.
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
    EXPECT(pc_version() == PC_VERSION && PC_VERSION >= 106);
    alignas(16) static char dummy[256];
    const uint8_t* u8 = reinterpret_cast<const uint8_t*>(dummy);
    float* fp = reinterpret_cast<float*>(dummy);
    float* odd = reinterpret_cast<float*>(dummy + 4);
    int32_t* ip = reinterpret_cast<int32_t*>(dummy);

    // pc_truth_frame_flags(truth, F, H, W, h0, w0, S, flags, s)
    REFUSED(pc_truth_frame_flags(nullptr, 4, 12, 12, 2, 2, 8, ip, nullptr), "null");
    REFUSED(pc_truth_frame_flags(u8, 4, 12, 12, 2, 2, 8, nullptr, nullptr), "null");
    REFUSED(pc_truth_frame_flags(u8, 0, 12, 12, 2, 2, 8, ip, nullptr), "outside");
    REFUSED(pc_truth_frame_flags(u8, -1, 12, 12, 2, 2, 8, ip, nullptr), "outside");
    REFUSED(pc_truth_frame_flags(u8, 4, 12, 12, 5, 2, 8, ip, nullptr), "outside");
    REFUSED(pc_truth_frame_flags(u8, 4, 12, 12, 2, 5, 8, ip, nullptr), "outside");
    REFUSED(pc_truth_frame_flags(u8, 4, 12, 12, -1, 2, 8, ip, nullptr), "outside");
    REFUSED(pc_truth_frame_flags(u8, 4, 12, 12, 2, -1, 8, ip, nullptr), "outside");
    REFUSED(pc_truth_frame_flags(u8, 4, 12, 12, 0, 0, 0, ip, nullptr), "outside");
    REFUSED(pc_truth_frame_flags(u8, 4, 12, 12, 0, 0, 13, ip, nullptr), "outside");
    REFUSED(pc_truth_frame_flags(u8, 4, INT_MAX, INT_MAX, INT_MAX - 4, INT_MAX - 4, 8, ip, nullptr), "outside");      // h0 + S beyond int32

    // pc_eval_clips_from_u8(video, truth, F, H, W, h0, w0, S, starts, n, f_skip, data, gt, s)
    int32_t starts[32];
    for (int c = 0; c < 32; ++c) starts[c] = c;
    REFUSED(pc_eval_clips_from_u8(nullptr, u8, 20, 12, 12, 2, 2, 8, starts, 2, 2, fp, fp, nullptr), "null");
    REFUSED(pc_eval_clips_from_u8(u8, nullptr, 20, 12, 12, 2, 2, 8, starts, 2, 2, fp, fp, nullptr), "null");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 2, 8, nullptr, 2, 2, fp, fp, nullptr), "null");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 2, 8, starts, 2, 2, nullptr, fp, nullptr), "null");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 2, 8, starts, 2, 2, fp, nullptr, nullptr), "null");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 0, 12, 12, 2, 2, 8, starts, 2, 2, fp, fp, nullptr), "outside");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 5, 2, 8, starts, 2, 2, fp, fp, nullptr), "outside");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 5, 8, starts, 2, 2, fp, fp, nullptr), "outside");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, -1, 2, 8, starts, 2, 2, fp, fp, nullptr), "outside");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, -1, 8, starts, 2, 2, fp, fp, nullptr), "outside");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 0, 0, 0, starts, 2, 2, fp, fp, nullptr), "outside");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, INT_MAX, INT_MAX, INT_MAX - 4, 0, 8, starts, 2, 2, fp, fp, nullptr), "outside");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 2, 8, starts, 0, 2, fp, fp, nullptr), "clips outside");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 2, 8, starts, -3, 2, fp, fp, nullptr), "clips outside");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 2, 8, starts, 33, 2, fp, fp, nullptr), "clips outside");       // starts[32] is never read
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 2, 8, starts, 2, 0, fp, fp, nullptr), "f_skip");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 2, 8, starts, 2, -2, fp, fp, nullptr), "f_skip");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 2, 8, starts, 2, 2, odd, fp, nullptr), "16-byte");
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 2, 8, starts, 2, 2, fp, odd, nullptr), "16-byte");
    starts[31] = -1;                                                  // the last of 32: the whole host array is walked
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 2, 8, starts, 32, 2, fp, fp, nullptr), "negative");
    starts[0] = INT_MIN;
    REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 2, 8, starts, 1, INT_MAX, fp, fp, nullptr), "negative");
    {   // a host array of exactly n entries: one read past it is a sanitizer report
        int32_t* three = new int32_t[3]{0, 1, -5};
        REFUSED(pc_eval_clips_from_u8(u8, u8, 20, 12, 12, 2, 2, 8, three, 3, 2, fp, fp, nullptr), "negative");
        delete[] three;
    }

    // pc_video_vote(pred, n, C, label, n_correct, s)
    REFUSED(pc_video_vote(nullptr, 3, 24, 1, ip, nullptr), "null");
    REFUSED(pc_video_vote(fp, 3, 24, 1, nullptr, nullptr), "null");
    REFUSED(pc_video_vote(fp, 0, 24, 1, ip, nullptr), "n = 0");
    REFUSED(pc_video_vote(fp, -1, 24, 1, ip, nullptr), "n = -1");
    REFUSED(pc_video_vote(fp, 3, 0, 0, ip, nullptr), "C = 0");
    REFUSED(pc_video_vote(fp, 1 << 20, 1 << 20, 0, ip, nullptr), "rows");      // n * C beyond int32
    REFUSED(pc_video_vote(fp, 3, 24, -1, ip, nullptr), "label");
    REFUSED(pc_video_vote(fp, 3, 24, 24, ip, nullptr), "label");

    if (fails) { std::printf("%d host-side checks failed\n", fails); return 1; }
    std::printf("evalclips host driver: all checks passed\n");
    return 0;
}
