// Host-side checks of pc_prob_truth_hist / pc_prob_truth_hist_ws_bytes without a GPU, linked against the AddressSanitizer + UBSan build of the
// library (`make -C pi-consistency-activity-detection_amd/csrc asan/prob_hist_host_driver`): every call returns through the entry's own
// argument checks, in front of any HIP call, so undefined behaviour on the host side (the pixel and workspace arithmetic at the ends of int, a
// read past the N threshold words) ends the process with a sanitizer report.  The thresholds, the table and the workspace are heap arrays of
// exactly their size.  tests/test_detect_sweep_cpu.py builds and runs it.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "picons.h"

static int fails = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { ++fails; std::printf("FAILED %s:%d  %s  [%s]\n", __FILE__, __LINE__, #cond, pc_last_error()); } \
    } while (0)
#define REFUSED(call, word) EXPECT((call) == PC_E_ARG && std::strstr(pc_last_error(), word) && std::strstr(pc_last_error(), "pc_prob_truth_hist"))
// (F, H, W, f0, nf) with good pointers and the three words of `three`
#define RANGE(F, H, W, f0, nf, word) REFUSED(pc_prob_truth_hist(pr, tr, F, H, W, f0, nf, three.get(), 3, out, ws, nullptr), word)

// N words on the heap, exactly: v0, v0 + step, ...
static std::unique_ptr<uint16_t[]> words(int N, int v0, int step) {
    std::unique_ptr<uint16_t[]> w(new uint16_t[N]);
    for (int k = 0; k < N; ++k) w[k] = (uint16_t)(v0 + k * step);
    return w;
}

int main() {
    EXPECT(pc_version() == PC_VERSION && PC_VERSION == 107);
    EXPECT(PC_SWEEP_MAX_THRESHOLDS == 64 && PC_PROB_ONE == 65535);
    // 4 frames of 12 x 12 at N = 3: the map sides are never read on a refusal; table and workspace exactly as large as the call would need
    std::unique_ptr<uint16_t[]> probs(new uint16_t[4 * 144 + 1]);
    std::unique_ptr<uint8_t[]> truths(new uint8_t[4 * 144 + 1]);
    const uint16_t* pr = probs.get() + 1;                                    // a map may start at any 2-byte address,
    const uint8_t* tr = truths.get() + 1;                                    // its truth at any byte
    std::unique_ptr<int32_t[]> table(new int32_t[4 * 2 * 4]);
    int32_t* out = table.get();
    EXPECT(pc_prob_truth_hist_ws_bytes(4, 12, 12, 3) == 4 * 8 * 4);
    std::unique_ptr<uint64_t[]> scratch(new uint64_t[4 * 8 * 4 / 8]);
    void* ws = scratch.get();
    const auto three = words(3, 100, 100);

    // pc_prob_truth_hist_ws_bytes(nf, H, W, N) = nf * bpf * 2 * (N + 1) * 4 with bpf = ceil(ceil(H * W / 4) / 1024) in 1..64
    EXPECT(pc_prob_truth_hist_ws_bytes(1, 1, 1, 1) == 4 * 4);
    EXPECT(pc_prob_truth_hist_ws_bytes(3, 5, 7, 19) == 3 * 40 * 4);
    EXPECT(pc_prob_truth_hist_ws_bytes(1, 64, 64, 1) == 4 * 4);                // 1024 groups: the last that one block takes
    EXPECT(pc_prob_truth_hist_ws_bytes(1, 64, 65, 1) == 2 * 4 * 4);
    EXPECT(pc_prob_truth_hist_ws_bytes(40, 240, 320, 19) == 40ll * 19 * 40 * 4);
    EXPECT(pc_prob_truth_hist_ws_bytes(1, 1, 63 * 4096, 64) == 63 * 130 * 4);
    EXPECT(pc_prob_truth_hist_ws_bytes(1, 1, 64 * 4096 + 1, 64) == 64 * 130 * 4);   // the cap
    EXPECT(pc_prob_truth_hist_ws_bytes(1, 1080, 1920, 64) == 64ll * 130 * 4);
    EXPECT(pc_prob_truth_hist_ws_bytes(INT_MAX, 46340, 46340, 64) == (int64_t)INT_MAX * 64 * 130 * 4);   // the largest there is
    EXPECT(pc_prob_truth_hist_ws_bytes(1, 1, INT_MAX, 64) == 64ll * 130 * 4);
    EXPECT(pc_prob_truth_hist_ws_bytes(0, 4, 4, 1) == -1 && pc_prob_truth_hist_ws_bytes(-1, 4, 4, 1) == -1 && pc_prob_truth_hist_ws_bytes(INT_MIN, 4, 4, 1) == -1);
    EXPECT(pc_prob_truth_hist_ws_bytes(1, 0, 4, 1) == -1 && pc_prob_truth_hist_ws_bytes(1, 4, 0, 1) == -1 && pc_prob_truth_hist_ws_bytes(1, INT_MIN, INT_MIN, 1) == -1);
    EXPECT(pc_prob_truth_hist_ws_bytes(1, 1 << 16, 1 << 15, 1) == -1 && pc_prob_truth_hist_ws_bytes(1, INT_MAX, INT_MAX, 1) == -1);
    EXPECT(pc_prob_truth_hist_ws_bytes(1, 46341, 46341, 1) == -1 && pc_prob_truth_hist_ws_bytes(1, 2, INT_MAX, 1) == -1);
    EXPECT(pc_prob_truth_hist_ws_bytes(1, 4, 4, 0) == -1 && pc_prob_truth_hist_ws_bytes(1, 4, 4, 65) == -1 && pc_prob_truth_hist_ws_bytes(1, 4, 4, INT_MAX) == -1);
    EXPECT(pc_prob_truth_hist_ws_bytes(1, 4, 4, -1) == -1 && pc_prob_truth_hist_ws_bytes(1, 4, 4, INT_MIN) == -1);

    // null pointers
    REFUSED(pc_prob_truth_hist(nullptr, tr, 4, 12, 12, 0, 4, three.get(), 3, out, ws, nullptr), "null");
    REFUSED(pc_prob_truth_hist(pr, nullptr, 4, 12, 12, 0, 4, three.get(), 3, out, ws, nullptr), "null");
    REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, nullptr, 3, out, ws, nullptr), "null");
    REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, three.get(), 3, nullptr, ws, nullptr), "null");
    REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, three.get(), 3, out, nullptr, nullptr), "null");
    // the frame and the range
    RANGE(0, 12, 12, 0, 1, "outside");
    RANGE(-1, 12, 12, 0, 1, "outside");
    RANGE(4, 0, 12, 0, 4, "outside");
    RANGE(4, 12, 0, 0, 4, "outside");
    RANGE(4, INT_MIN, 12, 0, 4, "outside");
    RANGE(4, 12, -3, 0, 4, "outside");
    RANGE(4, 1 << 16, 1 << 15, 0, 4, "2^31");                                // exactly 2^31 pixels
    RANGE(4, INT_MAX, INT_MAX, 0, 4, "2^31");
    RANGE(4, 46341, 46341, 0, 4, "2^31");
    RANGE(4, 12, 12, -1, 4, "f0");
    RANGE(4, 12, 12, 0, 0, "f0");
    RANGE(4, 12, 12, 0, -2, "f0");
    RANGE(4, 12, 12, 0, 5, "f0");
    RANGE(4, 12, 12, 3, 2, "f0");
    RANGE(4, 12, 12, 4, 1, "f0");
    RANGE(INT_MAX, 12, 12, INT_MAX, INT_MAX, "f0");                          // f0 + nf beyond int32
    RANGE(INT_MAX, 12, 12, 1, INT_MAX, "f0");
    // the number of thresholds: no word is read when it is out of range (a one-word array stands behind the pointer)
    const auto one = words(1, 32768, 0);
    for (int N : {0, -1, 65, INT_MAX, INT_MIN})
        REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, one.get(), N, out, ws, nullptr), "N =");
    // the words: exactly N of them are read
    REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, words(1, 0, 0).get(), 1, out, ws, nullptr), "word of 0");
    REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, words(3, 0, 7).get(), 3, out, ws, nullptr), "word of 0");
    REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, words(2, 5, 0).get(), 2, out, ws, nullptr), "ascending");        // twice the same
    REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, words(3, 300, -100).get(), 3, out, ws, nullptr), "ascending");
    REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, words(64, 65535, -1).get(), 64, out, ws, nullptr), "ascending");
    {
        auto w = words(64, 1, 1000);                                         // 1 .. 63001 ascending, the last one repeated
        w[63] = w[62];
        REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, w.get(), 64, out, ws, nullptr), "ascending");
        w[63] = 65535; w[31] = w[30] - 1;
        REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, w.get(), 64, out, ws, nullptr), "ascending");
    }
    // alignment
    REFUSED(pc_prob_truth_hist(reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(pr) + 1), tr, 4, 12, 12, 0, 4, three.get(), 3, out, ws, nullptr),
            "prob must be");
    for (int o = 1; o < 4; ++o)
        REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, three.get(), 3, reinterpret_cast<int32_t*>(reinterpret_cast<char*>(out) + o), ws, nullptr), "out must be");
    for (int o = 1; o < 8; ++o)
        REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, three.get(), 3, out, static_cast<char*>(ws) + o, nullptr), "ws must be");
    // with everything wrong: the pointers first, then the frame, the range, the thresholds, the alignment
    REFUSED(pc_prob_truth_hist(nullptr, nullptr, 0, 0, 0, -1, 0, nullptr, 0, nullptr, nullptr, nullptr), "null");
    REFUSED(pc_prob_truth_hist(pr, tr, 0, 0, 0, -1, 0, one.get(), 0, out, ws, nullptr), "outside");
    REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, -1, 0, one.get(), 0, out, ws, nullptr), "f0");
    REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, one.get(), 0, out, static_cast<char*>(ws) + 1, nullptr), "N =");
    REFUSED(pc_prob_truth_hist(pr, tr, 4, 12, 12, 0, 4, words(1, 0, 0).get(), 1, out, static_cast<char*>(ws) + 1, nullptr), "word of 0");

    if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
