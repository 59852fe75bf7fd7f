// Host-side checks of pc_map_crosstab / pc_map_crosstab_ws_bytes without a GPU, linked against the AddressSanitizer + UBSan build of the
// library (`make -C pi-consistency-activity-detection_amd/csrc asan/map_crosstab_host_driver`): every call returns through the entry's own
// argument checks, in front of any HIP call, so undefined behaviour on the host side (the pixel and workspace arithmetic at the ends of int)
// ends the process with a sanitizer report.  tests/test_detect_score_cpu.py builds and runs it.
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
#define REFUSED(call, word) EXPECT((call) == PC_E_ARG && std::strstr(pc_last_error(), word) && std::strstr(pc_last_error(), "pc_map_crosstab"))
// (F, H, W, f0, nf, P, A) with good pointers
#define RANGE(F, H, W, f0, nf, P, A, word) REFUSED(pc_map_crosstab(pr, tr, F, H, W, f0, nf, P, A, out, ws, nullptr), word)

int main() {
    EXPECT(pc_version() == PC_VERSION && PC_VERSION == 107);
    EXPECT(PC_CROSS_MAX_SLOTS == 32);
    alignas(16) static char dummy[512];
    const uint8_t* pr = reinterpret_cast<const uint8_t*>(dummy + 1);         // a map may start at any byte, and the two sides differently
    const uint8_t* tr = reinterpret_cast<const uint8_t*>(dummy + 130);
    int32_t* out = reinterpret_cast<int32_t*>(dummy + 256);
    void* ws = dummy + 384;

    // pc_map_crosstab_ws_bytes(nf, H, W, P, A) = nf * bpf * (P + 2) * (A + 2) * 4 with bpf = ceil(ceil(H * W / 4) / 1024) in 1..64
    EXPECT(pc_map_crosstab_ws_bytes(1, 1, 1, 1, 1) == 9 * 4);
    EXPECT(pc_map_crosstab_ws_bytes(3, 5, 7, 8, 3) == 3 * 10 * 5 * 4);
    EXPECT(pc_map_crosstab_ws_bytes(1, 64, 64, 1, 1) == 9 * 4);              // 1024 groups: the last that one block takes
    EXPECT(pc_map_crosstab_ws_bytes(1, 64, 65, 1, 1) == 2 * 9 * 4);
    EXPECT(pc_map_crosstab_ws_bytes(40, 240, 320, 1, 1) == 40ll * 19 * 9 * 4);
    EXPECT(pc_map_crosstab_ws_bytes(1, 1, 63 * 4096, 1, 1) == 63 * 9 * 4);
    EXPECT(pc_map_crosstab_ws_bytes(1, 1, 64 * 4096, 1, 1) == 64 * 9 * 4);
    EXPECT(pc_map_crosstab_ws_bytes(1, 1, 64 * 4096 + 1, 1, 1) == 64 * 9 * 4);   // the cap
    EXPECT(pc_map_crosstab_ws_bytes(1, 1080, 1920, 32, 32) == 64ll * 34 * 34 * 4);   // P = A = 32 at 64 blocks a frame
    EXPECT(pc_map_crosstab_ws_bytes(INT_MAX, 46340, 46340, 32, 32) == (int64_t)INT_MAX * 64 * 1156 * 4);   // the largest there is
    EXPECT(pc_map_crosstab_ws_bytes(1, 1, INT_MAX, 32, 32) == 64ll * 1156 * 4);
    EXPECT(pc_map_crosstab_ws_bytes(0, 4, 4, 1, 1) == -1 && pc_map_crosstab_ws_bytes(-1, 4, 4, 1, 1) == -1 && pc_map_crosstab_ws_bytes(INT_MIN, 4, 4, 1, 1) == -1);
    EXPECT(pc_map_crosstab_ws_bytes(1, 0, 4, 1, 1) == -1 && pc_map_crosstab_ws_bytes(1, 4, 0, 1, 1) == -1 && pc_map_crosstab_ws_bytes(1, INT_MIN, INT_MIN, 1, 1) == -1);
    EXPECT(pc_map_crosstab_ws_bytes(1, 1 << 16, 1 << 15, 1, 1) == -1 && pc_map_crosstab_ws_bytes(1, INT_MAX, INT_MAX, 1, 1) == -1);
    EXPECT(pc_map_crosstab_ws_bytes(1, 46341, 46341, 1, 1) == -1 && pc_map_crosstab_ws_bytes(1, 2, INT_MAX, 1, 1) == -1);
    EXPECT(pc_map_crosstab_ws_bytes(1, 4, 4, 0, 1) == -1 && pc_map_crosstab_ws_bytes(1, 4, 4, 33, 1) == -1 && pc_map_crosstab_ws_bytes(1, 4, 4, INT_MAX, 1) == -1);
    EXPECT(pc_map_crosstab_ws_bytes(1, 4, 4, 1, 0) == -1 && pc_map_crosstab_ws_bytes(1, 4, 4, 1, 33) == -1 && pc_map_crosstab_ws_bytes(1, 4, 4, 1, INT_MIN) == -1);

    // null pointers
    REFUSED(pc_map_crosstab(nullptr, tr, 4, 12, 12, 0, 4, 1, 1, out, ws, nullptr), "null");
    REFUSED(pc_map_crosstab(pr, nullptr, 4, 12, 12, 0, 4, 1, 1, out, ws, nullptr), "null");
    REFUSED(pc_map_crosstab(pr, tr, 4, 12, 12, 0, 4, 1, 1, nullptr, ws, nullptr), "null");
    REFUSED(pc_map_crosstab(pr, tr, 4, 12, 12, 0, 4, 1, 1, out, nullptr, nullptr), "null");
    // the frame and the range
    RANGE(0, 12, 12, 0, 1, 1, 1, "outside");
    RANGE(-1, 12, 12, 0, 1, 1, 1, "outside");
    RANGE(4, 0, 12, 0, 4, 1, 1, "outside");
    RANGE(4, 12, 0, 0, 4, 1, 1, "outside");
    RANGE(4, INT_MIN, 12, 0, 4, 1, 1, "outside");
    RANGE(4, 12, -3, 0, 4, 1, 1, "outside");
    RANGE(4, 1 << 16, 1 << 15, 0, 4, 1, 1, "2^31");                          // exactly 2^31 pixels
    RANGE(4, INT_MAX, INT_MAX, 0, 4, 1, 1, "2^31");
    RANGE(4, 46341, 46341, 0, 4, 1, 1, "2^31");
    RANGE(4, 12, 12, -1, 4, 1, 1, "f0");
    RANGE(4, 12, 12, 0, 0, 1, 1, "f0");
    RANGE(4, 12, 12, 0, -2, 1, 1, "f0");
    RANGE(4, 12, 12, 0, 5, 1, 1, "f0");
    RANGE(4, 12, 12, 3, 2, 1, 1, "f0");
    RANGE(4, 12, 12, 4, 1, 1, 1, "f0");
    RANGE(INT_MAX, 12, 12, INT_MAX, INT_MAX, 1, 1, "f0");                    // f0 + nf beyond int32
    RANGE(INT_MAX, 12, 12, 1, INT_MAX, 1, 1, "f0");
    // the slots
    RANGE(4, 12, 12, 0, 4, 0, 1, "P =");
    RANGE(4, 12, 12, 0, 4, -1, 1, "P =");
    RANGE(4, 12, 12, 0, 4, 33, 1, "P =");
    RANGE(4, 12, 12, 0, 4, INT_MAX, 1, "P =");
    RANGE(4, 12, 12, 0, 4, 1, 0, "A =");
    RANGE(4, 12, 12, 0, 4, 1, 33, "A =");
    RANGE(4, 12, 12, 0, 4, 32, INT_MIN, "A =");
    // alignment
    for (int o = 1; o < 4; ++o)
        REFUSED(pc_map_crosstab(pr, tr, 4, 12, 12, 0, 4, 1, 1, reinterpret_cast<int32_t*>(dummy + 256 + o), ws, nullptr), "out must be");
    for (int o = 1; o < 8; ++o)
        REFUSED(pc_map_crosstab(pr, tr, 4, 12, 12, 0, 4, 1, 1, out, dummy + 384 + o, nullptr), "ws must be");
    // with everything wrong: the pointers first, then the frame, the range, the slots
    REFUSED(pc_map_crosstab(nullptr, nullptr, 0, 0, 0, -1, 0, 0, 0, nullptr, nullptr, nullptr), "null");
    REFUSED(pc_map_crosstab(pr, tr, 0, 0, 0, -1, 0, 0, 0, out, ws, nullptr), "outside");
    REFUSED(pc_map_crosstab(pr, tr, 4, 12, 12, -1, 0, 0, 0, out, ws, nullptr), "f0");
    REFUSED(pc_map_crosstab(pr, tr, 4, 12, 12, 0, 4, 0, 0, out, ws, nullptr), "P =");

    if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
