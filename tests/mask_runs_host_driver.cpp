// Host-side checks of pc_mask_run_ws_bytes / pc_mask_run_index / pc_mask_runs without a GPU, linked against the AddressSanitizer + UBSan
// build of the library (`make -C pi-consistency-activity-detection_amd/csrc asan/mask_runs_host_driver`): every call returns through the
// entries' own argument checks, in front of any HIP call, so undefined behaviour on the host side (the row and pixel arithmetic at the ends
// of int) ends the process with a sanitizer report.  tests/test_mask_runs_cpu.py builds and runs it.
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
#define REFUSED(entry, call, word) EXPECT((call) == PC_E_ARG && std::strstr(pc_last_error(), word) && std::strstr(pc_last_error(), entry))
// both entries take (map, F, H, W, f0, nf, ...): the same range, the same refusal
#define BOTH(F, H, W, f0, nf, word)                                                                        \
    do {                                                                                                   \
        REFUSED("pc_mask_run_index", pc_mask_run_index(mp, F, H, W, f0, nf, ix, ws, nullptr), word);      \
        REFUSED("pc_mask_runs", pc_mask_runs(mp, F, H, W, f0, nf, ix, 4, rn, nullptr), word);             \
    } while (0)

int main() {
    EXPECT(pc_version() == PC_VERSION && PC_VERSION == 107);
    EXPECT(PC_RUN_WORDS == 2);
    alignas(16) static char dummy[256];
    const uint8_t* mp = reinterpret_cast<const uint8_t*>(dummy + 1);         // a map may start at any byte
    int32_t* ix = reinterpret_cast<int32_t*>(dummy);
    void* ws = dummy + 64;
    uint32_t* rn = reinterpret_cast<uint32_t*>(dummy + 128);
    int32_t* odd_i = reinterpret_cast<int32_t*>(dummy + 2);
    uint32_t* odd_r = reinterpret_cast<uint32_t*>(dummy + 130);

    // pc_mask_run_ws_bytes(nf, H): host arithmetic, -1 where the calls refuse
    EXPECT(pc_mask_run_ws_bytes(1, 1) >= 4 && pc_mask_run_ws_bytes(1, 1) % 4 == 0);
    EXPECT(pc_mask_run_ws_bytes(40, 240) >= 4 && pc_mask_run_ws_bytes(40, 240) <= 4ll * 40 * 240);
    EXPECT(pc_mask_run_ws_bytes(1 << 12, 1 << 12) > 0);                      // 2^24 rows: the last that fit
    EXPECT(pc_mask_run_ws_bytes((1 << 12) + 1, 1 << 12) == -1);
    EXPECT(pc_mask_run_ws_bytes(0, 4) == -1 && pc_mask_run_ws_bytes(4, 0) == -1 && pc_mask_run_ws_bytes(-1, 4) == -1);
    EXPECT(pc_mask_run_ws_bytes(INT_MAX, INT_MAX) == -1 && pc_mask_run_ws_bytes(INT_MIN, INT_MIN) == -1 && pc_mask_run_ws_bytes(INT_MAX, 1) == -1);

    // null pointers
    REFUSED("pc_mask_run_index", pc_mask_run_index(nullptr, 4, 12, 12, 0, 4, ix, ws, nullptr), "map is null");
    REFUSED("pc_mask_run_index", pc_mask_run_index(mp, 4, 12, 12, 0, 4, nullptr, ws, nullptr), "index is null");
    REFUSED("pc_mask_run_index", pc_mask_run_index(mp, 4, 12, 12, 0, 4, ix, nullptr, nullptr), "ws is null");
    REFUSED("pc_mask_runs", pc_mask_runs(nullptr, 4, 12, 12, 0, 4, ix, 4, rn, nullptr), "map is null");
    REFUSED("pc_mask_runs", pc_mask_runs(mp, 4, 12, 12, 0, 4, nullptr, 4, rn, nullptr), "index is null");
    REFUSED("pc_mask_runs", pc_mask_runs(mp, 4, 12, 12, 0, 4, ix, 1, nullptr, nullptr), "runs is null");
    REFUSED("pc_mask_runs", pc_mask_runs(mp, 4, 12, 12, 0, 4, ix, INT64_MAX, nullptr, nullptr), "runs is null");
    REFUSED("pc_mask_runs", pc_mask_runs(mp, 4, 12, 12, 0, 4, ix, -1, rn, nullptr), "cap =");
    REFUSED("pc_mask_runs", pc_mask_runs(mp, 4, 12, 12, 0, 4, ix, INT64_MIN, rn, nullptr), "cap =");
    REFUSED("pc_mask_runs", pc_mask_runs(mp, 4, 12, 12, 0, 4, ix, -1, nullptr, nullptr), "cap =");
    // the frame and the range
    BOTH(0, 12, 12, 0, 1, "outside");
    BOTH(-1, 12, 12, 0, 1, "outside");
    BOTH(4, 0, 12, 0, 4, "outside");
    BOTH(4, 12, 0, 0, 4, "outside");
    BOTH(4, INT_MIN, 12, 0, 4, "outside");
    BOTH(4, 12, -3, 0, 4, "outside");
    BOTH(4, 12, 65536, 0, 4, "W =");
    BOTH(4, 12, INT_MAX, 0, 4, "W =");
    BOTH(4, 12, 12, -1, 4, "f0");
    BOTH(4, 12, 12, 0, 0, "f0");
    BOTH(4, 12, 12, 0, -2, "f0");
    BOTH(4, 12, 12, 0, 5, "f0");
    BOTH(4, 12, 12, 3, 2, "f0");
    BOTH(4, 12, 12, 4, 1, "f0");
    BOTH(INT_MAX, 12, 12, INT_MAX, INT_MAX, "f0");                           // f0 + nf beyond int32
    BOTH(INT_MAX, 12, 12, 1, INT_MAX, "f0");
    BOTH(4097, 4096, 1, 0, 4097, "2^24");                                    // one row too many
    BOTH(INT_MAX, INT_MAX, 1, 0, INT_MAX, "2^24");
    BOTH(2, INT_MAX, 1, 0, 2, "2^24");
    BOTH(8, 1 << 14, 1 << 14, 0, 8, "2^31");                                 // 2^17 rows of 2^14: exactly 2^31 pixels
    BOTH(1, 1 << 16, 32768, 0, 1, "2^31");
    BOTH(1 << 12, 1 << 12, 65535, 0, 1 << 12, "2^31");                       // 2^24 rows pass, 2^40 pixels do not
    // alignment
    REFUSED("pc_mask_run_index", pc_mask_run_index(mp, 4, 12, 12, 0, 4, odd_i, ws, nullptr), "index must be");
    REFUSED("pc_mask_run_index", pc_mask_run_index(mp, 4, 12, 12, 0, 4, ix, dummy + 65, nullptr), "ws must be");
    REFUSED("pc_mask_run_index", pc_mask_run_index(mp, 4, 12, 12, 0, 4, ix, dummy + 66, nullptr), "ws must be");
    REFUSED("pc_mask_runs", pc_mask_runs(mp, 4, 12, 12, 0, 4, odd_i, 4, rn, nullptr), "index must be");
    REFUSED("pc_mask_runs", pc_mask_runs(mp, 4, 12, 12, 0, 4, ix, 4, odd_r, nullptr), "runs must be");
    REFUSED("pc_mask_runs", pc_mask_runs(mp, 4, 12, 12, 0, 4, ix, 0, odd_r, nullptr), "runs must be");
    // with everything wrong the map is named first, then the frame, the range, the sizes
    REFUSED("pc_mask_runs", pc_mask_runs(nullptr, 0, 0, 0, -1, 0, nullptr, -1, nullptr, nullptr), "map is null");
    REFUSED("pc_mask_runs", pc_mask_runs(mp, 0, 0, 0, -1, 0, nullptr, -1, nullptr, nullptr), "outside");
    REFUSED("pc_mask_runs", pc_mask_runs(mp, 4, 12, 12, -1, 0, nullptr, -1, nullptr, nullptr), "f0");
    REFUSED("pc_mask_runs", pc_mask_runs(mp, 4, 12, 12, 0, 4, nullptr, -1, nullptr, nullptr), "index is null");

    if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
