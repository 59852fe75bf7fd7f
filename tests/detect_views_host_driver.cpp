// Host-side checks of pc_clips_from_u8_views / pc_detect_frames_views / pc_detect_frames_views_ws_bytes without a GPU, linked against the
// AddressSanitizer + UBSan build of the library (`make -C pi-consistency-activity-detection_amd/csrc asan/detect_views_host_driver`): every
// call returns through the entry's own argument checks, in front of any HIP call, so an out-of-bounds access or undefined behaviour on the
// host side (the walks over the host arrays `views` and `starts`, the crop and workspace arithmetic) ends the process with a sanitizer
// report.  tests/test_detect_views_cpu.py builds and runs it.
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
    alignas(16) static char dummy[256];
    const uint8_t* u8 = reinterpret_cast<const uint8_t*>(dummy);
    uint8_t* mk = reinterpret_cast<uint8_t*>(dummy);
    float* fp = reinterpret_cast<float*>(dummy);
    float* odd = reinterpret_cast<float*>(dummy + 4);
    int32_t* ip = reinterpret_cast<int32_t*>(dummy);
    void* ws = dummy;
    int32_t starts[32];
    for (int c = 0; c < 32; ++c) starts[c] = c;
    const int32_t vw[2][3] = {{2, 2, 0}, {1, 3, 1}};                  // two good views of a 12 x 12 frame at S = 8
    const int32_t* views = &vw[0][0];

    // pc_clips_from_u8_views(video, F, H, W, S, views, V, view_stride, starts, n, f_skip, data, s)
    REFUSED(pc_clips_from_u8_views(nullptr, 20, 12, 12, 8, views, 2, 2, starts, 2, 2, fp, nullptr), "null");
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, nullptr, 2, 2, starts, 2, 2, fp, nullptr), "null");
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, views, 2, 2, nullptr, 2, 2, fp, nullptr), "null");
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, views, 2, 2, starts, 2, 2, nullptr, nullptr), "null");
    REFUSED(pc_clips_from_u8_views(u8, 0, 12, 12, 8, views, 2, 2, starts, 2, 2, fp, nullptr), "outside");
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 0, views, 2, 2, starts, 2, 2, fp, nullptr), "outside");
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 16, views, 2, 2, starts, 2, 2, fp, nullptr), "outside");
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, views, 0, 2, starts, 2, 2, fp, nullptr), "views outside");
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, views, -1, 2, starts, 2, 2, fp, nullptr), "views outside");
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, views, 33, 2, starts, 2, 2, fp, nullptr), "views outside");     // views[6..] is never read
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, views, 2, 1, starts, 2, 2, fp, nullptr), "view_stride");
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, views, 2, -5, starts, 2, 2, fp, nullptr), "view_stride");
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, views, 2, 2, starts, 0, 2, fp, nullptr), "clips outside");
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, views, 2, 40, starts, 33, 2, fp, nullptr), "clips outside");    // starts[32] is never read
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, views, 2, 2, starts, 2, 0, fp, nullptr), "f_skip");
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, views, 2, 2, starts, 2, 2, odd, nullptr), "16-byte");

    // pc_detect_frames_views(logits, F, H, W, S, views, V, view_stride, starts, n, f_skip, row0, mask, rec, ws, s)
    REFUSED(pc_detect_frames_views(nullptr, 20, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, mk, ip, ws, nullptr), "null");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, nullptr, 2, 2, starts, 2, 2, 0, mk, ip, ws, nullptr), "null");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, 2, nullptr, 2, 2, 0, mk, ip, ws, nullptr), "null");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, mk, nullptr, ws, nullptr), "null");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, mk, ip, nullptr, nullptr), "null");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, nullptr, ip, nullptr, nullptr), "null");   // a null mask alone is no refusal
    REFUSED(pc_detect_frames_views(fp, 0, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, mk, ip, ws, nullptr), "outside");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 0, views, 2, 2, starts, 2, 2, 0, mk, ip, ws, nullptr), "outside");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 16, views, 2, 2, starts, 2, 2, 0, mk, ip, ws, nullptr), "outside");
    REFUSED(pc_detect_frames_views(fp, 20, 1 << 16, 1 << 16, 8, views, 2, 2, starts, 2, 2, 0, mk, ip, ws, nullptr), "2^31");  // H * W beyond int32
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 6, views, 2, 2, starts, 2, 2, 0, mk, ip, ws, nullptr), "multiple of 4");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 0, 2, starts, 2, 2, 0, mk, ip, ws, nullptr), "views outside");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 33, 2, starts, 2, 2, 0, mk, ip, ws, nullptr), "views outside");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, 1, starts, 2, 2, 0, mk, ip, ws, nullptr), "view_stride");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, 2, starts, 0, 2, 0, mk, ip, ws, nullptr), "clips outside");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, 40, starts, 33, 2, 0, mk, ip, ws, nullptr), "clips outside");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, 2, starts, 2, 0, 0, mk, ip, ws, nullptr), "f_skip");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, 2, starts, 2, 2, -1, mk, ip, ws, nullptr), "row0");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, 2, starts, 2, 2, INT_MAX - 1000, mk, ip, ws, nullptr), "row0");   // row0 + c * V beyond int32
    REFUSED(pc_detect_frames_views(odd, 20, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, mk, ip, ws, nullptr), "16-byte");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, mk, ip, dummy + 4, nullptr), "aligned");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, mk, reinterpret_cast<int32_t*>(dummy + 2), ws, nullptr), "aligned");

    {   // host arrays of exactly V * 3 and n entries: one read past either is a sanitizer report.  The bad view is the last of 32.
        int32_t* tab = new int32_t[32 * 3];
        int32_t* three = new int32_t[3]{0, 1, -5};
        const int32_t bad[][3] = {{5, 2, 0}, {2, 5, 0}, {-1, 2, 0}, {2, -1, 1}, {INT_MAX - 4, 0, 0}, {0, INT_MAX, 1}};
        for (const auto& b : bad) {
            for (int v = 0; v < 32; ++v) { tab[3 * v] = v % 5; tab[3 * v + 1] = v % 4; tab[3 * v + 2] = v & 1; }
            tab[93] = b[0]; tab[94] = b[1]; tab[95] = b[2];
            REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, tab, 32, 2, starts, 2, 2, fp, nullptr), "outside");
            REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, tab, 32, 2, starts, 2, 2, 0, mk, ip, ws, nullptr), "outside");
        }
        const int32_t badflip[] = {2, -1, INT_MIN, 256};
        for (int fl : badflip) {
            tab[93] = 4; tab[94] = 4; tab[95] = fl;
            REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, tab, 32, 2, starts, 2, 2, fp, nullptr), "flip");
            REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, tab, 32, 2, starts, 2, 2, 0, mk, ip, ws, nullptr), "flip");
        }
        tab[95] = 1;
        REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, tab, 32, 3, three, 3, 2, fp, nullptr), "negative");
        REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, tab, 32, 3, three, 3, 2, 0, mk, ip, ws, nullptr), "negative");
        delete[] three;
        delete[] tab;
    }
    starts[31] = -1;                                                  // the last of 32: the whole host array is walked
    REFUSED(pc_clips_from_u8_views(u8, 20, 12, 12, 8, views, 2, 32, starts, 32, 2, fp, nullptr), "negative");
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, 32, starts, 32, 2, 0, mk, ip, ws, nullptr), "negative");
    starts[0] = INT_MIN;
    REFUSED(pc_detect_frames_views(fp, 20, 12, 12, 8, views, 2, INT_MAX, starts, 1, INT_MAX, 0, mk, ip, ws, nullptr), "negative");

    // pc_detect_frames_views_ws_bytes(n, H, W): host arithmetic only
    EXPECT(pc_detect_frames_views_ws_bytes(0, 8, 8) == -1 && pc_detect_frames_views_ws_bytes(33, 8, 8) == -1 && pc_detect_frames_views_ws_bytes(-1, 8, 8) == -1);
    EXPECT(pc_detect_frames_views_ws_bytes(2, 0, 8) == -1 && pc_detect_frames_views_ws_bytes(2, 8, 0) == -1 && pc_detect_frames_views_ws_bytes(2, -4, 8) == -1);
    EXPECT(pc_detect_frames_views_ws_bytes(2, 1 << 16, 1 << 15) == -1 && pc_detect_frames_views_ws_bytes(2, INT_MAX, INT_MAX) == -1);
    EXPECT(pc_detect_frames_views_ws_bytes(1, 9, 11) == 8 * 32);                             // one block per frame, one 32-byte partial per block
    EXPECT(pc_detect_frames_views_ws_bytes(14, 240, 320) == 14 * 8 * 19 * 32);               // 19200 groups of four per frame: 19 blocks of 1024
    EXPECT(pc_detect_frames_views_ws_bytes(32, 46340, 46340) == 32ll * 8 * 64 * 32);         // at most 64 blocks per frame

    if (fails) { std::printf("%d host-side checks failed\n", fails); return 1; }
    std::printf("detect views host driver: all checks passed\n");
    return 0;
}
