// Host-side checks of pc_clips_from_u8 / pc_detect_frames / pc_detect_frames_ws_bytes / pc_video_class without a GPU, linked against the
// AddressSanitizer + UBSan build of the library (`make -C pi-consistency-activity-detection_amd/csrc asan/detect_host_driver`): every call
// returns through the entry's own argument checks, in front of any HIP call, so an out-of-bounds access or undefined behaviour on the host
// side (the walk over the host array `starts`, the crop and workspace arithmetic) ends the process with a sanitizer report.
// tests/test_detect_cpu.py builds and runs it.
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

    // pc_clips_from_u8(video, F, H, W, h0, w0, S, starts, n, f_skip, data, s)
    REFUSED(pc_clips_from_u8(nullptr, 20, 12, 12, 2, 2, 8, starts, 2, 2, fp, nullptr), "null");
    REFUSED(pc_clips_from_u8(u8, 20, 12, 12, 2, 2, 8, nullptr, 2, 2, fp, nullptr), "null");
    REFUSED(pc_clips_from_u8(u8, 20, 12, 12, 2, 2, 8, starts, 2, 2, nullptr, nullptr), "null");
    REFUSED(pc_clips_from_u8(u8, 0, 12, 12, 2, 2, 8, starts, 2, 2, fp, nullptr), "outside");
    REFUSED(pc_clips_from_u8(u8, 20, 12, 12, 5, 2, 8, starts, 2, 2, fp, nullptr), "outside");
    REFUSED(pc_clips_from_u8(u8, 20, 12, 12, 2, 5, 8, starts, 2, 2, fp, nullptr), "outside");
    REFUSED(pc_clips_from_u8(u8, 20, 12, 12, -1, 2, 8, starts, 2, 2, fp, nullptr), "outside");
    REFUSED(pc_clips_from_u8(u8, 20, 12, 12, 2, -1, 8, starts, 2, 2, fp, nullptr), "outside");
    REFUSED(pc_clips_from_u8(u8, 20, 12, 12, 0, 0, 0, starts, 2, 2, fp, nullptr), "outside");
    REFUSED(pc_clips_from_u8(u8, 20, INT_MAX, INT_MAX, INT_MAX - 4, 0, 8, starts, 2, 2, fp, nullptr), "outside");
    REFUSED(pc_clips_from_u8(u8, 20, 12, 12, 2, 2, 8, starts, 0, 2, fp, nullptr), "clips outside");
    REFUSED(pc_clips_from_u8(u8, 20, 12, 12, 2, 2, 8, starts, -3, 2, fp, nullptr), "clips outside");
    REFUSED(pc_clips_from_u8(u8, 20, 12, 12, 2, 2, 8, starts, 33, 2, fp, nullptr), "clips outside");       // starts[32] is never read
    REFUSED(pc_clips_from_u8(u8, 20, 12, 12, 2, 2, 8, starts, 2, 0, fp, nullptr), "f_skip");
    REFUSED(pc_clips_from_u8(u8, 20, 12, 12, 2, 2, 8, starts, 2, 2, odd, nullptr), "16-byte");

    // pc_detect_frames(logits, F, H, W, h0, w0, S, starts, n, f_skip, row0, mask, rec, ws, s)
    REFUSED(pc_detect_frames(nullptr, 20, 12, 12, 2, 2, 8, starts, 2, 2, 0, mk, ip, ws, nullptr), "null");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, nullptr, 2, 2, 0, mk, ip, ws, nullptr), "null");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, starts, 2, 2, 0, mk, nullptr, ws, nullptr), "null");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, starts, 2, 2, 0, mk, ip, nullptr, nullptr), "null");
    REFUSED(pc_detect_frames(fp, 0, 12, 12, 2, 2, 8, starts, 2, 2, 0, mk, ip, ws, nullptr), "outside");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 5, 2, 8, starts, 2, 2, 0, mk, ip, ws, nullptr), "outside");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 5, 8, starts, 2, 2, 0, mk, ip, ws, nullptr), "outside");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, -1, 2, 8, starts, 2, 2, 0, mk, ip, ws, nullptr), "outside");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, -1, 8, starts, 2, 2, 0, mk, ip, ws, nullptr), "outside");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 0, 0, 0, starts, 2, 2, 0, mk, ip, ws, nullptr), "outside");
    REFUSED(pc_detect_frames(fp, 20, INT_MAX, INT_MAX, INT_MAX - 4, INT_MAX - 4, 8, starts, 2, 2, 0, mk, ip, ws, nullptr), "outside");
    REFUSED(pc_detect_frames(fp, 20, 1 << 16, 1 << 16, 0, 0, 8, starts, 2, 2, 0, mk, ip, ws, nullptr), "2^31");    // H * W beyond int32
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 6, starts, 2, 2, 0, mk, ip, ws, nullptr), "multiple of 4");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, starts, 0, 2, 0, mk, ip, ws, nullptr), "clips outside");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, starts, -1, 2, 0, mk, ip, ws, nullptr), "clips outside");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, starts, 33, 2, 0, mk, ip, ws, nullptr), "clips outside");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, starts, 2, 0, 0, mk, ip, ws, nullptr), "f_skip");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, starts, 2, 2, -1, mk, ip, ws, nullptr), "row0");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, starts, 2, 2, INT_MAX, mk, ip, ws, nullptr), "row0");     // row0 + c beyond int32
    REFUSED(pc_detect_frames(odd, 20, 12, 12, 2, 2, 8, starts, 2, 2, 0, mk, ip, ws, nullptr), "16-byte");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, starts, 2, 2, 0, mk, ip, dummy + 4, nullptr), "aligned");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, starts, 2, 2, 0, mk, reinterpret_cast<int32_t*>(dummy + 2), ws, nullptr), "aligned");
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, starts, 2, 2, 0, nullptr, ip, nullptr, nullptr), "null");  // a null mask alone is no refusal
    {   // a host array of exactly n entries: one read past it is a sanitizer report
        int32_t* three = new int32_t[3]{0, 1, -5};
        REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, three, 3, 2, 0, mk, ip, ws, nullptr), "negative");
        REFUSED(pc_clips_from_u8(u8, 20, 12, 12, 2, 2, 8, three, 3, 2, fp, nullptr), "negative");
        delete[] three;
    }
    starts[31] = -1;                                                  // the last of 32: the whole host array is walked
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, starts, 32, 2, 0, mk, ip, ws, nullptr), "negative");
    REFUSED(pc_clips_from_u8(u8, 20, 12, 12, 2, 2, 8, starts, 32, 2, fp, nullptr), "negative");
    starts[0] = INT_MIN;
    REFUSED(pc_detect_frames(fp, 20, 12, 12, 2, 2, 8, starts, 1, INT_MAX, 0, mk, ip, ws, nullptr), "negative");

    // pc_detect_frames_ws_bytes(n, S): host arithmetic only
    EXPECT(pc_detect_frames_ws_bytes(0, 8) == -1 && pc_detect_frames_ws_bytes(33, 8) == -1 && pc_detect_frames_ws_bytes(-1, 8) == -1);
    EXPECT(pc_detect_frames_ws_bytes(2, 0) == -1 && pc_detect_frames_ws_bytes(2, 6) == -1 && pc_detect_frames_ws_bytes(2, -4) == -1);
    EXPECT(pc_detect_frames_ws_bytes(2, 32772) == -1 && pc_detect_frames_ws_bytes(2, INT_MAX) == -1);
    EXPECT(pc_detect_frames_ws_bytes(1, 4) == 8 * 32);                                    // one block per frame, one 32-byte partial per block
    EXPECT(pc_detect_frames_ws_bytes(14, 224) == 14 * 8 * 13 * 32);                       // 12544 float4 per frame: 13 blocks of 1024
    EXPECT(pc_detect_frames_ws_bytes(32, 32768) == 32ll * 8 * 64 * 32);                   // at most 64 blocks per frame

    // pc_video_class(scores, n, C, out, s)
    REFUSED(pc_video_class(nullptr, 3, 24, fp, nullptr), "null");
    REFUSED(pc_video_class(fp, 3, 24, nullptr, nullptr), "null");
    REFUSED(pc_video_class(fp, 0, 24, fp, nullptr), "n = 0");
    REFUSED(pc_video_class(fp, -1, 24, fp, nullptr), "n = -1");
    REFUSED(pc_video_class(fp, 3, 0, fp, nullptr), "C = 0");
    REFUSED(pc_video_class(fp, 3, -7, fp, nullptr), "C = -7");
    REFUSED(pc_video_class(fp, 1 << 20, 1 << 20, fp, nullptr), "rows");        // n * C beyond int32

    if (fails) { std::printf("%d host-side checks failed\n", fails); return 1; }
    std::printf("detect host driver: all checks passed\n");
    return 0;
}
