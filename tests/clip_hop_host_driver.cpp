// Host-side checks of pc_clip_hop_starts / pc_clip_planes_bytes / pc_clip_planes / pc_detect_frames_planes_ws_bytes / pc_detect_frames_planes
// without a GPU, linked against the AddressSanitizer + UBSan build of the library (`make -C pi-consistency-activity-detection_amd/csrc
// asan/clip_hop_host_driver`): the starts entry writes exactly its count into heap arrays of exactly that size, and every call of the two
// launch entries returns through its own argument checks, in front of any HIP call, so an out-of-bounds access or undefined behaviour on the
// host side ends the process with a sanitizer report.  tests/test_clip_hop_cpu.py builds and runs it.
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
#define REFUSED(call, who, word) EXPECT((call) == PC_E_ARG && std::strstr(pc_last_error(), word) && std::strstr(pc_last_error(), who))

int main() {
    EXPECT(pc_version() == PC_VERSION && PC_VERSION >= 107);

    // pc_clip_hop_starts(F, f_skip, hop, starts, cap): host arithmetic only
    const int badhop[][3] = {{0, 2, 8}, {-1, 2, 8}, {17, 0, 8}, {17, -2, 8}, {17, 2, 0}, {17, 2, 1}, {17, 2, 3}, {17, 2, 18}, {17, 2, -2}, {17, 3, 4},
                             {17, (1 << 20) + 1, (1 << 20) + 1}, {17, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN}};
    for (const auto& b : badhop) EXPECT(pc_clip_hop_starts(b[0], b[1], b[2], nullptr, 0) == PC_E_ARG && std::strstr(pc_last_error(), "pc_clip_hop_starts"));
    EXPECT(pc_clip_hop_starts(INT_MAX, 1, 1, nullptr, 0) == (int64_t)INT_MAX - 7);       // 1 + (F - 8) windows of one clip: the count alone
    EXPECT(pc_clip_hop_starts(INT_MAX, 1 << 20, 1 << 20, nullptr, 0) == 2041ll << 20);      // 2041 windows of 2^20 phases each
    for (int fs = 1; fs <= 3; ++fs)
        for (int hop = fs; hop <= 8 * fs; hop += fs)
            for (int F = 1; F <= 119; ++F) {
                const int64_t n = pc_clip_hop_starts(F, fs, hop, nullptr, 0);
                EXPECT(n >= 1);
                int32_t* st = new int32_t[n];                            // exactly n entries: one written past them is a report
                for (int64_t i = 0; i < n; ++i) st[i] = -7;
                if (n > 1) EXPECT(pc_clip_hop_starts(F, fs, hop, st, n - 1) == n && st[0] == -7 && st[n - 2] == -7);      // too small: untouched
                EXPECT(pc_clip_hop_starts(F, fs, hop, st, n) == n);
                bool ok = st[0] == 0;
                for (int64_t i = 0; i < n; ++i) {
                    ok = ok && st[i] >= 0 && st[i] < F && st[i] % hop < fs && (i == 0 || st[i] > st[i - 1]);
                    ok = ok && (int64_t)(st[i] / hop) * fs + st[i] % hop == i;
                }
                ok = ok && st[n - 1] / hop * hop + 8 * fs >= F;          // the last window reaches the end
                EXPECT(ok);
                delete[] st;
            }

    // pc_clip_planes_bytes(F, Hs, Ws, f_skip, hop) and pc_detect_frames_planes_ws_bytes(nf, H, W): host arithmetic only
    EXPECT(pc_clip_planes_bytes(0, 8, 8, 2, 8) == -1 && pc_clip_planes_bytes(17, 0, 8, 2, 8) == -1 && pc_clip_planes_bytes(17, 8, -1, 2, 8) == -1);
    EXPECT(pc_clip_planes_bytes(17, 1 << 16, 1 << 15, 2, 8) == -1 && pc_clip_planes_bytes(17, 8, 8, 2, 7) == -1 && pc_clip_planes_bytes(17, 8, 8, 0, 0) == -1);
    EXPECT(pc_clip_planes_bytes(17, 8, 8, 2, 18) == -1 && pc_clip_planes_bytes(INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX) == -1);
    EXPECT(pc_clip_planes_bytes(17, 3, 3, 2, 8) == 2 * 17 * 12 * 4 + 12);                 // 9 pixels round up to 12; M = 2
    EXPECT(pc_clip_planes_bytes(40, 10, 12, 2, 6) == 3 * 40 * 120 * 4 + 120 && pc_clip_planes_bytes(40, 10, 12, 2, 2) == 8 * 40 * 120 * 4 + 120);
    EXPECT(pc_clip_planes_bytes(40, 10, 12, 2, 16) == 40 * 120 * 4 + 120);
    EXPECT(pc_clip_planes_bytes(1 << 20, 46340, 46340, 1, 8) == (1ll << 20) * 2147395600ll * 4 + 2147395600ll);
    EXPECT(pc_clip_planes_bytes(INT_MAX, 46340, 46340, 1, 1) == -1);                      // beyond 64 bits
    EXPECT(pc_detect_frames_planes_ws_bytes(0, 8, 8) == -1 && pc_detect_frames_planes_ws_bytes(PC_PLANES_MAX_FRAMES + 1, 8, 8) == -1);
    EXPECT(pc_detect_frames_planes_ws_bytes(1, 0, 8) == -1 && pc_detect_frames_planes_ws_bytes(1, 8, -3) == -1 && pc_detect_frames_planes_ws_bytes(1, 1 << 16, 1 << 15) == -1);
    EXPECT(pc_detect_frames_planes_ws_bytes(1, 9, 11) == 32 && pc_detect_frames_planes_ws_bytes(PC_PLANES_MAX_FRAMES, 240, 320) == 256 * 19 * 32);
    EXPECT(pc_detect_frames_planes_ws_bytes(3, 1080, 1920) == 3 * 64 * 32);

    alignas(16) static char dummy[256];
    float* fp = reinterpret_cast<float*>(dummy);
    float* odd = reinterpret_cast<float*>(dummy + 4);
    uint8_t* mk = reinterpret_cast<uint8_t*>(dummy);
    uint16_t* pb = reinterpret_cast<uint16_t*>(dummy);
    int32_t* ip = reinterpret_cast<int32_t*>(dummy);
    const int32_t* tb = reinterpret_cast<const int32_t*>(dummy);
    void* ws = dummy;
    int32_t starts[32];
    for (int c = 0; c < 32; ++c) starts[c] = (c / 2) * 8 + c % 2;       // the starts of hop 8 at f_skip 2
    const int32_t vw[2][3] = {{2, 2, 0}, {1, 3, 1}};                  // two good views of a 12 x 12 frame at S = 8
    const int32_t* views = &vw[0][0];

    // pc_clip_planes(logits, F, Hs, Ws, S, views, V, view_stride, starts, n, f_skip, hop, plane, cover, s)
    const char* cp = "pc_clip_planes";
#define PLANES(logits, F, Hs, Ws, S, views, V, stride, starts, n, f_skip, hop, plane, cover) \
    pc_clip_planes(logits, F, Hs, Ws, S, views, V, stride, starts, n, f_skip, hop, plane, cover, nullptr)
    REFUSED(PLANES(nullptr, 40, 12, 12, 8, views, 2, 2, starts, 2, 2, 8, fp, mk), cp, "null");
    REFUSED(PLANES(fp, 40, 12, 12, 8, nullptr, 2, 2, starts, 2, 2, 8, fp, mk), cp, "null");
    REFUSED(PLANES(fp, 40, 12, 12, 8, views, 2, 2, nullptr, 2, 2, 8, fp, mk), cp, "null");
    REFUSED(PLANES(fp, 40, 12, 12, 8, views, 2, 2, starts, 2, 2, 8, nullptr, mk), cp, "null");
    REFUSED(PLANES(fp, 40, 12, 12, 8, views, 2, 2, starts, 2, 2, 8, nullptr, nullptr), cp, "null");      // a null cover alone is no refusal
    REFUSED(PLANES(fp, 0, 12, 12, 8, views, 2, 2, starts, 2, 2, 8, fp, mk), cp, "outside");
    REFUSED(PLANES(fp, 40, 12, 12, 0, views, 2, 2, starts, 2, 2, 8, fp, mk), cp, "outside");
    REFUSED(PLANES(fp, 40, 12, 12, 16, views, 2, 2, starts, 2, 2, 8, fp, mk), cp, "outside");
    REFUSED(PLANES(fp, 40, 7, 12, 8, views, 2, 2, starts, 2, 2, 8, fp, mk), cp, "outside");
    REFUSED(PLANES(fp, 40, 12, 7, 8, views, 2, 2, starts, 2, 2, 8, fp, mk), cp, "outside");
    REFUSED(PLANES(fp, 40, 1 << 16, 1 << 16, 8, views, 2, 2, starts, 2, 2, 8, fp, mk), cp, "2^31");
    REFUSED(PLANES(fp, 40, 12, 12, 6, views, 2, 2, starts, 2, 2, 8, fp, mk), cp, "multiple of 4");
    REFUSED(PLANES(fp, 40, 12, 12, 8, views, 0, 2, starts, 2, 2, 8, fp, mk), cp, "views outside");
    REFUSED(PLANES(fp, 40, 12, 12, 8, views, 33, 2, starts, 2, 2, 8, fp, mk), cp, "views outside");
    REFUSED(PLANES(fp, 40, 12, 12, 8, views, 2, 1, starts, 2, 2, 8, fp, mk), cp, "view_stride");
    REFUSED(PLANES(fp, 40, 12, 12, 8, views, 2, 2, starts, 0, 2, 8, fp, mk), cp, "clips outside");
    REFUSED(PLANES(fp, 40, 12, 12, 8, views, 2, 40, starts, 33, 2, 8, fp, mk), cp, "clips outside");
    REFUSED(PLANES(fp, 40, 12, 12, 8, views, 2, 2, starts, 2, 0, 8, fp, mk), cp, "f_skip");
    const int hops[] = {0, 1, 7, 18, 32, -8, INT_MAX, INT_MIN};
    for (int h : hops) REFUSED(PLANES(fp, 40, 12, 12, 8, views, 2, 2, starts, 2, 2, h, fp, mk), cp, "hop");
    REFUSED(PLANES(fp, 40, 12, 12, 8, views, 2, 2, starts, 2, (1 << 20) + 1, (1 << 20) + 1, fp, mk), cp, "hop");
    REFUSED(PLANES(odd, 40, 12, 12, 8, views, 2, 2, starts, 2, 2, 8, fp, mk), cp, "16-byte");
    REFUSED(PLANES(fp, 40, 12, 12, 8, views, 2, 2, starts, 2, 2, 8, odd, mk), cp, "16-byte");
    REFUSED(PLANES(fp, 40, 12, 12, 8, views, 2, 2, starts, 2, 2, 8, fp, mk + 2), cp, "4-byte");
    {   // host arrays of exactly V * 3 and n entries: one read past either is a sanitizer report.  The bad view is the last of 32.
        int32_t* tab = new int32_t[32 * 3];
        const int32_t bad[][3] = {{5, 2, 0}, {2, 5, 0}, {-1, 2, 0}, {2, -1, 1}, {INT_MAX - 4, 0, 0}, {0, INT_MAX, 1}};
        for (const auto& b : bad) {
            for (int v = 0; v < 32; ++v) { tab[3 * v] = v % 5; tab[3 * v + 1] = v % 4; tab[3 * v + 2] = v & 1; }
            tab[93] = b[0]; tab[94] = b[1]; tab[95] = b[2];
            REFUSED(PLANES(fp, 40, 12, 12, 8, tab, 32, 2, starts, 2, 2, 8, fp, mk), cp, "outside");
        }
        const int32_t badflip[] = {2, -1, INT_MIN, 256};
        for (int fl : badflip) {
            tab[93] = 4; tab[94] = 4; tab[95] = fl;
            REFUSED(PLANES(fp, 40, 12, 12, 8, tab, 32, 2, starts, 2, 2, 8, fp, mk), cp, "flip");
        }
        tab[95] = 1;
        int32_t* three = new int32_t[3]{0, 1, -5};
        REFUSED(PLANES(fp, 40, 12, 12, 8, tab, 32, 3, three, 3, 2, 8, fp, mk), cp, "negative");
        three[2] = 2;                                                 // 2 % 8 >= f_skip: no start of the rule
        REFUSED(PLANES(fp, 40, 12, 12, 8, tab, 32, 3, three, 3, 2, 8, fp, mk), cp, "no clip start");
        three[2] = 32;                                                // window 4 of a 40-frame video at hop 8 is not kept (window 3 reaches the end)
        REFUSED(PLANES(fp, 40, 12, 12, 8, tab, 32, 3, three, 3, 2, 8, fp, mk), cp, "no clip start");
        three[0] = 40;                                                // the first clip holds no frame: no cover from this launch
        three[2] = 41;
        REFUSED(PLANES(fp, 40, 12, 12, 8, tab, 32, 3, three, 3, 2, 8, fp, mk), cp, "cover");
        delete[] three;
        delete[] tab;
    }
    starts[31] = -1;                                                  // the last of 32: the whole host array is walked
    REFUSED(PLANES(fp, 400, 12, 12, 8, views, 2, 32, starts, 32, 2, 8, fp, mk), cp, "negative");
    starts[31] = 15 * 8 + 2;
    REFUSED(PLANES(fp, 400, 12, 12, 8, views, 2, 32, starts, 32, 2, 8, fp, mk), cp, "no clip start");

    // pc_detect_frames_planes(plane, cover, F, H, W, Hs, Ws, V, f_skip, hop, f0, nf, row0, dev_tab, mask, prob, rec, ws, s)
    const char* dp = "pc_detect_frames_planes";
#define FRAMES(plane, cover, F, H, W, Hs, Ws, V, f_skip, hop, f0, nf, row0, tab, mask, prob, rec, ws) \
    pc_detect_frames_planes(plane, cover, F, H, W, Hs, Ws, V, f_skip, hop, f0, nf, row0, tab, mask, prob, rec, ws, nullptr)
    REFUSED(FRAMES(nullptr, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "null");
    REFUSED(FRAMES(fp, nullptr, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "null");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, 0, nullptr, mk, pb, ip, ws), dp, "null");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, nullptr, ws), dp, "null");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, nullptr), dp, "null");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, 0, tb, nullptr, nullptr, ip, nullptr), dp, "null");   // null mask and prob alone are no refusal
    REFUSED(FRAMES(fp, mk, 0, 9, 10, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "F = 0");
    REFUSED(FRAMES(fp, mk, 40, 0, 10, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "native");
    REFUSED(FRAMES(fp, mk, 40, 9, -3, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "native");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 0, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "working");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, INT_MIN, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "working");
    REFUSED(FRAMES(fp, mk, 40, 1 << 16, 1 << 15, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "2^31");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 1 << 16, 1 << 16, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "2^31");
    REFUSED(FRAMES(fp, mk, 40, 1 << 23, 1, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "2^24");
    REFUSED(FRAMES(fp, mk, 40, 1, 1 << 23, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "2^24");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 0, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "views outside");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 33, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "views outside");
    for (int h : hops) REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, h, 0, 40, 0, tb, mk, pb, ip, ws), dp, "hop");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 0, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "hop");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, -1, 40, 0, tb, mk, pb, ip, ws), dp, "outside the video");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 0, 0, tb, mk, pb, ip, ws), dp, "outside the video");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 41, 0, tb, mk, pb, ip, ws), dp, "outside the video");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, 39, 2, 0, tb, mk, pb, ip, ws), dp, "outside the video");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, INT_MAX, INT_MAX, 0, tb, mk, pb, ip, ws), dp, "outside the video");
    REFUSED(FRAMES(fp, mk, 400, 9, 10, 12, 12, 2, 2, 8, 0, PC_PLANES_MAX_FRAMES + 1, 0, tb, mk, pb, ip, ws), dp, "outside the video");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, -1, tb, mk, pb, ip, ws), dp, "row0");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, INT_MAX - 15, tb, mk, pb, ip, ws), dp, "row0");      // 8 clips of 2 views: 16 rows
    REFUSED(FRAMES(odd, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "aligned");
    REFUSED(FRAMES(fp, mk + 1, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, ws), dp, "aligned");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, 0, reinterpret_cast<const int32_t*>(dummy + 2), mk, pb, ip, ws), dp, "aligned");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, reinterpret_cast<int32_t*>(dummy + 2), ws), dp, "aligned");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, pb, ip, dummy + 4), dp, "aligned");
    REFUSED(FRAMES(fp, mk, 40, 9, 10, 12, 12, 2, 2, 8, 0, 40, 0, tb, mk, reinterpret_cast<uint16_t*>(dummy + 1), ip, ws), dp, "2-byte");

    if (fails) { std::printf("%d host-side checks failed\n", fails); return 1; }
    std::printf("clip hop host driver: all checks passed\n");
    return 0;
}
