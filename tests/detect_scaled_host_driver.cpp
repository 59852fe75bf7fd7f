// Host-side checks of pc_resample_tables / pc_detect_frames_scaled_ws_bytes / pc_detect_frames_scaled without a GPU, linked against the
// AddressSanitizer + UBSan build of the library (`make -C pi-consistency-activity-detection_amd/csrc asan/detect_scaled_host_driver`): the
// table builder writes exactly 2 * (H + W) words into heap arrays of exactly that size, and every call of the launch entry returns through
// its own argument checks, in front of any HIP call, so an out-of-bounds access or undefined behaviour on the host side ends the process
// with a sanitizer report.  tests/test_detect_scaled_cpu.py builds and runs it.
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
#define REFUSED(call, word) EXPECT((call) == PC_E_ARG && std::strstr(pc_last_error(), word) && std::strstr(pc_last_error(), "pc_detect_frames_scaled"))

static float as_float(int32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

int main() {
    EXPECT(pc_version() == PC_VERSION && PC_VERSION >= 107);

    // pc_resample_tables(Hs, Ws, H, W, tab, cap): host arithmetic only
    EXPECT(pc_resample_tables(0, 4, 4, 4, nullptr, 0) == PC_E_ARG && std::strstr(pc_last_error(), "pc_resample_tables"));
    EXPECT(pc_resample_tables(4, 0, 4, 4, nullptr, 0) == PC_E_ARG && pc_resample_tables(4, 4, 0, 4, nullptr, 0) == PC_E_ARG);
    EXPECT(pc_resample_tables(4, 4, 4, -1, nullptr, 0) == PC_E_ARG && pc_resample_tables(INT_MIN, 4, 4, 4, nullptr, 0) == PC_E_ARG);
    EXPECT(pc_resample_tables(4, 4, 1 << 23, 4, nullptr, 0) == PC_E_ARG && pc_resample_tables(4, 4, 4, 1 << 23, nullptr, 0) == PC_E_ARG);
    EXPECT(pc_resample_tables(4, 4, INT_MAX, INT_MAX, nullptr, 0) == PC_E_ARG);
    EXPECT(pc_resample_tables(INT_MAX, INT_MAX, (1 << 23) - 1, 1, nullptr, 0) == 2ll * (1 << 23));      // the source has no bound of its own
    const int cases[][4] = {{1, 1, 1, 1}, {1, 5, 5, 1}, {8, 5, 5, 8}, {256, 256, 240, 320}, {256, 256, 1080, 1920}, {INT_MAX, 3, 7, (1 << 23) - 1}};
    for (const auto& c : cases) {
        const int64_t n = pc_resample_tables(c[0], c[1], c[2], c[3], nullptr, 0);
        EXPECT(n == 2ll * ((int64_t)c[2] + c[3]));
        int32_t* tab = new int32_t[n];                                   // exactly n words: one written past them is a report
        for (int64_t i = 0; i < n; ++i) tab[i] = 7;
        EXPECT(pc_resample_tables(c[0], c[1], c[2], c[3], tab, n - 1) == n && tab[0] == 7 && tab[n - 2] == 7);      // too small: untouched
        EXPECT(pc_resample_tables(c[0], c[1], c[2], c[3], tab, n) == n);
        bool ok = true;
        for (int axis = 0; axis < 2; ++axis) {
            const int L = c[axis], D = c[2 + axis];
            const int32_t* t = tab + (axis ? 2 * (int64_t)c[2] : 0);
            for (int d = 0; d < D; ++d) {
                const float w = as_float(t[2 * d + 1]);
                ok = ok && t[2 * d] >= 0 && t[2 * d] <= L - 1 && w >= 0.0f && w < 1.0f && (w == 0.0f || t[2 * d] < L - 1);
                if (L == D) ok = ok && t[2 * d] == d && t[2 * d + 1] == 0;                                         // the identity
            }
        }
        EXPECT(ok);
        delete[] tab;
    }

    // pc_detect_frames_scaled_ws_bytes(n, Hs, Ws, H, W): host arithmetic only
    EXPECT(pc_detect_frames_scaled_ws_bytes(0, 8, 8, 8, 8) == -1 && pc_detect_frames_scaled_ws_bytes(33, 8, 8, 8, 8) == -1);
    EXPECT(pc_detect_frames_scaled_ws_bytes(2, 0, 8, 8, 8) == -1 && pc_detect_frames_scaled_ws_bytes(2, 8, -1, 8, 8) == -1);
    EXPECT(pc_detect_frames_scaled_ws_bytes(2, 8, 8, 0, 8) == -1 && pc_detect_frames_scaled_ws_bytes(2, 8, 8, 8, 0) == -1);
    EXPECT(pc_detect_frames_scaled_ws_bytes(2, 1 << 16, 1 << 15, 8, 8) == -1 && pc_detect_frames_scaled_ws_bytes(2, 8, 8, 1 << 16, 1 << 15) == -1);
    EXPECT(pc_detect_frames_scaled_ws_bytes(2, 8, 8, 1 << 23, 1) == -1 && pc_detect_frames_scaled_ws_bytes(2, INT_MAX, INT_MAX, INT_MAX, INT_MAX) == -1);
    EXPECT(pc_detect_frames_scaled_ws_bytes(1, 3, 3, 9, 11) == 8 * 32 + 16 + 8 * 12 * 5);                 // 9 working pixels round up to 12
    EXPECT(pc_detect_frames_scaled_ws_bytes(32, 256, 256, 240, 320) == 32ll * 8 * 19 * 32 + 16 + 32ll * 8 * 65536 * 5);
    EXPECT(pc_detect_frames_scaled_ws_bytes(32, 46340, 46340, 1080, 1920) == 32ll * 8 * 64 * 32 + 16 + 32ll * 8 * 2147395600ll * 5);

    // pc_detect_frames_scaled(logits, F, H, W, Hs, Ws, S, views, V, view_stride, starts, n, f_skip, row0, dev_tab, mask, prob, rec, ws, s)
    alignas(16) static char dummy[256];
    float* fp = reinterpret_cast<float*>(dummy);
    float* odd = reinterpret_cast<float*>(dummy + 4);
    uint8_t* mk = reinterpret_cast<uint8_t*>(dummy);
    uint16_t* pb = reinterpret_cast<uint16_t*>(dummy);
    int32_t* ip = reinterpret_cast<int32_t*>(dummy);
    const int32_t* tb = reinterpret_cast<const int32_t*>(dummy);
    void* ws = dummy;
    int32_t starts[32];
    for (int c = 0; c < 32; ++c) starts[c] = c;
    const int32_t vw[2][3] = {{2, 2, 0}, {1, 3, 1}};                  // two good views of a 12 x 12 working frame at S = 8
    const int32_t* views = &vw[0][0];
#define SCALED(logits, F, H, W, Hs, Ws, S, views, V, stride, starts, n, f_skip, row0, tab, mask, prob, rec, ws) \
    pc_detect_frames_scaled(logits, F, H, W, Hs, Ws, S, views, V, stride, starts, n, f_skip, row0, tab, mask, prob, rec, ws, nullptr)
    REFUSED(SCALED(nullptr, 20, 9, 10, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "null");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, nullptr, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "null");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 2, nullptr, 2, 2, 0, tb, mk, pb, ip, ws), "null");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, nullptr, mk, pb, ip, ws), "dev_tab");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, nullptr, ws), "null");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, nullptr), "null");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, nullptr, nullptr, ip, nullptr), "null");   // null mask and prob alone are no refusal
    REFUSED(SCALED(fp, 0, 9, 10, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "outside");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 0, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "outside");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 16, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "outside");
    REFUSED(SCALED(fp, 20, 9, 10, 7, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "outside");               // the WORKING frame below the crop
    REFUSED(SCALED(fp, 20, 9, 10, 12, 7, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "outside");
    REFUSED(SCALED(fp, 20, 9, 10, 1 << 16, 1 << 16, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "2^31");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 6, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "multiple of 4");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 0, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "views outside");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 33, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "views outside");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 1, starts, 2, 2, 0, tb, mk, pb, ip, ws), "view_stride");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 2, starts, 0, 2, 0, tb, mk, pb, ip, ws), "clips outside");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 40, starts, 33, 2, 0, tb, mk, pb, ip, ws), "clips outside");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 2, starts, 2, 0, 0, tb, mk, pb, ip, ws), "f_skip");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 2, starts, 2, 2, -1, tb, mk, pb, ip, ws), "row0");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 2, starts, 2, 2, INT_MAX - 1000, tb, mk, pb, ip, ws), "row0");
    REFUSED(SCALED(odd, 20, 9, 10, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "16-byte");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, dummy + 4), "aligned");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, reinterpret_cast<int32_t*>(dummy + 2), ws), "aligned");
    // the native frame and prob: the entry's own
    REFUSED(SCALED(fp, 20, 0, 10, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "native");
    REFUSED(SCALED(fp, 20, 9, -3, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "native");
    REFUSED(SCALED(fp, 20, 1 << 16, 1 << 15, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "2^31");
    REFUSED(SCALED(fp, 20, 1 << 23, 1, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "2^24");
    REFUSED(SCALED(fp, 20, 1, 1 << 23, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "2^24");
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 2, starts, 2, 2, 0, tb, mk, reinterpret_cast<uint16_t*>(dummy + 1), ip, ws), "2-byte");

    {   // host arrays of exactly V * 3 and n entries: one read past either is a sanitizer report.  The bad view is the last of 32.
        int32_t* tab = new int32_t[32 * 3];
        int32_t* three = new int32_t[3]{0, 1, -5};
        const int32_t bad[][3] = {{5, 2, 0}, {2, 5, 0}, {-1, 2, 0}, {2, -1, 1}, {INT_MAX - 4, 0, 0}, {0, INT_MAX, 1}};
        for (const auto& b : bad) {
            for (int v = 0; v < 32; ++v) { tab[3 * v] = v % 5; tab[3 * v + 1] = v % 4; tab[3 * v + 2] = v & 1; }
            tab[93] = b[0]; tab[94] = b[1]; tab[95] = b[2];
            REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, tab, 32, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "outside");
        }
        const int32_t badflip[] = {2, -1, INT_MIN, 256};
        for (int fl : badflip) {
            tab[93] = 4; tab[94] = 4; tab[95] = fl;
            REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, tab, 32, 2, starts, 2, 2, 0, tb, mk, pb, ip, ws), "flip");
        }
        tab[95] = 1;
        REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, tab, 32, 3, three, 3, 2, 0, tb, mk, pb, ip, ws), "negative");
        delete[] three;
        delete[] tab;
    }
    starts[31] = -1;                                                  // the last of 32: the whole host array is walked
    REFUSED(SCALED(fp, 20, 9, 10, 12, 12, 8, views, 2, 32, starts, 32, 2, 0, tb, mk, pb, ip, ws), "negative");

    if (fails) { std::printf("%d host-side checks failed\n", fails); return 1; }
    std::printf("detect scaled host driver: all checks passed\n");
    return 0;
}
