// Host-side checks of pc_val_metrics / pc_val_metrics_ws_floats / pc_val_record_words without a GPU, linked against the AddressSanitizer +
// UBSan build of the library (`make -C pi-consistency-activity-detection_amd/csrc asan/valmetrics_host_driver`): every call returns through the
// entry's own argument checks, in front of any HIP call, or is host arithmetic (record and workspace sizes), so an out-of-bounds access or
// undefined behaviour on the host side ends the process with a sanitizer report.  tests/test_valstep_cpu.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "picons.h"

static int fails = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { ++fails; std::printf("FAILED %s:%d  %s  [%s]\n", __FILE__, __LINE__, #cond, pc_last_error()); } \
    } while (0)

int main() {
    EXPECT(pc_version() == PC_VERSION);
    alignas(16) static char dummy[256];
    float* fp = reinterpret_cast<float*>(dummy);
    float* odd = reinterpret_cast<float*>(dummy + 4);
    int32_t* ip = reinterpret_cast<int32_t*>(dummy);

    // sizes: 10 + 3 B words; blocks per clip = ceil(pix / 4 / 1024) in [1, 256], per block 4 doubles + 4 int32, per clip 4 doubles more
    EXPECT(pc_val_record_words(1) == 13 && pc_val_record_words(16) == 58 && pc_val_record_words(0) == -1 && pc_val_record_words(-3) == -1);
    const long long shapes[][3] = {{1, 32, 1}, {3, 280, 1}, {2, 25088, 7}, {16, 6272, 2}, {16, 401408, 98}, {1, 4 * 1024 * 300, 256}};
    for (const auto& s : shapes) {
        const long long B = s[0], nbx = s[2];
        EXPECT(pc_val_metrics_ws_floats((int)B, s[1]) == 2 * (B * nbx * 4 + B * 4) + B * nbx * 4);
    }
    EXPECT(pc_val_metrics_ws_floats(0, 32) == -1 && pc_val_metrics_ws_floats(2, 30) == -1 && pc_val_metrics_ws_floats(2, 0) == -1);
    EXPECT(pc_val_metrics_ws_floats(2, -4) == -1 && pc_val_metrics_ws_floats(2, 1ll << 31) == -1 && pc_val_metrics_ws_floats(70000, 32) == -1);

    // every refusal comes before the first HIP call (there is no device here to make one on) and leaves a message
    EXPECT(pc_val_metrics(nullptr, fp, fp, ip, 2, 32, 24, ip, fp, nullptr) == PC_E_ARG && std::strstr(pc_last_error(), "null"));
    EXPECT(pc_val_metrics(fp, nullptr, fp, ip, 2, 32, 24, ip, fp, nullptr) == PC_E_ARG);
    EXPECT(pc_val_metrics(fp, fp, nullptr, ip, 2, 32, 24, ip, fp, nullptr) == PC_E_ARG);
    EXPECT(pc_val_metrics(fp, fp, fp, nullptr, 2, 32, 24, ip, fp, nullptr) == PC_E_ARG);
    EXPECT(pc_val_metrics(fp, fp, fp, ip, 2, 32, 24, nullptr, fp, nullptr) == PC_E_ARG);
    EXPECT(pc_val_metrics(fp, fp, fp, ip, 2, 32, 24, ip, nullptr, nullptr) == PC_E_ARG && std::strstr(pc_last_error(), "null"));
    EXPECT(pc_val_metrics(fp, fp, fp, ip, 0, 32, 24, ip, fp, nullptr) == PC_E_ARG && std::strstr(pc_last_error(), "B = 0"));
    EXPECT(pc_val_metrics(fp, fp, fp, ip, 70000, 32, 24, ip, fp, nullptr) == PC_E_ARG);
    EXPECT(pc_val_metrics(fp, fp, fp, ip, 2, 32, 0, ip, fp, nullptr) == PC_E_ARG && std::strstr(pc_last_error(), "C = 0"));
    EXPECT(pc_val_metrics(fp, fp, fp, ip, 65535, 32, 1 << 20, ip, fp, nullptr) == PC_E_ARG);              // B * C beyond int32
    EXPECT(pc_val_metrics(fp, fp, fp, ip, 2, 30, 24, ip, fp, nullptr) == PC_E_ARG && std::strstr(pc_last_error(), "multiple of 4"));
    EXPECT(pc_val_metrics(fp, fp, fp, ip, 2, 0, 24, ip, fp, nullptr) == PC_E_ARG);
    EXPECT(pc_val_metrics(fp, fp, fp, ip, 2, 1ll << 31, 24, ip, fp, nullptr) == PC_E_ARG);
    EXPECT(pc_val_metrics(odd, fp, fp, ip, 2, 32, 24, ip, fp, nullptr) == PC_E_ARG && std::strstr(pc_last_error(), "16-byte"));
    EXPECT(pc_val_metrics(fp, odd, fp, ip, 2, 32, 24, ip, fp, nullptr) == PC_E_ARG);
    EXPECT(pc_val_metrics(fp, fp, fp, ip, 2, 32, 24, ip, odd, nullptr) == PC_E_ARG && std::strstr(pc_last_error(), "16-byte"));
    EXPECT(pc_val_metrics(fp, fp, reinterpret_cast<float*>(dummy + 2), ip, 2, 32, 24, ip, fp, nullptr) == PC_E_ARG);
    {   // the op-list runner hands its operands to the same checks
        pc_op op;
        std::memset(&op, 0, sizeof op);
        op.kind = PC_OP_VAL_METRICS;
        op.i[0] = 2; op.i[1] = 24; op.l[0] = 32;
        EXPECT(pc_run_ops(&op, 1, nullptr) == PC_E_ARG && std::strstr(pc_last_error(), "pc_val_metrics"));
    }
    if (fails) { std::printf("%d host-side checks failed\n", fails); return 1; }
    std::printf("valmetrics host driver: all checks passed\n");
    return 0;
}
