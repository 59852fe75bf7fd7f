// Host-side checks of PC_F_BKMAJOR (K-major weight planes for the bf16-split conv kernel) and pc_wino_weights_multi without a GPU, linked
// against the AddressSanitizer + UBSan build of the library (`make -C pi-consistency-activity-detection_amd/csrc asan/bkmajor_host_driver`):
// every call returns through the library's own descriptor checks or is host arithmetic (tile choice, tail split, variant string), so an
// out-of-bounds access or undefined behaviour on the host side ends the process with a sanitizer report.  tests/test_bkmajor_host_cpu.py
// builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "picons.h"

static int fails = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { ++fails; std::printf("FAILED %s:%d  %s  [%s]\n", __FILE__, __LINE__, #cond, pc_last_error()); } \
    } while (0)

// grouped 1 x 9 x 1 input gradient with mirrored taps (the spectral PrimaryCaps form): [G * nf][20][K] -> [G * nf][28][N]
static pc_conv_desc dgrad(int G, int nf, int K, int N, bool fwd_planes) {
    pc_conv_desc d;
    std::memset(&d, 0, sizeof(d));
    d.N = G * nf; d.Ti = 1; d.Hi = 20; d.Wi = 1; d.Ci = K; d.ldi = K;
    d.Tq = 1; d.Hq = 28; d.Wq = 1; d.To = 1; d.Ho = 28; d.Wo = 1; d.Co = N; d.ldo = N;
    for (int i = 0; i < 3; ++i) { d.ostr[i] = 1; d.istr[i] = 1; d.ntap[i] = 1; d.istep[i] = -1; d.wkstep[i] = 1; }
    d.ntap[1] = 9; d.KT = 1; d.KH = 9; d.KW = 1;
    d.ldw = fwd_planes ? N : K;
    d.flags = PC_F_X6 | PC_F_NFAST | (fwd_planes ? PC_F_BKMAJOR : 0);
    d.wgstride = K * 9 * N; d.groups = G;
    return d;
}

int main() {
    EXPECT(pc_version() == PC_VERSION);
    char name[160], ref[160], tiny[6];
    alignas(16) static char dummy[256];
    float* fp = reinterpret_cast<float*>(dummy);
    const uint16_t* hp = reinterpret_cast<const uint16_t*>(dummy);

    // the flag changes neither the tile, nor the tail split, nor the reported variant -- for every tile it is built for
    const int shapes[][4] = {{4, 2, 96, 160}, {41, 2, 96, 416}, {41, 4, 96, 224}, {41, 16, 544, 832}, {41, 4, 544, 832}};
    const char* tiles[] = {"x6:64x64:", "x6:64x128:", "x6:128x64:", "x6:64x128:", "x6:128x64:"};
    for (int c = 0; c < 5; ++c) {
        const pc_conv_desc f = dgrad(shapes[c][0], shapes[c][1], shapes[c][2], shapes[c][3], true), t = dgrad(shapes[c][0], shapes[c][1], shapes[c][2], shapes[c][3], false);
        EXPECT(pc_conv_x6_ok(&f) == pc_conv_x6_ok(&t));
        const long long nws = pc_conv_x6_ws_floats(&t);
        EXPECT(pc_conv_x6_ws_floats(&f) == nws);
        EXPECT(pc_conv_variant(&t, 0, ref, (int)sizeof ref) == PC_OK && std::strstr(ref, tiles[c]) == ref);
        EXPECT(pc_conv_variant(&f, 0, name, (int)sizeof name) == PC_OK && std::strcmp(name, ref) == 0);
        EXPECT(std::strstr(name, "major") == nullptr);                                     // the reporter does not print the flag
        if (nws > 0) {
            EXPECT(pc_conv_variant(&t, nws, ref, (int)sizeof ref) == PC_OK && pc_conv_variant(&f, nws, name, (int)sizeof name) == PC_OK && std::strcmp(name, ref) == 0);
            EXPECT(pc_conv_variant(&f, nws - 1, name, (int)sizeof name) == PC_E_ARG);      // a short workspace is refused as without the flag
        }
        EXPECT(pc_conv_variant(&f, 0, tiny, (int)sizeof tiny) == PC_E_ARG);                // never beyond `cap`
        double wf[7], wt[7];
        EXPECT(pc_conv_work(&f, 0, 0, wf) == PC_OK && pc_conv_work(&t, 0, 0, wt) == PC_OK && std::memcmp(wf, wt, sizeof wf) == 0);
        EXPECT(pc_conv_bnpart_rows(&f) == pc_conv_bnpart_rows(&t));
        // the launch's own checks, in front of any GPU call
        EXPECT(pc_conv_fwd_x6(&f, nullptr, hp, 8, nullptr, nullptr, fp, nullptr, nullptr) == PC_E_ARG);
        EXPECT(pc_conv_fwd_x6(&f, fp, hp, 12, nullptr, nullptr, fp, nullptr, nullptr) == PC_E_ARG);          // plane stride not a multiple of 8
        if (nws > 0)                                                                                              // a workspace too small for the split
            EXPECT(pc_conv_fwd_x6_ws(&f, fp, hp, (int64_t)shapes[c][0] * f.wgstride, nullptr, nullptr, fp, nullptr, fp, 1, nullptr) == PC_E_ARG);
    }
    {   // a tile the K-major fetch is not built for: 32 output channels take 128 x 32
        pc_conv_desc f = dgrad(4, 2, 96, 32, true);
        EXPECT(pc_conv_variant(&f, 0, name, (int)sizeof name) == PC_E_ARG && std::strstr(pc_last_error(), "128 x 32") != nullptr);
        EXPECT(pc_conv_fwd_x6(&f, fp, hp, 4 * 96 * 9 * 32, nullptr, nullptr, fp, nullptr, nullptr) == PC_E_ARG && std::strstr(pc_last_error(), "PC_F_BKMAJOR") != nullptr);
        f.flags &= ~PC_F_BKMAJOR; f.ldw = 96;
        EXPECT(pc_conv_variant(&f, 0, name, (int)sizeof name) == PC_OK && std::strstr(name, "x6:128x32:") == name);
        // 256 x 128 (a launch of many full rounds of 8-wave blocks)
        const pc_conv_desc b = dgrad(41, 64, 544, 1024, true), bt = dgrad(41, 64, 544, 1024, false);
        if (pc_conv_variant(&bt, 0, ref, (int)sizeof ref) == PC_OK && std::strstr(ref, "x6:256x128:") == ref)
            EXPECT(pc_conv_variant(&b, 0, name, (int)sizeof name) == PC_E_ARG);
        // output channels that are no multiple of 8, or rows shorter than the output channels
        pc_conv_desc o = dgrad(4, 2, 96, 164, true);
        o.ldw = 168;
        EXPECT(pc_conv_variant(&o, 0, name, (int)sizeof name) == PC_E_ARG && std::strstr(pc_last_error(), "Co % 8") != nullptr);
        o = dgrad(4, 2, 96, 160, true);
        o.ldw = 152;
        EXPECT(pc_conv_variant(&o, 0, name, (int)sizeof name) == PC_E_ARG);
        // the flag without PC_F_X6 means nothing to pc_conv_fwd's reporter and is not an x6 launch
        o = dgrad(4, 2, 96, 160, true);
        o.flags &= ~PC_F_X6;
        EXPECT(pc_conv_x6_ok(&o) == 0 && pc_conv_x6_ws_floats(&o) == 0);
    }
    {   // pc_wino_weights_multi: every job is checked before the pack's launch
        pc_wino_weights_job j[2];
        std::memset(j, 0, sizeof j);
        EXPECT(pc_wino_weights_multi(nullptr, 1, nullptr) == PC_E_ARG && pc_wino_weights_multi(j, 0, nullptr) == PC_E_ARG);
        j[0].w = j[0].U = (uint64_t)(uintptr_t)fp; j[0].sO = 64 * 27; j[0].sT = 1; j[0].sI = 27; j[0].O = 64; j[0].I = 64; j[0].KT = 3; j[0].m = 2;
        j[1] = j[0];
        j[1].I = 12;
        EXPECT(pc_wino_weights_multi(j, 2, nullptr) == PC_E_ARG && std::strstr(pc_last_error(), "bad job 1") != nullptr);
        j[1].I = 64; j[1].m = 3;
        EXPECT(pc_wino_weights_multi(j, 2, nullptr) == PC_E_ARG);
        j[1].m = 4; j[1].U = 0;
        EXPECT(pc_wino_weights_multi(j, 2, nullptr) == PC_E_ARG);
        pc_op op;
        std::memset(&op, 0, sizeof op);
        op.kind = PC_OP_WINO_WEIGHTS_MULTI;                                                 // the runner hands a null job table to the same checks
        EXPECT(pc_run_ops(&op, 1, nullptr) == PC_E_ARG);
    }
    if (fails) { std::printf("%d host-side checks failed\n", fails); return 1; }
    std::printf("bkmajor host driver: all checks passed\n");
    return 0;
}
