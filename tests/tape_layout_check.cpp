// Stand-alone check of csrc/nlr_tape.h (plain C++, no HIP; built and run by tests/test_tape_layout.py):
//   * the walk of a GEMM visits every (row, col) of the padded matrix exactly once, in whole fragments, for both k widths and both RH;
//   * the GEMMs of the inference and training programs, walked one by one, give the fragment counts and positions of the program tables
//     the kernels take their constants from, and the bias blocks end where the tables say;
//   * nlr_tape_matches, the comparison behind the builders' run-time check, refuses a tape with one GEMM too many or too few and a bias
//     block one unit short, and names both numbers;
//   * the stacked heads put every layer where the kernels read it.
#include <stdio.h>
#include <string.h>

#include "../nerf-lidar_amd/csrc/nlr_tape.h"

static int failures = 0;
#define EXPECT(cond, ...)                     \
    do {                                      \
        if (!(cond)) {                        \
            ++failures;                       \
            printf("FAIL %s: ", #cond);       \
            printf(__VA_ARGS__);              \
            printf("\n");                     \
        }                                     \
    } while (0)

typedef TapeMat<int32_t, -1> IMat;
typedef TapeLinear<int32_t, -1> ILin;

// fragments of one GEMM [out_pad, in_pad]; every element of the padded matrix must come by exactly once
static int walk(uint32_t out_pad, uint32_t in_pad, uint32_t KW, uint32_t RH, uint32_t frags_per_step) {
    const uint32_t rows = RH == 2 ? out_pad : 16;
    IMat m(rows, in_pad);
    for (size_t i = 0; i < m.a.size(); ++i) m.a[i] = (int32_t)i;
    std::vector<int> seen(m.a.size(), 0);
    uint32_t frags = 0;
    nlr_tape_walk(m, out_pad, in_pad, KW, RH, [&](const int32_t *v, uint32_t n) {
        EXPECT(n * (KW == 32 ? 2 : 4) == NLR_FRAG_BYTES, "fragment of %u elements at k width %u", n, KW);
        for (uint32_t i = 0; i < n; ++i) {
            EXPECT(v[i] >= 0, "element outside the padded matrix");
            if (v[i] >= 0) ++seen[v[i]];
        }
        ++frags;
    });
    for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] != 1) {
            EXPECT(seen[i] == 1, "[%u x %u] KW %u RH %u: element (%zu, %zu) visited %d times", out_pad, in_pad, KW, RH, i / in_pad, i % in_pad, seen[i]);
            break;
        }
    return (int)(frags * frags_per_step);
}

static void inference(int W, int WB, int Fp, int HT, int D, int prec) {
    const bool fast = prec == NLR_PREC_FAST, f32 = prec == NLR_PREC_F32;
    const uint32_t tk = fast ? 32 : 16, tf = fast ? 2 : 1, vk = f32 ? 16 : 32;  // trunk / view k width, hi + lo fragments
    const int src = fast ? 64 : WB;                                              // what the heads and the view layers read
    const MlpProgram PG = nlr_mlp_program(W / 32, WB / 32, Fp / 32, HT, prec, 0);
    const int d0 = walk(64, Fp, tk, 2, tf), d2 = walk(fast ? 32 : WB, 64, tk, 2, tf);
    const int h1 = HT ? walk(32 * HT, src, tk, 2, tf) : 0, h2 = HT ? walk(32, 32 * HT, tk, 2, tf) : 0;
    const int v0 = walk(W, src + 32, vk, 2, 1), v1 = walk(W, W + src + 32, vk, 2, 1), hl = walk(W, W, vk, 2, 1), rgb = walk(16, W, vk, 1, 1);
    EXPECT(d0 == PG.FR_D0 && d2 == PG.FR_D2 && h1 == PG.FR_H1 && h2 == PG.FR_H2, "trunk / heads W%d HT%d prec%d: %d %d %d %d against %d %d %d %d", W,
           HT, prec, d0, d2, h1, h2, PG.FR_D0, PG.FR_D2, PG.FR_H1, PG.FR_H2);
    EXPECT(v0 == PG.FR_V0 && v1 == PG.FR_V1 && hl == PG.FR_HL && rgb == PG.FR_RGB, "view W%d prec%d: %d %d %d %d against %d %d %d %d", W, prec, v0, v1,
           hl, rgb, PG.FR_V0, PG.FR_V1, PG.FR_HL, PG.FR_RGB);
    const int T = d0 + d2 + h1 + h2, half = T + v0 + v1, tape = (f32 ? 1 : 2) * half + (D - 2) * hl + rgb;
    EXPECT(T == PG.FR_T && half == PG.FR_HALF, "T %d half %d against %d %d", T, half, PG.FR_T, PG.FR_HALF);
    EXPECT(tape == PG.frags(D), "W%d HT%d D%d prec%d: tape of %d fragments, program of %d", W, HT, D, prec, tape, PG.frags(D));
    char msg[256] = "", want[64];
    EXPECT(nlr_tape_matches("tape", tape, PG.frags(D), msg, sizeof(msg)) && !msg[0], "an exact tape is refused");
    EXPECT(!nlr_tape_matches("tape", tape + hl, PG.frags(D), msg, sizeof(msg)), "a hidden layer too many goes unnoticed");
    snprintf(want, sizeof(want), "built %d, the kernel's program has %d", tape + hl, PG.frags(D));
    EXPECT(strstr(msg, want) != nullptr, "message '%s' does not name both numbers (%s)", msg, want);
    EXPECT(!nlr_tape_matches("tape", tape - rgb, PG.frags(D), msg, sizeof(msg)), "a missing rgb_layer goes unnoticed");
    EXPECT(PG.F_HID == (f32 ? 1 : 2) * half && PG.F_END == PG.F_HID + rgb, "positions");
    if (fast) {
        const MlpProgram PL = nlr_mlp_program(W / 32, WB / 32, Fp / 32, HT, prec, 2);
        EXPECT(PL.frags(D) == 2 * T, "LiDAR-only tape of %d fragments, program of %d", 2 * T, PL.frags(D));
    }
    const int d2rows = fast ? 32 : WB, bias = 64 + d2rows + 32 * HT + 32 + D * W + 32;
    EXPECT(bias == PG.bias_end(D), "bias block of %d floats, table says %d", bias, PG.bias_end(D));
    EXPECT(!nlr_tape_matches("bias", bias - 32, PG.bias_end(D), msg, sizeof(msg)), "a bias block without the b_h2 slot goes unnoticed");
    EXPECT(PG.OB_D2 == 64 && PG.OB_H1 == 64 + d2rows && PG.OB_H2 == PG.OB_H1 + 32 * HT && PG.OB_V0 == PG.OB_H2 + 32 && PG.OB_V1 == PG.OB_V0 + W &&
               PG.OB_VL == PG.OB_V1 + W, "bias offsets");
}

static void training(int W, int WB, int HT, int D) {
    for (int view = 1; view >= 0; --view) {
        const TrainProgram PG = nlr_train_program(W / 32, WB / 32, 2, HT, view != 0);
        const int VW = view ? W : 0, HH = 32 * HT;
        int f = walk(64, 64, 32, 2, 1) + walk(WB, 64, 32, 2, 1);
        if (HH) f += walk(HH, WB, 32, 2, 1) + walk(32, HH, 32, 2, 1);
        EXPECT(f == PG.FR_T, "training trunk + heads %d against %d", f, PG.FR_T);
        if (view) {
            f += walk(W, WB + 32, 32, 2, 1) + walk(W, W + WB + 32, 32, 2, 1);
            EXPECT(f == PG.FF_HID, "FF_HID %d against %d", f, PG.FF_HID);
            for (int l = 2; l < D; ++l) f += walk(W, W, 32, 2, 1);
            f += walk(16, W, 32, 1, 1);
        }
        EXPECT(f == PG.fwd_frags(D), "W%d HT%d D%d view%d: forward tape of %d fragments, program of %d", W, HT, D, view, f, PG.fwd_frags(D));
        int b = 0;
        if (view) {
            b += walk(W, 32, 32, 2, 1);
            EXPECT(b == PG.BR_RGB && b == PG.BF_V1A, "RGB^T");
            for (int l = D - 1; l >= 2; --l) b += walk(W, W, 32, 2, 1);
            b += walk(W, W, 32, 2, 1);
        }
        EXPECT(b == PG.BF_H2 + (view ? (D - 2) * PG.FR_HL : 0), "BF_H2");
        if (HH) b += walk(HH, 32, 32, 2, 1);
        b += walk(WB, 2 * VW + HH + 32, 32, 2, 1) + walk(64, WB, 32, 2, 1) + walk(64, 64, 32, 2, 1);
        EXPECT(b == PG.bwd_frags(D), "W%d HT%d D%d view%d: backward tape of %d fragments, program of %d", W, HT, D, view, b, PG.bwd_frags(D));
        EXPECT(PG.bias_end(D) == 64 + WB + HH + 32 + D * W + 32, "training bias block");
    }
}

static void heads() {
    const uint32_t WB = 256, K = 5;
    auto lin = [](uint32_t rows, uint32_t cols, int32_t id) {
        ILin l;
        l.w = IMat(rows, cols);
        for (auto &x : l.w.a) x = id;
        l.b.assign(rows, id + 1);
        return l;
    };
    const ILin s0 = lin(64, WB, 10), s2 = lin(K, 64, 20), i0 = lin(64, WB, 30), i2 = lin(1, 64, 40), none;
    const TapeHeads<int32_t, -1> both = nlr_tape_heads<int32_t, -1>(WB, K, &s0, &s2, &i0, &i2);
    EXPECT(both.h1.rows == 128 && both.h2.rows == 32 && both.h2.cols == 128, "shapes of both heads");
    EXPECT(both.h1.get(0, 0) == 10 && both.h1.get(63, 255) == 10 && both.h1.get(64, 0) == 30 && both.h1.get(127, 255) == 30, "h1 = [sem0 ; int0]");
    EXPECT(both.h2.get(0, 0) == 20 && both.h2.get(K - 1, 63) == 20 && both.h2.get(K - 1, 64) == -1 && both.h2.get(K, 63) == -1 &&
               both.h2.get(K, 64) == 40 && both.h2.get(K, 127) == 40 && both.h2.get(K + 1, 64) == -1, "h2 block-diagonal, intensity row behind the class rows");
    EXPECT(both.b1[0] == 11 && both.b1[64] == 31 && both.b2[K - 1] == 21 && both.b2[K] == 41 && both.b2[K + 1] == -1, "bias rows");
    const TapeHeads<int32_t, -1> inten = nlr_tape_heads<int32_t, -1>(WB, 0, (const ILin *)nullptr, &none, &i0, &i2);
    EXPECT(inten.h1.get(0, 0) == 30 && inten.h2.get(0, 0) == 40 && inten.b2[0] == 41, "intensity alone sits in row 0");
    const TapeHeads<int32_t, -1> pass = nlr_tape_heads<int32_t, -1>(WB, K, &none, &none, (const ILin *)nullptr, &none);
    EXPECT(pass.h1.rows == 64 && pass.h1.get(0, 0) == -1 && pass.b1.size() == 64 && pass.b2.size() == 32, "an empty head keeps its rows absent");
    const TapeHeads<int32_t, -1> no = nlr_tape_heads<int32_t, -1>(WB, 0, (const ILin *)nullptr, &none, (const ILin *)nullptr, &none);
    EXPECT(no.h1.rows == 0 && no.b1.empty() && no.b2.size() == 32, "no heads: the b_h2 slot stays");
}

int main() {
    for (int W : {128, 256})
        for (int HT : {0, 2, 4})
            for (int D : {2, 3, 5}) {
                for (int prec : {NLR_PREC_F32, NLR_PREC_MIXED, NLR_PREC_FAST}) inference(W, 256, 64, HT, D, prec);
                training(W, 256, HT, D);
            }
    inference(256, 256, 96, 4, 2, NLR_PREC_FAST);  // three k-blocks of grid features
    heads();
    static_assert(NLR_CHUNK_BYTES == 32768 && NLR_CHUNK_BF16 == 16384, "chunk size");
    printf(failures ? "%d FAILURES\n" : "tape layout ok\n", failures);
    return failures ? 1 : 0;
}
