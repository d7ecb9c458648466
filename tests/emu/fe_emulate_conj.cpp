// tests/emu/fe_emulate_conj.cpp -- host-side lane emulator for the conjugate form of phase A (lele_amd/csrc/fe_core.h:
// phase_a_conj, tw_conj_image), test infrastructure beside fe_emulate.cpp.  It runs what the HIP kernel runs for the 16 lanes of one
// frame -- phase_a_conj, the exchange's addressing, phase_b on the conjugated table image -- and returns the bins as the lanes hold
// them: `re`, the STORED imaginary part (-im where the lane's class is primed), and the power the kernel would compute from the stored
// pair.  tests/test_fe_core_conj.py un-primes by class and compares with the oracle's restatement of the reference FFT.
#include <math.h>
#include <string.h>
#include <vector>
#include "../../lele_amd/csrc/fe_core.h"

extern "C" int fe_conj_primed(int r) { return fe::primed(r) ? 1 : 0; }

// the library's own host routine for the table image phase B reads in this form
extern "C" void fe_conj_tw_image(const float* tw_re, const float* tw_im, int n, float* out /* 2 n */) { fe::tw_conj_image(tw_re, tw_im, n, out); }

// fe::power of n (re, im) pairs: what the kernel computes from a normal pair, for the bit-for-bit comparison of the powers
extern "C" void fe_conj_power(const float* re, const float* im, int n, float* out) {
    for (int i = 0; i < n; ++i) out[i] = fe::power(fe::cmk(re[i], im[i]));
}

extern "C" void fe_emulate_conj_fft512(const float* frame /*512, zero padded*/, const float* tw_re, const float* tw_im /* 511 */,
                                       float* out_re /*257*/, float* out_im_stored /*257*/, float* out_pw /*257*/) {
    using namespace fe;
    std::vector<float> img(2 * 511);
    tw_conj_image(tw_re, tw_im, 511, img.data());
    std::vector<cf> a(kLanes * kRegs);
    for (int p = 0; p < kLanes; ++p) {
        float x[kRegs];
        for (int r = 0; r < kRegs; ++r) x[r] = frame[16 * rev5(r) + p];
        phase_a_conj(x, &a[p * kRegs], tw_re, tw_im);
    }
    for (int k = 0; k < kBins; ++k) out_re[k] = out_im_stored[k] = out_pw[k] = nanf("");
    auto twf = [&](int i) { return cmk(img[2 * i], img[2 * i + 1]); };
    for (int rho = 0; rho < 2; ++rho) {
        std::vector<cf> lds(16 * kXchgPitch, cmk(nanf(""), nanf("")));
        for (int p = 0; p < kLanes; ++p) {
            int h = rev4(p);
            for (int cc = 0; cc < 16; ++cc) lds[xchg_slot(h, cc)] = a[p * kRegs + rho * 16 + cc];
        }
        for (int c = 0; c < kLanes; ++c) {
            cf b[16];
            for (int v = 0; v < 16; ++v) b[v] = lds[xchg_slot(v, c)];
            float re256 = 0.0f;
            phase_b(b, c, rho, twf, &re256);
            for (int v = 0; v < 8; ++v) {
                int j = (2 * v + rho) * 16 + c;
                cf z = b[v];
                if (j == 0) z = cmk(z.x, 0.0f);  // kernels/fft.rs:256-257
                out_re[j] = z.x;
                out_im_stored[j] = z.y;
                out_pw[j] = power(z);
            }
            if (c == 0 && rho == 0) {
                out_re[256] = re256;
                out_im_stored[256] = 0.0f;
                out_pw[256] = power(re256, 0.0f);
            }
        }
    }
}
