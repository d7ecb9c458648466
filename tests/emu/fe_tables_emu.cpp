// tests/emu/fe_tables_emu.cpp -- host-side view of the compile-time tables of lele_amd/csrc/fe_core.h (test infrastructure):
// the constant twiddles of phase_a_fast and the LDS layout of the default mel bank.  tests/test_frontend_tables.py drives it.
// Also the host's choice of the fused kernel's form (fe::select_form), which tests/test_frontend_form.py enumerates.
#include <math.h>
#include <string.h>
#include "../../lele_amd/csrc/fe_core.h"

extern "C" {

int fe_tw_const_n() { return fe::kTwConstN; }
int fe_tw_const_used(int i) { return fe::tw_const_used(i) ? 1 : 0; }
// the constants as the accessor hands them out (entries 0 .. kTwConstN - 1)
void fe_tw_const(float* re, float* im) {
    for (int i = 0; i < fe::kTwConstN; ++i) {
        re[i] = fe::TwConst{false}[i];
        im[i] = fe::TwConst{true}[i];
    }
}
int fe_tw_const_matches(const float* tw_re, const float* tw_im) { return fe::tw_const_matches(tw_re, tw_im) ? 1 : 0; }

// the reference's table with the host's libm (kernels/fft.rs:136-157, as the library's host code builds it): 511 entries
void fe_host_twiddles512(float* re, float* im) {
    const float pi = 3.14159265358979323846264338327950288f;
    int o = 0;
    for (int size = 2; size <= 512; size *= 2) {
        const int half = size / 2, step = 512 / size;
        for (int k = 0; k < half; ++k, ++o) {
            const float angle = -2.0f * pi * (float)(k * step) / 512.0f;
            re[o] = cosf(angle);
            im[o] = sinf(angle);
        }
    }
}

// phase_a_fast on the 32 real inputs of one lane: out_table with the table accessor, out_const with the constants; (re, im) interleaved
void fe_phase_a_fast_both(const float* x, const float* tw_re, const float* tw_im, float* out_table, float* out_const) {
    fe::cf a[fe::kRegs], b[fe::kRegs];
    fe::phase_a_fast(x, a, tw_re, tw_im);
    fe::phase_a_fast(x, b, fe::TwConst{false}, fe::TwConst{true});
    for (int r = 0; r < fe::kRegs; ++r) {
        out_table[2 * r] = a[r].x, out_table[2 * r + 1] = a[r].y;
        out_const[2 * r] = b[r].x, out_const[2 * r + 1] = b[r].y;
    }
}

int fe_mel_lds_weights() { return fe::kMelLdsWeights; }
int fe_mel_lds_chunks() { return fe::kMelLdsChunks; }
int fe_mel_lds_index(int s, int p) { return fe::mel_lds_index(s, p); }

// fe::select_form (tests/test_frontend_form.py): out = {mode, std_mel, fused, opt}
void fe_select_form(int std_mel, int const_match, int const_tw, int lds_tables, int lean, int conj, int dpp, int fused, int* out) {
    const fe::FeForm f = fe::select_form(std_mel != 0, const_match != 0, const_tw != 0, lds_tables != 0, lean != 0, conj != 0, dpp, fused != 0);
    out[0] = f.mode, out[1] = f.std_mel, out[2] = f.fused, out[3] = f.opt;
}
}
