// fe_core.h -- per-lane arithmetic of the 512-point front-end FFT, shared by the HIP kernel
// (frontend.hip) and by the host-side lane emulator used in tests (tests/emu/fe_emulate.cpp).
//
// The reference computes a full 512-point complex radix-2 DIT FFT on the real frame
// (/root/reference/src/kernels/fft.rs:172-266, x86 AVX2 branch).  Its f32 round-off noise is
// comparable to the weakest bins of a high-dynamic-range frame, so agreeing with it to 1e-4
// requires reproducing the SAME butterfly network with the SAME roundings:
//   stages 1,2 (half_size 1,2  -> scalar tail, fft.rs:236-250):  tr = wr*or - wi*oi (two roundings + sub)
//   stages 3..9 (half_size>=4 -> SSE/AVX, fft.rs:192-234):        tr = fma(wr,or, -(wi*oi)), ti = fma(wr,oi, wi*or)
// and the same twiddle table values (cosf/sinf of the f32 angle, fft.rs:136-157).
//
// Mapping of the 512 positions j (after bit reversal) onto a 16-lane group holding 32 points per lane:
//   phase A  lane p (0..15), h = rev4(p) = j[8:5], register r = j[4:0]; input sample n = 16*rev5(r) + p.
//            stages 1..5 pair register bits 0..4; twiddle index k = r mod half (wave-uniform).
//   exchange (LDS), two rounds rho = r>>4:  register r of lane h  ->  lane c = r&15, register v = h.
//   phase B  lane c = j[3:0], register v = j[8:5], rho = j[4]; stages 6..9 pair register bits 0..3 of v;
//            twiddle index k = (v mod 2^(s-6))*32 + rho*16 + c (per lane, fetched from the table).
//            Only bins 0..256 are needed: stage 9 computes the '+' outputs (v<8) and, for (c=0,rho=0), bin 256.
//
// Complex values are (re, im) pairs in ONE two-element vector so that gfx950's packed-f32 VALU ops
// (v_pk_mul/add/fma_f32, each IEEE-exact per element) do a whole complex add or half a complex multiply per
// instruction; the host build uses a plain struct with the same element-wise semantics.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FE_HD __host__ __device__ __forceinline__
#else
#define FE_HD inline
#endif

namespace fe {

constexpr int kNfft = 512;
constexpr int kFrame = 400;
constexpr int kHop = 160;
constexpr int kBins = 257;
constexpr int kLanes = 16;   // lanes per frame
constexpr int kRegs = 32;    // points per lane
constexpr int kQ = 25;       // samples per lane that are inside the 400-sample frame (q = 0..24)

FE_HD constexpr int rev4(int x) { return ((x & 1) << 3) | ((x & 2) << 1) | ((x & 4) >> 1) | ((x & 8) >> 3); }
FE_HD constexpr int rev5(int x) {
    return ((x & 1) << 4) | ((x & 2) << 2) | (x & 4) | ((x & 8) >> 2) | ((x & 16) >> 4);
}
// offset of stage s (1-based) inside the concatenated twiddle table of precompute_twiddles()
FE_HD constexpr int tw_off(int s) { return (1 << (s - 1)) - 1; }

// explicit roundings: the translation unit is built with -ffp-contract=off, fma only where written.
FE_HD float fmul(float a, float b) { return a * b; }
FE_HD float fadd(float a, float b) { return a + b; }
FE_HD float fsub(float a, float b) { return a - b; }
FE_HD float ffma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
typedef float cf __attribute__((ext_vector_type(2)));
FE_HD cf cmk(float re, float im) { return (cf){re, im}; }
FE_HD cf cadd(cf a, cf b) { return a + b; }
FE_HD cf csub(cf a, cf b) { return a - b; }
FE_HD cf cmulv(cf a, cf b) { return a * b; }  // element-wise
FE_HD cf cfmav(cf a, cf b, cf c) { return __builtin_elementwise_fma(a, b, c); }
FE_HD cf cswap(cf a) { return a.yx; }
FE_HD cf cxx(cf a) { return a.xx; }
#else
struct cf {
    float x, y;
};
FE_HD cf cmk(float re, float im) { return cf{re, im}; }
FE_HD cf cadd(cf a, cf b) { return cf{a.x + b.x, a.y + b.y}; }
FE_HD cf csub(cf a, cf b) { return cf{a.x - b.x, a.y - b.y}; }
FE_HD cf cmulv(cf a, cf b) { return cf{a.x * b.x, a.y * b.y}; }
FE_HD cf cfmav(cf a, cf b, cf c) { return cf{__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y)}; }
FE_HD cf cswap(cf a) { return cf{a.y, a.x}; }
FE_HD cf cxx(cf a) { return cf{a.x, a.x}; }
#endif

// Twiddle in the two forms the butterfly consumes: w = (wr, wi) and wn = (-wi, wi).
struct Tw {
    cf w, wn;
};
FE_HD Tw make_tw(float wr, float wi) { return Tw{cmk(wr, wi), cmk(-wi, wi)}; }

// t = w * o with the reference's SIMD roundings (fft.rs:200-201):
//   t.re = fma(wr, o.re, -(wi*o.im))   t.im = fma(wr, o.im, wi*o.re)
FE_HD cf tw_mul_fma(const Tw& t, cf o) { return cfmav(cxx(t.w), o, cmulv(t.wn, cswap(o))); }

// Generic butterfly of the SIMD stages (fft.rs:200-208)
FE_HD void bfly_fma(const Tw& tw, cf& e, cf& o) {
    cf t = tw_mul_fma(tw, o);
    cf n = csub(e, t);
    e = cadd(e, t);
    o = n;
}
// Scalar-tail butterfly (fft.rs:236-250): both products rounded, then add/sub.
FE_HD void bfly_scalar(float wr, float wi, cf& e, cf& o) {
    float tr = fsub(fmul(wr, o.x), fmul(wi, o.y));
    float ti = fadd(fmul(wr, o.y), fmul(wi, o.x));
    cf t = cmk(tr, ti);
    cf n = csub(e, t);
    e = cadd(e, t);
    o = n;
}
// scalar-argument forms used by the generic any-n FFT kernel (features_ops.hip)
FE_HD void bfly_fma(float wr, float wi, float& er, float& ei, float& o_r, float& oi) {
    cf e = cmk(er, ei), o = cmk(o_r, oi);
    bfly_fma(make_tw(wr, wi), e, o);
    er = e.x;
    ei = e.y;
    o_r = o.x;
    oi = o.y;
}
FE_HD void bfly_scalar(float wr, float wi, float& er, float& ei, float& o_r, float& oi) {
    cf e = cmk(er, ei), o = cmk(o_r, oi);
    bfly_scalar(wr, wi, e, o);
    er = e.x;
    ei = e.y;
    o_r = o.x;
    oi = o.y;
}

// ---- phase A: stages 1..5 on the 32 register-resident points of one lane ---------------------------
// a[r] (r = 0..31).  On entry a[r] = (windowed sample n = 16*rev5(r)+p, 0); samples with rev5(r) >= 25 are 0.
// tw_re/tw_im: the reference's concatenated twiddle table (511 entries).
template <typename TW>
FE_HD void phase_a(cf* a, const TW& tw_re, const TW& tw_im) {
    // stage 1 (half 1, scalar path, w = table[0] = (1, -0))
#pragma unroll
    for (int r = 0; r < kRegs; r += 2) bfly_scalar(tw_re[tw_off(1)], tw_im[tw_off(1)], a[r], a[r + 1]);
    // stage 2 (half 2, scalar path)
#pragma unroll
    for (int b = 0; b < kRegs; b += 4) {
#pragma unroll
        for (int k = 0; k < 2; ++k) bfly_scalar(tw_re[tw_off(2) + k], tw_im[tw_off(2) + k], a[b + k], a[b + 2 + k]);
    }
    // stages 3..5 (half 4,8,16 -> SSE/AVX path with fma)
#pragma unroll
    for (int s = 3; s <= 5; ++s) {
        const int half = 1 << (s - 1);
#pragma unroll
        for (int b = 0; b < kRegs; b += 2 * half) {
#pragma unroll
            for (int k = 0; k < half; ++k)
                bfly_fma(make_tw(tw_re[tw_off(s) + k], tw_im[tw_off(s) + k]), a[b + k], a[b + half + k]);
        }
    }
}

// Same network with the structural zeros folded away (values identical to phase_a up to the sign of zeros):
//   * stage 1 and stage 2/k=0 use table[0] = table[1] = (1, -0): x*1 == x, x - (+-0) == x, so they are
//     real add/sub while the imaginary parts are still exactly zero;
//   * registers whose sample index 16*rev5(r)+p is >= 400 are the zero padding: stage-1 butterflies whose
//     odd input is padding reduce to copies (e + 0, e - 0);
//   * stage 2/k=1 and stage 3/k even have zero imaginary inputs: fma(w, 0, x) == x, w*0 == +-0.
//   * stage 4/k=0 and stage 5/k=0 use table[7] = table[15] = (1, -0) on complex inputs: t = (fma(1, or, -((-0)*oi)),
//     fma(1, oi, (-0)*or)) is o itself, except that a zero component of o may come out with the other sign
//     (-0 + +0 == +0).  So the butterfly is e + o, e - o: two packed instructions instead of four.  A zero's sign
//     cannot reach the result.  Call two finite values "alike" when they are equal or both zero.  Every operation
//     the network applies from here on (add, subtract, multiply, fma, negation) maps alike inputs to alike
//     outputs: a sum or fma whose other terms are not all zero does not see the sign of a zero term, and one whose
//     terms are all zero gives a zero of either sign; a product with a zero is a zero.  The network ends in the power
//     re*re + im*im (bin 256: re256*re256 + 0*0), which is +0 for a zero of either sign and equal for equal
//     values.  (Finite values: like the other folds here, this one does not reproduce the NaNs that 0 * inf makes
//     of a frame that has already overflowed.)
// REQUIRES tw_re[i]==1, tw_im[i]==+-0 for i = 0, 1, tw_off(4), tw_off(5) (checked on the host when tables are built).
// Input: x[r] real (r = 0..31, zero where rev5(r) >= 25).  Output: a[r] complex.
template <typename TW>
FE_HD void phase_a_fast(const float* x, cf* a, const TW& tw_re, const TW& tw_im) {
    float s1[kRegs];
    // stage 1
#pragma unroll
    for (int r = 0; r < kRegs; r += 2) {
        if (rev5(r + 1) >= kQ) {  // odd input is zero padding (compile-time condition)
            s1[r] = x[r];
            s1[r + 1] = x[r];
        } else {
            s1[r] = fadd(x[r], x[r + 1]);
            s1[r + 1] = fsub(x[r], x[r + 1]);
        }
    }
    // stage 2: k=0 real add/sub; k=1 twiddle table[2] on a real odd input
    {
        const float wr = tw_re[tw_off(2) + 1], wi = tw_im[tw_off(2) + 1];
#pragma unroll
        for (int b = 0; b < kRegs; b += 4) {
            a[b] = cmk(fadd(s1[b], s1[b + 2]), 0.0f);
            a[b + 2] = cmk(fsub(s1[b], s1[b + 2]), 0.0f);
            const float tr = fmul(wr, s1[b + 3]);  // wr*or - wi*0
            const float ti = fmul(wi, s1[b + 3]);  // wr*0 + wi*or
            a[b + 1] = cmk(fadd(s1[b + 1], tr), ti);   // (e + tr, 0 + ti)
            a[b + 3] = cmk(fsub(s1[b + 1], tr), -ti);  // (e - tr, 0 - ti)
        }
    }
    // stage 3: k = 0,2 have purely real inputs
#pragma unroll
    for (int b = 0; b < kRegs; b += 8) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float wr = tw_re[tw_off(3) + k], wi = tw_im[tw_off(3) + k];
            if ((k & 1) == 0) {
                const float e = a[b + k].x, o = a[b + 4 + k].x;
                const float tr = fmul(wr, o);  // fma(wr, or, -(wi*0))
                const float ti = fmul(wi, o);  // fma(wr, 0, wi*or)
                a[b + k] = cmk(fadd(e, tr), ti);
                a[b + 4 + k] = cmk(fsub(e, tr), -ti);
            } else {
                bfly_fma(make_tw(wr, wi), a[b + k], a[b + 4 + k]);
            }
        }
    }
#pragma unroll
    for (int s = 4; s <= 5; ++s) {
        const int half = 1 << (s - 1);
#pragma unroll
        for (int b = 0; b < kRegs; b += 2 * half) {
            {  // k = 0: w = (1, -0)
                const cf e = a[b], o = a[b + half];
                a[b] = cadd(e, o);
                a[b + half] = csub(e, o);
            }
#pragma unroll
            for (int k = 1; k < half; ++k)
                bfly_fma(make_tw(tw_re[tw_off(s) + k], tw_im[tw_off(s) + k]), a[b + k], a[b + half + k]);
        }
    }
}

// ---- phase A on real and conjugate values ----------------------------------------------------------
// The same network again, with two more kinds of work taken out.  Every register is in one of three classes:
//   real    -- the imaginary part is structurally zero (up to its sign): kept as ONE scalar, combined by real adds;
//   normal  -- the pair holds (re, im);
//   primed  -- the pair holds (re, -im), the conjugate of the value.
// Conjugation commutes with every rounding: a butterfly on two primed operands with the conjugate twiddle (wr, -wi) gives the
// conjugates of the normal butterfly's outputs bit for bit -- fma(wr, -oi, (-wi) * or) == -fma(wr, oi, wi * or), and so on down to
// e' +- t'.  The network ends in re * re + im * im, which does not see the sign of im, so nothing is ever flipped back: phase B reads
// conjugated twiddles in the lanes that hold primed values (tw_conj_image below) and the power is the same bits.
// Where classes come from: a butterfly of stage s at k = 0 has w = (1, -0) and, in phase A, two REAL inputs, so it is a real add and
// subtract (the "alike zeros" argument above covers the sign of the zero it no longer computes); at k = half / 2 it has two real inputs
// e, o and gives (e + wr * o, wi * o) and (e - wr * o, -(wi * o)): with nti = (-wi) * o == -(wi * o) the first is stored primed as
// (e + tr, nti), the second normal as (e - tr, nti) -- one product, no sign flip.  Every other butterfly keeps the class of its inputs.
// CLASS INVARIANT: both operands of every complex butterfly share a class (a primed register is never paired with a normal one), and
// the class a register has once it is complex is the class it ends with: primed(r).  Both are asserted below over every (s, b, k).
// Registers 0 and 16 end real (bins 0 and 256 come from them).
FE_HD constexpr bool primed(int r) { return r == 8 || ((0x2636 >> (r & 15)) & 1) != 0; }  // r % 16 in {1, 2, 4, 5, 9, 10, 13}, or r == 8
enum : int { kClsReal = 0, kClsNormal = 1, kClsPrimed = 2 };
// class of register r after stage s (1..5) of phase_a_conj, from the rules above alone
FE_HD constexpr int conj_class(int s, int r) {
    if (s <= 1) return kClsReal;
    const int half = 1 << (s - 1), k = r & (half - 1);
    if (k == 0) return kClsReal;
    if (k == half / 2 && conj_class(s - 1, r) == kClsReal) return (r & half) ? kClsNormal : kClsPrimed;
    return conj_class(s - 1, r);
}
FE_HD constexpr bool conj_classes_hold() {
    for (int s = 2; s <= 5; ++s) {
        const int half = 1 << (s - 1);
        for (int b = 0; b < kRegs; b += 2 * half)
            for (int k = 0; k < half; ++k) {
                const int ce = conj_class(s - 1, b + k), co = conj_class(s - 1, b + half + k);
                if (ce != co) return false;                                         // the operands of a butterfly share a class
                if ((k == 0 || k == half / 2) != (ce == kClsReal)) return false;   // real inputs exactly at k = 0 and k = half / 2
                if (ce != kClsReal && (ce == kClsPrimed) != primed(b + k)) return false;           // a complex register's class is final
                if (ce != kClsReal && (co == kClsPrimed) != primed(b + half + k)) return false;
            }
    }
    for (int r = 0; r < kRegs; ++r) {
        if ((conj_class(5, r) == kClsReal) != (r == 0 || r == 16)) return false;
        if ((conj_class(5, r) == kClsPrimed) != primed(r)) return false;
    }
    return true;
}
static_assert(conj_classes_hold(), "phase_a_conj never pairs a primed register with a normal one, and ends in primed(r)");

// REQUIRES what phase_a_fast requires of the table -- tw_re[i]==1, tw_im[i]==+-0 for i = 0, 1, tw_off(4), tw_off(5) -- and the same of entry
// tw_off(3): stage 3 at k = 0 is a bare add and subtract here, where phase_a_fast still multiplies by the entry.  (The nti fold at
// k = half / 2 holds for any table.)  precompute_twiddles gives (1, -0) at every one of them; a host caller with another table checks.  Input: x[r] real.  Output: a[r] = (re, primed(r) ? -im : im); a[0], a[16] = (re, 0).
template <typename TW>
FE_HD void phase_a_conj(const float* x, cf* a, const TW& tw_re, const TW& tw_im) {
    float s1[kRegs];
    // stage 1, as in phase_a_fast
#pragma unroll
    for (int r = 0; r < kRegs; r += 2) {
        if (rev5(r + 1) >= kQ) {
            s1[r] = x[r];
            s1[r + 1] = x[r];
        } else {
            s1[r] = fadd(x[r], x[r + 1]);
            s1[r + 1] = fsub(x[r], x[r + 1]);
        }
    }
    float re[kRegs];  // the registers that are real at this point of the network (the others' entries are unused)
    // stage 2: k = 0 real; k = 1 = half / 2 on a real odd input
    {
        const float wr = tw_re[tw_off(2) + 1], nwi = -tw_im[tw_off(2) + 1];
#pragma unroll
        for (int b = 0; b < kRegs; b += 4) {
            re[b] = fadd(s1[b], s1[b + 2]);
            re[b + 2] = fsub(s1[b], s1[b + 2]);
            const float tr = fmul(wr, s1[b + 3]);
            const float nti = fmul(nwi, s1[b + 3]);
            a[b + 1] = cmk(fadd(s1[b + 1], tr), nti);  // primed
            a[b + 3] = cmk(fsub(s1[b + 1], tr), nti);  // normal
        }
    }
#pragma unroll
    for (int s = 3; s <= 5; ++s) {
        const int half = 1 << (s - 1);
#pragma unroll
        for (int b = 0; b < kRegs; b += 2 * half) {
#pragma unroll
            for (int k = 0; k < half; ++k) {
                const int i = b + k, j = b + half + k;
                if (k == 0) {  // w = (1, -0) on two real values
                    const float e = re[i], o = re[j];
                    re[i] = fadd(e, o);
                    re[j] = fsub(e, o);
                } else if (k == half / 2) {  // two real values
                    const float wr = tw_re[tw_off(s) + k], nwi = -tw_im[tw_off(s) + k];
                    const float e = re[i], o = re[j];
                    const float tr = fmul(wr, o);    // fma(wr, or, -(wi * 0))
                    const float nti = fmul(nwi, o);  // -fma(wr, 0, wi * or)
                    a[i] = cmk(fadd(e, tr), nti);  // primed
                    a[j] = cmk(fsub(e, tr), nti);  // normal
                } else {
                    const float wr = tw_re[tw_off(s) + k], wi = tw_im[tw_off(s) + k];
                    bfly_fma(make_tw(wr, primed(i) ? -wi : wi), a[i], a[j]);
                }
            }
        }
    }
    a[0] = cmk(re[0], 0.0f);
    a[16] = cmk(re[16], 0.0f);
}

// The interleaved (re, im) twiddle table that phase B reads behind phase_a_conj: after the exchange lane c of round rho holds only
// values of class primed(16 * rho + c), and its twiddle index is tw_off(s) + 32 * k + 16 * rho + c with tw_off(s) + 1 a multiple of 32
// (s >= 6), so entry i >= 31 is conjugated exactly where primed((i + 1) & 31).  Entries below 31 (phase A's) are copied.
inline void tw_conj_image(const float* tw_re, const float* tw_im, int n, float* out /* 2 n */) {
    for (int i = 0; i < n; ++i) {
        out[2 * i] = tw_re[i];
        out[2 * i + 1] = (i >= tw_off(6) && primed((i + 1) & 31)) ? -tw_im[i] : tw_im[i];
    }
}

// ---- the entries phase_a_fast reads, as compile-time constants -------------------------------------
// Stages 2..5 use wave-uniform entries tw_off(2)+1, tw_off(3)+0..3, tw_off(4)+1..7 and tw_off(5)+1..15: 27 of the first 31
// table entries, the same in every pass of every launch.  Below are the f32 bit patterns of entries 0..30 as
// precompute_twiddles(512) gives them (cosf / sinf of the f32 angle); an accessor over them hands phase_a_fast literals, so the
// kernel fetches nothing for these stages.  The host compares them with the table it builds before it selects that form
// (tw_const_matches): a libm that rounds one entry differently keeps the table-reading kernel.
constexpr int kTwConstN = 31;
constexpr uint32_t kTwConstRe[kTwConstN] = {
    0x3f800000u, 0x3f800000u, 0xb33bbd2eu, 0x3f800000u, 0x3f3504f3u, 0xb33bbd2eu, 0xbf3504f3u, 0x3f800000u,
    0x3f6c835eu, 0x3f3504f3u, 0x3ec3ef15u, 0xb33bbd2eu, 0xbec3ef18u, 0xbf3504f3u, 0xbf6c8360u, 0x3f800000u,
    0x3f7b14beu, 0x3f6c835eu, 0x3f54db31u, 0x3f3504f3u, 0x3f0e39d9u, 0x3ec3ef15u, 0x3e47c5bcu, 0xb33bbd2eu,
    0xbe47c5c2u, 0xbec3ef18u, 0xbf0e39dcu, 0xbf3504f3u, 0xbf54db32u, 0xbf6c8360u, 0xbf7b14bfu};
constexpr uint32_t kTwConstIm[kTwConstN] = {
    0x80000000u, 0x80000000u, 0xbf800000u, 0x80000000u, 0xbf3504f3u, 0xbf800000u, 0xbf3504f3u, 0x80000000u,
    0xbec3ef16u, 0xbf3504f3u, 0xbf6c835eu, 0xbf800000u, 0xbf6c835eu, 0xbf3504f3u, 0xbec3ef10u, 0x80000000u,
    0xbe47c5c2u, 0xbec3ef16u, 0xbf0e39dau, 0xbf3504f3u, 0xbf54db32u, 0xbf6c835eu, 0xbf7b14bfu, 0xbf800000u,
    0xbf7b14beu, 0xbf6c835eu, 0xbf54db30u, 0xbf3504f3u, 0xbf0e39d9u, 0xbec3ef10u, 0xbe47c5c1u};
FE_HD bool tw_const_used(int i) {  // the 27 entries phase_a_fast reads
    return i == tw_off(2) + 1 || (i >= tw_off(3) && i < tw_off(4)) || (i > tw_off(4) && i < tw_off(5)) ||
           (i > tw_off(5) && i < kTwConstN);
}
struct TwConst {  // table accessor for phase_a_fast ({false}: real parts, {true}: imaginary): operator[] of a compile-time index is a literal
    bool im;
    FE_HD float operator[](int i) const { return __builtin_bit_cast(float, im ? kTwConstIm[i] : kTwConstRe[i]); }
};
// true where the table (tw_re, tw_im) holds exactly the constants at every entry phase_a_fast reads
inline bool tw_const_matches(const float* tw_re, const float* tw_im) {
    for (int i = 0; i < kTwConstN; ++i) {
        if (!tw_const_used(i)) continue;
        if (__builtin_bit_cast(uint32_t, tw_re[i]) != kTwConstRe[i] || __builtin_bit_cast(uint32_t, tw_im[i]) != kTwConstIm[i]) return false;
    }
    return true;
}

// ---- phase B: stages 6..9 on 16 points (register v = j[8:5]) of lane c, round rho -------------------
// Twiddles are per lane: index = tw_off(s) + (v mod 2^(s-6))*32 + rho*16 + c; TWF(i) returns (wr, wi) of entry i.
// After the call: b[v] for v<8 hold bins j = (2v+rho)*16 + c; *re256 = re of position 256 (meaningful for
// c==0, rho==0 only).
template <typename TWF>
FE_HD void phase_b(cf* b, int c, int rho, const TWF& twf, float* re256) {
#pragma unroll
    for (int s = 6; s <= 8; ++s) {
        const int hv = 1 << (s - 6);  // half size in units of v
#pragma unroll
        for (int k = 0; k < hv; ++k) {
            const cf w = twf(tw_off(s) + k * 32 + rho * 16 + c);
            const Tw tw = make_tw(w.x, w.y);
#pragma unroll
            for (int base = 0; base < 16; base += 2 * hv) bfly_fma(tw, b[base + k], b[base + hv + k]);
        }
    }
    // stage 9: pairs v and v+8.  Bins <256 are the even ('+') outputs.
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const cf w = twf(tw_off(9) + k * 32 + rho * 16 + c);
        const cf t = tw_mul_fma(make_tw(w.x, w.y), b[8 + k]);
        if (k == 0) *re256 = fsub(b[0].x, t.x);  // position 256 = odd output of the k=0 butterfly
        b[k] = cadd(b[k], t);
    }
}


// power spectrum exactly as features/pipeline.rs:165-169 after kernels/fft.rs:256-265 forced
// im[0] = im[256] = 0:  re*re + im*im  (two products, one add, no fma).
FE_HD float power(float re, float im) { return fadd(fmul(re, re), fmul(im, im)); }
FE_HD float power(cf z) {
    cf sq = cmulv(z, z);
    return fadd(sq.x, sq.y);
}

// LDS slot (in 8-byte units) of element (v = writer h, c) of one round of the exchange, per frame.
// Row pitch 17 slots (136 B = 34 banks): the 16 writers (lanes h, fixed c) land on banks 2h (+1), the 16
// readers (lanes c, fixed v) read consecutive slots -- both conflict-free, and every address is
// lane_base + compile-time immediate (no per-access address arithmetic).
constexpr int kXchgPitch = 17;
FE_HD constexpr int xchg_slot(int v, int c) { return v * kXchgPitch + c; }

// LDS image of the default mel bank's weights (80 filters = 5 rounds of 3, 4, 6, 10, 17 steps: 40 weights a lane, 640 in all).
// Weight s (0..39, rounds back to back) of lane p sits at word mel_lds_index(s, p): chunk j = s / 4 holds weights 4j .. 4j+3 of every
// lane, 16 bytes a lane, lanes consecutive.  A lane reads a chunk with one 16-byte load at lane_base + 256 j bytes; the 16 lanes of a
// frame then cover 64 consecutive words, every bank once (the four frames of a wave read the same addresses).
constexpr int kMelLdsWeights = 40;
constexpr int kMelLdsChunks = kMelLdsWeights / 4;
FE_HD constexpr int mel_lds_index(int s, int p) { return ((s >> 2) * kLanes + p) * 4 + (s & 3); }

// ---- which fused kernel a front-end runs (host) ------------------------------------------------------
// The template tuple <MODE, STDMEL, FUSED, OPT> of fe_main_kernel / fe_seg_main_kernel / fe_stream_main_kernel (frontend.hip describes
// the parameters).  opt is a chain: each bit is a form of the kernel with every lower bit set.
constexpr int kFeConstTw = 1, kFeLdsMel = 2, kFeLeanLds = 4, kFeConjA = 8;
struct FeForm {
    int mode;      // 1: the lane rotation is a DPP row_ror, 0: __shfl
    bool std_mel;  // the mel bank has the default round structure
    bool fused;    // the frame sums are computed inside the kernel
    int opt;       // kFe* bits; non-zero only with mode == 1, std_mel and fused
};
// The one statement of the selection rule.  std_mel: the bank has the default round structure; const_match: the twiddle table holds the
// compiled-in constants (tw_const_matches); const_tw, lds_tables, lean, conj: the product switches LELE_HIP_FE_CONST_TW / _LDS_TABLES /
// _LEAN_LDS / _CONJ_A; dpp, fused: the lab values LELE_HIP_FE_DPP / _FUSED (1 and true outside the lab build).
inline FeForm select_form(bool std_mel, bool const_match, bool const_tw, bool lds_tables, bool lean, bool conj, int dpp, bool fused) {
    FeForm f{dpp == 1 ? 1 : 0, std_mel, fused, 0};
    if (const_match && const_tw && std_mel && fused && dpp == 1) {
        f.opt = kFeConstTw | (lds_tables ? kFeLdsMel : 0);
        if (f.opt == (kFeConstTw | kFeLdsMel) && lean) f.opt |= kFeLeanLds | (conj ? kFeConjA : 0);
    }
    return f;
}

}  // namespace fe
